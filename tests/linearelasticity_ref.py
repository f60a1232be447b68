"""The yardstick of the linearelasticity block (MHA_PHYSICS_LINEARELASTICITY): the reference's volume and boundary loop
nests restated on the numpy forward-AD class of tests/oracle_lib.py, with derivative arrays of width n = dofs per element.

TEST INFRASTRUCTURE (the checker), imported by tests/test_linearelasticity.py and tests/test_linearelasticity_gpu.py only.
Built on the unchanged oracle's bases, quadrature and side geometry (physical_basis_var, physical_side_basis).

  * seeding: Workset::computeSolnTransientSeeded, seedwhat 1 (src/tools/workset.cpp:589-623);
  * linearelasticity::computeStress (src/physics/linearelasticity.cpp:913-1099), the Lame form and incplanestress;
  * linearelasticity::volumeResidual (:92-240);
  * linearelasticity::boundaryResidual (:244-672): Neumann and weak Dirichlet, the b vectors line by line as written
    (:379-386, 437-443 in 2-D, :501-509, 565-573, 628-636 in 3-D);
  * getWeightedMass (the mass mode), the L2 error of postprocessManager.cpp:1255-1268;
  * the scatter of assemblyManager.cpp:4031-4145 (ns_thermal_ref.scatter).

Variables: dx, dy[, dz] (linearelasticity.cpp:28-39).  A function is a number, ("sinprod", amp, freq), ("array", a) or a
deck string in x, y, z, t and the other named strings of `functions` (oracle_lib.deck_eval_ad).
"""
import os

import numpy as np

from ns_thermal_ref import RTOL, crs_err, rel_err, scatter, transient_state, warp  # noqa: F401  (re-exported)

FUNC_DEFAULTS = {"lambda": 1.0, "mu": 0.5, "source dx": 0.0, "source dy": 0.0, "source dz": 0.0}
PARAM_DEFAULTS = {"incplanestress": 0, "form_param": 1.0, "penalty": 10.0}
NAMES = ["dx", "dy", "dz"]
BC_NEUMANN, BC_WEAK_DIRICHLET = 1, 2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")


def le_mesh(oracle, dim, ncell, order, do_warp=True):
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * dim, [order] * dim)
    return warp(m) if do_warp else m


def func_at(oracle, spec, ip, elems=None, functions=None, nrm=None):
    """A named function at points ip [E][q][dim] -> [E][q]."""
    E, nq, dim = ip.shape
    if isinstance(spec, str):
        fields = {c: ip[..., d] for d, c in enumerate("xyz"[:dim])}
        fields["t"] = np.zeros((E, nq))
        if nrm is not None:
            fields.update({"n" + c: nrm[..., d] for d, c in enumerate("xyz"[:dim])})
        return np.broadcast_to(np.asarray(oracle.deck_eval_ad(spec, fields, functions), dtype=np.float64), (E, nq)).copy()
    if isinstance(spec, (int, float)):
        return np.full((E, nq), float(spec))
    if spec[0] == "sinprod":
        v = np.full((E, nq), float(spec[1]))
        for d in range(dim):
            v = v * np.sin(spec[2][d] * ip[..., d])
        return v
    if spec[0] == "array":
        a = np.asarray(spec[1], dtype=np.float64)
        return a if elems is None else a[elems]
    raise ValueError(spec)


def _alphas(transient):
    if transient is None:
        return 1.0, 0.0
    t = transient
    st = t["stage"]
    return t["butcher_A"][st, st] / t["butcher_b"][st], t["bdf"][0] / t["dt"] / t["butcher_b"][st]


def seeded_values(u, rows, transient):
    """The stage solution at the dofs `rows` (the .val() of the seeded AD values)."""
    cu = u[rows]
    if transient is None:
        return cu
    t = transient
    A, b, st = t["butcher_A"], t["butcher_b"], t["stage"]
    alpha_u = A[st, st] / b[st]
    up, us = t["u_prev"][rows], t["u_stage"][rows]
    beta_u = (1.0 - alpha_u) * up[..., 0]
    for s in range(st):
        beta_u = beta_u + A[st, s] / b[s] * (us[..., s] - up[..., 0])
    return alpha_u * cu + beta_u


def seeded_fields(oracle, m, u, transient, lids, B, G):
    """Displacements and their gradients at the points of B [E][card][q], G [E][card][q][dim] as ADViews of width n."""
    AD = oracle.ADView
    dim = m["dim"]
    E, n = lids.shape
    nq = B.shape[2]
    alpha_u, _ = _alphas(transient)
    val, grad, offs = [], [], []
    for v in range(dim):
        off = np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]])
        sv = seeded_values(u, lids[:, off], transient)

        def field(T):
            dx = np.zeros((E, nq, n))
            dx[:, :, off] = alpha_u * np.transpose(T, (0, 2, 1))
            return AD(np.einsum("ej,ejq->eq", sv, T), dx)
        val.append(field(B))
        grad.append([field(G[..., d]) for d in range(dim)])
        offs.append(off)
    return val, grad, offs


def stress(dim, gu, lam, mu, plane_stress=False):
    """computeStress (linearelasticity.cpp:985-1073): sigma[d][j] from the gradient fields gu[d][j]."""
    if dim == 2 and plane_stress:  # :990-1000
        return [[gu[0][0] * (4.0 * mu) + gu[1][1] * (2.0 * mu), (gu[0][1] + gu[1][0]) * mu],
                [(gu[0][1] + gu[1][0]) * mu, gu[1][1] * (4.0 * mu) + gu[0][0] * (2.0 * mu)]]
    S = [[None] * dim for _ in range(dim)]
    for d in range(dim):
        for j in range(dim):
            if d == j:
                other = None
                for k in range(dim):
                    if k != d:
                        other = gu[k][k] if other is None else other + gu[k][k]
                S[d][j] = gu[d][d] * (2.0 * mu + lam) + other * lam
            else:
                S[d][j] = (gu[d][j] + gu[j][d]) * mu
    return S


def _settings(funcs, params):
    fs = dict(FUNC_DEFAULTS)
    fs.update(funcs or {})
    assert set(fs) == set(FUNC_DEFAULTS), set(fs) - set(FUNC_DEFAULTS)
    P = dict(PARAM_DEFAULTS)
    P.update(params or {})
    assert set(P) == set(PARAM_DEFAULTS), set(P) - set(PARAM_DEFAULTS)
    return fs, P


def _add_rows(R, J, off, B, G, Fv, Fg):
    """res(elem, off(dof)) += sum_pt Fv basis + sum_d Fg[d] basis_grad[d]   (weights already in Fv, Fg)"""
    rv = np.einsum("eq,ejq->ej", Fv.val, B)
    rdx = np.einsum("eqw,ejq->ejw", Fv.dx, B)
    for d, fg in enumerate(Fg):
        if fg is None:
            continue
        rv = rv + np.einsum("eq,ejq->ej", fg.val, G[..., d])
        rdx = rdx + np.einsum("eqw,ejq->ejw", fg.dx, G[..., d])
    R[:, off] += rv
    J[:, off, :] += rdx


def element_arrays(oracle, m, qdeg, u, *, funcs=None, params=None, transient=None, elems=None, functions=None):
    """volumeResidual: res(elem, pos) and its derivative array -> (R [E][n], J [E][n][n]) in LID-position order + fields."""
    AD = oracle.ADView
    dim, order = m["dim"], int(m["orders"][0])
    assert all(int(o) == order for o in m["orders"])
    elems = np.arange(m["nelem"]) if elems is None else np.asarray(elems)
    lids = m["lids"][elems]
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, m["nodes"][elems])
    B, G, w, ip = pb["basis"][..., 0], pb["grad"], pb["wts"], pb["ip"]
    fs, P = _settings(funcs, params)
    val, gu, offs = seeded_fields(oracle, m, u, transient, lids, B, G)
    E, n = lids.shape
    fv = {k: func_at(oracle, s, ip, elems, functions) for k, s in fs.items()}
    S = stress(dim, gu, fv["lambda"], fv["mu"], bool(P["incplanestress"]))
    R, J = np.zeros((E, n)), np.zeros((E, n, n))
    for d in range(dim):
        src = AD(-fv["source " + NAMES[d]] * w, W=n)
        _add_rows(R, J, offs[d], B, G, src, [S[d][j] * w for j in range(dim)])
    F = dict(val=val, grad=gu, B=B, G=G, off=offs, wts=w, ip=ip, lids=lids, elems=elems)
    return R, J, F


def assemble(oracle, m, qdeg, u, *, funcs=None, params=None, fixed=None, transient=None, rowptr=None, colind=None,
             elems=None, functions=None):
    """The block's res / crs_vals / local_J / local_res (elems: a subset -> the local arrays of those elements only)."""
    R, J, F = element_arrays(oracle, m, qdeg, u, funcs=funcs, params=params, transient=transient, elems=elems,
                             functions=functions)
    out = dict(local_res=-R, local_J=J, fields=F)
    if elems is None:
        out.update(scatter(m, R, J, F["lids"], fixed, rowptr, colind, oracle))
    return out


def boundary_arrays(oracle, m, qdeg, u, belem, bside, bc_type, data, *, funcs=None, params=None, transient=None,
                    functions=None):
    """boundaryResidual on the entries (belem, bside), every component with the condition bc_type; data[d] = the function
    "Neumann d* <side>" / "Dirichlet d* <side>" ([K][q] arrays allowed).  -> (R [K][n], J [K][n][n])."""
    AD = oracle.ADView
    dim, order = m["dim"], int(m["orders"][0])
    belem = np.asarray(belem)
    lids = m["lids"][belem]
    K, n = lids.shape
    sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], belem, bside)
    B, G, w, ip, nrm = sb["basis"], sb["basis_grad"], sb["wts"], sb["ip"], sb["normals"]
    fs, P = _settings(funcs, params)
    src = [func_at(oracle, data[d], ip, None, functions, nrm) for d in range(dim)]
    R, J = np.zeros((K, n)), np.zeros((K, n, n))
    val, gu, offs = seeded_fields(oracle, m, u, transient, lids, B, G)
    if bc_type == BC_NEUMANN:  # :361-371, 419-429, 482-492, 546-556, 609-619
        for d in range(dim):
            _add_rows(R, J, offs[d], B, G, AD(-src[d] * w, W=n), [None] * dim)
        return R, J
    assert bc_type == BC_WEAK_DIRICHLET
    lam, mu = func_at(oracle, fs["lambda"], ip, None, functions, nrm), func_at(oracle, fs["mu"], ip, None, functions, nrm)
    S = stress(dim, gu, lam, mu, bool(P["incplanestress"]))
    h = w.sum(axis=1) ** (1.0 / (dim - 1))                              # Workset::getSideElementSize
    penalty = float(P["penalty"]) * (lam + 2.0 * mu) / h[:, None]
    fp = float(P["form_param"])
    dl = [val[d] - src[d] for d in range(dim)]                          # deltadx, deltady[, deltadz]
    nx, ny = nrm[..., 0], nrm[..., 1]
    if dim == 2:
        b = [[dl[0] * ((lam + 2.0 * mu) * nx) + dl[1] * (lam * ny), dl[1] * (mu * nx) + dl[0] * (mu * ny)],              # :382-383
             [dl[1] * (mu * nx) + dl[0] * (mu * ny), dl[0] * (lam * nx) + dl[1] * ((lam + 2.0 * mu) * ny)]]              # :440-441
    else:
        nz = nrm[..., 2]
        b = [[dl[0] * ((lam + 2.0 * mu) * nx) + dl[1] * (lam * ny) + dl[2] * (lam * nz),                                # :505-507
              dl[1] * (mu * nx) + dl[0] * (mu * ny), dl[2] * (mu * nx) + dl[0] * (mu * nz)],
             [dl[1] * (mu * nx) + dl[0] * (mu * ny),                                                                     # :569-571
              dl[0] * (lam * nx) + dl[1] * ((lam + 2.0 * mu) * ny) + dl[2] * (lam * nz), dl[2] * (mu * ny) + dl[1] * (mu * nz)],
             [dl[2] * (mu * nx) + dl[0] * (mu * nz), dl[2] * (mu * ny) + dl[1] * (mu * nz),                              # :632-634
              dl[0] * (lam * nx) + dl[1] * (lam * ny) + dl[2] * ((lam + 2.0 * mu) * nz)]]
    for d in range(dim):
        sn = None
        for j in range(dim):
            t = S[d][j] * nrm[..., j]
            sn = t if sn is None else sn + t
        Fv = (dl[d] * penalty - sn) * w
        _add_rows(R, J, offs[d], B, G, Fv, [b[d][j] * (-fp * w) for j in range(dim)])
    return R, J


def add_boundary(oracle, m, qdeg, u, ref, belem, bside, bc_type, data, *, fixed=None, **kw):
    """Accumulates one boundary group on top of an assembled dict(res, crs_vals, rowptr, colind); returns a new dict."""
    R, J = boundary_arrays(oracle, m, qdeg, u, belem, bside, bc_type, data, **kw)
    g = scatter(m, R, J, m["lids"][np.asarray(belem)], fixed, ref["rowptr"], ref["colind"])
    return dict(ref, res=ref["res"] + g["res"], crs_vals=ref["crs_vals"] + g["crs_vals"])


def get_mass(oracle, m, qdeg, masswts=None):
    """getWeightedMass: dense element matrices [E][n][n] in LID-position order, masswts[v] (value, v) blocks."""
    dim, order = m["dim"], int(m["orders"][0])
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, m["nodes"])
    B, w = pb["basis"][..., 0], pb["wts"]
    E, n = m["lids"].shape
    M = np.zeros((E, n, n))
    blockm = np.einsum("eiq,ejq,eq->eij", B, B, w)
    for v in range(dim):
        off = np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]])
        M[:, off[:, None], off[None, :]] = (1.0 if masswts is None else masswts[v]) * blockm
    return M


def l2_errors(oracle, m, qdeg, u, true_solutions, functions=None):
    """sqrt(sum_elem sum_pt (sol - true)^2 wts) per variable (postprocessManager.cpp:1255-1268)."""
    dim, order = m["dim"], int(m["orders"][0])
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, m["nodes"])
    B, w, ip = pb["basis"][..., 0], pb["wts"], pb["ip"]
    errs = []
    for v in range(dim):
        off = np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]])
        sol = np.einsum("ej,ejq->eq", u[m["lids"][:, off]], B)
        diff = sol - func_at(oracle, true_solutions[v], ip, None, functions)
        errs.append(float(np.sqrt((diff * diff * w).sum())))
    return errs


def read_deck(name):
    """The parts of a mirrored reference deck the yardstick reads: mesh sizes, the Functions strings (verbatim), the
    orders, the quadrature degree and the true solutions."""
    deck = dict(functions={}, true={}, mesh={}, order={}, quadrature=None)
    section, sub = None, None
    for raw in open(os.path.join(GOLD, name)):
        line = raw.rstrip("\n")
        if not line.strip() or line.strip() in ("---", "...") or line.startswith("%"):
            continue
        indent = len(line) - len(line.lstrip())
        key, _, value = line.strip().partition(":")
        value = value.strip().strip("'")
        if indent == 2:
            section, sub = key, None
            continue
        if section == "Mesh" and value:
            deck["mesh"][key] = value
        elif section == "Functions" and value:
            deck["functions"][key] = value
        elif section == "Discretization":
            if key == "quadrature":
                deck["quadrature"] = int(value)
            elif key == "order":
                sub = "order"
            elif sub == "order" and value:
                deck["order"][key] = int(value)
        elif section == "Postprocess":
            if key == "True solutions":
                sub = "true"
            elif sub == "true" and value:
                deck["true"][key] = value
    return deck


def gold_errors(name):
    """The printed L2 errors of a mirrored mrhyde.gold -> {variable: text}."""
    out = {}
    for line in open(os.path.join(GOLD, name)):
        if "L2 norm of the error for" in line:
            var, _, rest = line.split("for ")[1].partition(" = ")
            out[var.strip()] = rest.split()[0]
    return out


def solve_deck(oracle, deck):
    """Assemble the manufactured-solution deck with the restatement (strong Dirichlet rows with unit diagonal, zero data),
    solve with scipy and return the L2 errors of the variables."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    dim = int(deck["mesh"]["dimension"])
    ncell = tuple(int(deck["mesh"][k]) for k in ("NX", "NY", "NZ")[:dim])
    order, qdeg = deck["order"]["dx"], deck["quadrature"]
    assert all(deck["order"][v] == order for v in NAMES[:dim])
    m = le_mesh(oracle, dim, ncell, order, do_warp=False)
    fn = deck["functions"]
    funcs = {k: fn[k] for k in FUNC_DEFAULTS if k in fn}
    named = {k: v for k, v in fn.items() if k not in funcs}
    named.update({k: fn[k] for k in ("lambda", "mu")})
    fixed = (m["side_mask"] != 0).astype(np.uint8)
    ref = assemble(oracle, m, qdeg, np.zeros(m["ndof"]), funcs=funcs, fixed=fixed, functions=named)
    vals = ref["crs_vals"].copy()
    oracle.apply_dbc_diag(fixed, ref["rowptr"], ref["colind"], vals)
    A = sp.csr_matrix((vals, ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2)
    u = spla.spsolve(A.tocsc(), ref["res"])                       # J du = -res at u = 0; the problem is linear
    true = [deck["true"][v] for v in NAMES[:dim]]
    return l2_errors(oracle, m, qdeg, u, true, named)
