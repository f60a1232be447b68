"""The yardstick of the coupled linearelasticity + thermal block (MHA_PHYSICS_LINEARELASTICITY_THERMAL) and of the stress
output of both elasticity blocks: the reference's loop nests restated on the numpy forward-AD class of tests/oracle_lib.py,
with derivative arrays of width n = dofs per element.

TEST INFRASTRUCTURE (the checker), imported by tests/test_thermoelastic.py and tests/test_thermoelastic_gpu.py only.  Built
from tests/linearelasticity_ref.py (stress, seeded_fields, _add_rows, func_at, scatter) and the unchanged oracle's bases.

  * linearelasticity::setWorkset (src/physics/linearelasticity.cpp:860-906): e_num >= 0 when the block holds "e";
  * linearelasticity::computeStress with the e term (:913-1276): every normal stress gets -alpha_T (e - T_ambient) c,
    c = 3 lambda + 2 mu (:1024-1034, 1074-1084), c = 5 mu under incplanestress in 2-D (:1001-1011);
  * linearelasticity::volumeResidual (:92-240) on the displacement rows, thermal::volumeResidual without have_nsvel
    (src/physics/thermal.cpp:125-163) on the e row;
  * linearelasticity::getDerivedValues (:1301-1360): "VM stress", "MAG stress".

Variables: dx, dy[, dz], e (the displacements of one order, e of its own).  Functions as in linearelasticity_ref.
"""
import os

import numpy as np

import linearelasticity_ref as LE
from linearelasticity_ref import GOLD, NAMES, RTOL, crs_err, rel_err, scatter, transient_state, warp  # noqa: F401

FUNC_DEFAULTS = {"lambda": 1.0, "mu": 0.5, "source dx": 0.0, "source dy": 0.0, "source dz": 0.0, "thermal source": 0.0,
                 "thermal diffusion": 1.0, "specific heat": 1.0, "density": 1.0, "bx": 0.0, "by": 0.0, "bz": 0.0}
PARAM_DEFAULTS = {"incplanestress": 0, "T_ambient": 0.0, "alpha_T": 1.0e-6, "include advection": 0, "form_param": 1.0,
                  "penalty": 10.0}


def coupled_mesh(oracle, dim, ncell, orders, do_warp=True):
    """orders = (displacements, e) -> mesh_multi of dx, dy[, dz], e."""
    od, oe = orders
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * (dim + 1), [od] * dim + [oe])
    return warp(m) if do_warp else m


def var_names(dim):
    return NAMES[:dim] + ["e"]


def var_off(m, v):
    return np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]])


def var_rows(m, v):
    return np.unique(m["lids"][:, var_off(m, v)])


def _settings(funcs, params):
    fs = dict(FUNC_DEFAULTS)
    fs.update(funcs or {})
    assert set(fs) == set(FUNC_DEFAULTS), set(fs) - set(FUNC_DEFAULTS)
    P = dict(PARAM_DEFAULTS)
    P.update(params or {})
    assert set(P) == set(PARAM_DEFAULTS), set(P) - set(PARAM_DEFAULTS)
    return fs, P


def thermal_coefficient(lam, mu, dim, plane_stress):
    """c of the term -alpha_T (e - T_ambient) c: 3 lambda + 2 mu, and 5 mu under incplanestress (:1007-1008)."""
    return 5.0 * mu if (dim == 2 and plane_stress) else 3.0 * lam + 2.0 * mu


def e_fields(oracle, m, u, transient, lids, B, G):
    """e, its time derivative and gradient at the points of e's basis as ADViews of width n (computeSolnTransientSeeded)."""
    AD = oracle.ADView
    dim = m["dim"]
    E, n = lids.shape
    nq = B.shape[2]
    off = var_off(m, dim)
    rows = lids[:, off]
    alpha_u, alpha_t = LE._alphas(transient)
    sv = LE.seeded_values(u, rows, transient)
    if transient is None:
        sd = np.zeros_like(sv)
    else:
        t = transient
        timewt = 1.0 / t["dt"] / t["butcher_b"][t["stage"]]
        beta_t = np.zeros_like(sv)
        for s in range(1, len(t["bdf"])):
            beta_t = beta_t + t["bdf"][s] * t["u_prev"][rows][..., s - 1]
        sd = alpha_t * u[rows] + beta_t * timewt

    def field(coef, T, scale):
        dx = np.zeros((E, nq, n))
        dx[:, :, off] = scale * np.transpose(T, (0, 2, 1))
        return AD(np.einsum("ej,ejq->eq", coef, T), dx)
    return field(sv, B, alpha_u), field(sd, B, alpha_t), [field(sv, G[..., d], alpha_u) for d in range(dim)], off


def coupled_stress(dim, gu, T, lam, mu, P):
    """computeStress with e_num >= 0: the plain stress, then the thermoelastic term on the normal components."""
    ps = bool(P["incplanestress"])
    S = LE.stress(dim, gu, lam, mu, ps)
    if T is not None:
        th = (T - float(P["T_ambient"])) * (float(P["alpha_T"]) * thermal_coefficient(lam, mu, dim, ps))
        for d in range(dim):
            S[d][d] = S[d][d] - th
    return S


def element_arrays(oracle, m, qdeg, u, *, funcs=None, params=None, transient=None, elems=None, functions=None):
    """Both modules' volumeResidual: res(elem, pos) and its derivative array -> (R [E][n], J [E][n][n]) in LID-position
    order + the fields."""
    AD = oracle.ADView
    dim = m["dim"]
    od, oe = int(m["orders"][0]), int(m["orders"][dim])
    assert len(m["orders"]) == dim + 1 and all(int(o) == od for o in m["orders"][:dim])
    elems = np.arange(m["nelem"]) if elems is None else np.asarray(elems)
    lids = m["lids"][elems]
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, od, qdeg, m["nodes"][elems])
    pe = pb if oe == od else oracle.physical_basis_var(dim, oracle.HGRAD, oe, qdeg, m["nodes"][elems])
    B, G, w, ip = pb["basis"][..., 0], pb["grad"], pb["wts"], pb["ip"]
    Be, Ge = pe["basis"][..., 0], pe["grad"]
    fs, P = _settings(funcs, params)
    val, gu, offs = LE.seeded_fields(oracle, m, u, transient, lids, B, G)
    T, Tdot, gT, off_e = e_fields(oracle, m, u, transient, lids, Be, Ge)
    E, n = lids.shape
    fv = {k: LE.func_at(oracle, s, ip, elems, functions) for k, s in fs.items()}
    S = coupled_stress(dim, gu, T, fv["lambda"], fv["mu"], P)
    R, J = np.zeros((E, n)), np.zeros((E, n, n))
    for d in range(dim):
        src = AD(-fv["source " + NAMES[d]] * w, W=n)
        LE._add_rows(R, J, offs[d], B, G, src, [S[d][j] * w for j in range(dim)])
    # thermal (thermal.cpp:125-163): rho cp de/dt - source, kappa grad e, (b . grad e) with "include advection"
    Fv = (Tdot * (fv["density"] * fv["specific heat"]) - fv["thermal source"]) * w
    if P["include advection"]:
        for d, k in enumerate(["bx", "by", "bz"][:dim]):
            Fv = Fv + gT[d] * (fv[k] * w)
    LE._add_rows(R, J, off_e, Be, Ge, Fv, [gT[d] * (fv["thermal diffusion"] * w) for d in range(dim)])
    F = dict(val=val + [T], dot=[None] * dim + [Tdot], grad=gu + [gT], B=[B] * dim + [Be], G=[G] * dim + [Ge],
             off=offs + [off_e], wts=w, ip=ip, lids=lids, elems=elems, coef=fv)
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


def add_traction(oracle, m, qdeg, ref, belem, bside, data, fixed=None, functions=None):
    """A traction group (linearelasticity.cpp:361-371, ...) on the displacement rows of the coupled element: -g_d (N_a, 1)."""
    AD = oracle.ADView
    dim, od = m["dim"], int(m["orders"][0])
    belem = np.asarray(belem)
    lids = m["lids"][belem]
    K, n = lids.shape
    sb = oracle.physical_side_basis(dim, od, qdeg, m["nodes"], belem, bside)
    R, J = np.zeros((K, n)), np.zeros((K, n, n))
    for d in range(dim):
        g = LE.func_at(oracle, data[d], sb["ip"], None, functions, sb["normals"])
        LE._add_rows(R, J, var_off(m, d), sb["basis"], sb["basis_grad"], AD(-g * sb["wts"], W=n), [None] * dim)
    s = scatter(m, R, J, lids, fixed, ref["rowptr"], ref["colind"])
    return dict(ref, res=ref["res"] + s["res"], crs_vals=ref["crs_vals"] + s["crs_vals"])


def get_mass(oracle, m, qdeg, masswts=None):
    """getWeightedMass of the coupled block: [E][n][n] in LID-position order."""
    return oracle.get_mass(m, qdeg, masswts)


def derived(dim, S):
    """getDerivedValues (:1326-1354) of a stress given as nested lists of arrays -> (VM, MAG)."""
    if dim == 2:
        sxx, syy, sxy = S[0][0], S[1][1], S[0][1]
        return np.sqrt(sxx * sxx - sxx * syy + syy * syy + 3.0 * sxy * sxy), np.sqrt(sxx * sxx + syy * syy)
    sxx, syy, szz, sxy, syz, szx = S[0][0], S[1][1], S[2][2], S[0][1], S[1][2], S[2][0]
    vm = np.sqrt(0.5 * ((sxx - syy) ** 2 + (syy - szz) ** 2 + (szz - sxx) ** 2) + 3.0 * (sxy * sxy + syz * syz + szx * szx))
    return vm, np.sqrt(sxx * sxx + syy * syy + szz * szz)


def stress_output(oracle, m, qdeg, u, *, funcs=None, params=None, functions=None):
    """getDerivedValues on a plain (dim variables) or coupled (dim + 1) block from u as given.
    -> dict(stress [E][q][dim][dim], vm [E][q], mag [E][q])."""
    dim = m["dim"]
    has_e = len(m["orders"]) == dim + 1
    od = int(m["orders"][0])
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, od, qdeg, m["nodes"])
    B, G, ip = pb["basis"][..., 0], pb["grad"], pb["ip"]
    fs = dict(FUNC_DEFAULTS if has_e else LE.FUNC_DEFAULTS)
    fs.update(funcs or {})
    P = dict(PARAM_DEFAULTS)
    P.update(params or {})
    lids = m["lids"]
    gu = [[np.einsum("ej,ejq->eq", u[lids[:, var_off(m, v)]], G[..., d]) for d in range(dim)] for v in range(dim)]
    T = None
    if has_e:
        oe = int(m["orders"][dim])
        Be = B if oe == od else oracle.physical_basis_var(dim, oracle.HGRAD, oe, qdeg, m["nodes"])["basis"][..., 0]
        T = np.einsum("ej,ejq->eq", u[lids[:, var_off(m, dim)]], Be)
    lam, mu = LE.func_at(oracle, fs["lambda"], ip, None, functions), LE.func_at(oracle, fs["mu"], ip, None, functions)
    S = coupled_stress(dim, gu, T, lam, mu, P)
    vm, mag = derived(dim, S)
    return dict(stress=np.stack([np.stack(row, axis=-1) for row in S], axis=-2), vm=vm, mag=mag)


def dof_coordinates(oracle, m):
    """Positions of the dofs of an order-1 block [ndof][dim]: the coordinates are in the span of the order-1 basis, so
    sum_j X_j N_j(q) = x(q) at the 2^dim points of the degree-2 rule gives X."""
    dim = m["dim"]
    assert all(int(o) == 1 for o in m["orders"])
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, 1, 2, m["nodes"])
    B, ip = pb["basis"][..., 0], pb["ip"]
    X = np.linalg.solve(np.transpose(B, (0, 2, 1)), ip)
    x = np.zeros((m["ndof"], dim))
    for v in range(len(m["orders"])):
        x[m["lids"][:, var_off(m, v)]] = X
    return x


def l2_errors(oracle, m, qdeg, u):
    """sqrt(sum_elem sum_pt sol^2 wts) per variable: the L2 error against a zero true solution
    (postprocessManager.cpp:1255-1268)."""
    dim = m["dim"]
    errs = []
    for v in range(len(m["orders"])):
        pb = oracle.physical_basis_var(dim, oracle.HGRAD, int(m["orders"][v]), qdeg, m["nodes"])
        sol = np.einsum("ej,ejq->eq", u[m["lids"][:, var_off(m, v)]], pb["basis"][..., 0])
        errs.append(float(np.sqrt((sol * sol * pb["wts"]).sum())))
    return errs


def gold_series(name):
    """The printed L2 errors of the mirrored transient gold -> {variable: [text per printed time]}."""
    out = {}
    for line in open(os.path.join(GOLD, name)):
        if "L2 norm of the error for" in line:
            var, _, rest = line.split("for ")[1].partition(" = ")
            out.setdefault(var.strip(), []).append(rest.split()[0])
    return out


def run_deck_bwe(oracle, deck, assemble_step, nsteps=10, final_time=1.0):
    """regression/thermoelastic/2D_transient: backward Euler (Butcher 'BWE', BDF order 1), strong zero Dirichlet rows on
    every side and every variable, zero initial state.  assemble_step(m, qdeg, u, tr, fixed, funcs) -> (J csr with unit
    diagonal on the fixed rows, rhs).  -> (mesh, [errors of dx, dy, e per printed time])."""
    import scipy.sparse.linalg as spla
    dim = int(deck["mesh"]["dimension"])
    ncell = tuple(int(deck["mesh"][k]) for k in ("NX", "NY", "NZ")[:dim])
    od, oe, qdeg = deck["order"]["dx"], deck["order"]["e"], deck["quadrature"]
    m = coupled_mesh(oracle, dim, ncell, (od, oe), do_warp=False)
    funcs = {k: v for k, v in deck["functions"].items() if k in FUNC_DEFAULTS}
    for k in ("lambda", "mu"):
        funcs[k] = float(funcs[k])
    fixed = (m["side_mask"] != 0).astype(np.uint8)
    A, b, bdf = np.array([[1.0]]), np.array([1.0]), np.array([1.0, -1.0])
    dt = final_time / nsteps
    u = np.zeros(m["ndof"])
    series = [l2_errors(oracle, m, qdeg, u)]
    for _ in range(nsteps):
        u_prev = u.copy()
        for it in range(3):  # Newton: the problem is linear, the second pass only confirms convergence
            tr = dict(u_prev=u_prev[:, None].copy(), u_stage=u[:, None].copy(), stage=0, butcher_A=A, butcher_b=b, bdf=bdf,
                      dt=dt)
            J, rhs = assemble_step(m, qdeg, u, tr, fixed, funcs)
            if it > 0 and np.abs(rhs).max() < 1e-10:
                break
            u = u + spla.spsolve(J.tocsc(), rhs)
        series.append(l2_errors(oracle, m, qdeg, u))
    return m, series
