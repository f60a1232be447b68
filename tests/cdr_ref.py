"""The yardstick of the cdr module (MHA_PHYSICS_CDR) and of the c row of the coupled navierstokes + cdr block
(MHA_PHYSICS_NAVIERSTOKES_CDR): cdr::volumeResidual restated on the numpy forward-AD class of tests/oracle_lib.py.

TEST INFRASTRUCTURE (the checker), imported by tests/test_cdr.py and tests/test_cdr_gpu.py only.

  * seeding: Workset::computeSolnTransientSeeded, seedwhat 1 (src/tools/workset.cpp:589-623), through
    ns_thermal_ref.fields_at_points -- AD arrays as wide as the whole block, so a function that reads "ux" gives the
    c-row / ux-column entries;
  * the functions: FunctionManager<AD>::evaluate (oracle_lib.deck_eval_ad) for deck strings that may read the solution
    fields and other named functions; numbers, ("sinprod", amp, freq) and ("array", a) as the other yardsticks take them;
  * cdr::volumeResidual (src/physics/cdr.cpp:62-142): (c_t + v . grad c + reaction - source) v
    + 1 / (density specific heat) diffusion grad c . grad v; "SUPG tau" is accepted and, as in the reference, unused;
  * the navierstokes rows of the coupled block: the UNCHANGED oracle (assemble_block with PHYS_NAVIERSTOKES) on the same
    cells, mapped through the two LID tables (ns_thermal_ref.sub_mesh);
  * the scatter of assemblyManager.cpp:4031-4145 (ns_thermal_ref.scatter).
"""
import numpy as np

import ns_thermal_ref as N
from ns_thermal_ref import RTOL, crs_err, rel_err, transient_state, var_rows, warp  # noqa: F401  (re-exported)

# reference defaults (cdr.cpp:40-48)
FUNC_DEFAULTS = {"source": 0.0, "diffusion": 1.0, "specific heat": 1.0, "density": 1.0, "reaction": 1.0, "xvel": 1.0,
                 "yvel": 1.0, "zvel": 1.0, "SUPG tau": 0.0}
NS_FUNC_NAMES = ("source ux", "source pr", "source uy", "source uz", "density", "viscosity")


def var_names(dim, coupled):
    return (["ux", "pr", "uy"] + (["uz"] if dim == 3 else []) + ["c"]) if coupled else ["c"]


def cdr_mesh(oracle, dim, ncell, order, do_warp=True, hi=None):
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD], [order], hi=hi)
    return warp(m) if do_warp else m


def coupled_mesh(oracle, dim, ncell, orders, do_warp=True, hi=None):
    """orders = (velocity, pressure, c) -> mesh_multi of ux, pr, uy[, uz], c."""
    ov, op, oc = orders
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * (dim + 2), [ov, op] + [ov] * (dim - 1) + [oc], hi=hi)
    return warp(m) if do_warp else m


def field_dict(oracle, F, names, time=0.0):
    """Workset::getSolutionField names -> AD views: <v>, grad(<v>)[x|y|z], <v>_t, the coordinates and t."""
    n = F["n"]
    dim = F["ip"].shape[-1]
    fields = {}
    for v, nm in enumerate(names):
        fields[nm] = F["val"][v]
        fields[nm + "_t"] = F["dot"][v]
        for d, c in enumerate("xyz"[:dim]):
            fields["grad(%s)[%s]" % (nm, c)] = F["grad"][v][d]
    for d, c in enumerate("xyz"[:dim]):
        fields[c] = oracle.ADView(F["ip"][..., d], W=n)
    fields["t"] = oracle.ADView(np.full(F["wts"].shape, float(time)), W=n)
    # the known variables without data in a volume function: z on a 2-D block, the normal, and h, whose leaf the
    # reference never fills (functionManager.cpp:386-404)
    for c in ["z"][:3 - dim] + ["nx", "ny", "nz", "h"]:
        fields[c] = oracle.ADView(np.zeros(F["wts"].shape), W=n)
    return fields


def eval_function(oracle, spec, fields, strings, F):
    """One named function at the points as an AD view."""
    like = fields["t"]
    if isinstance(spec, str):
        return oracle.ADView._lift(oracle.deck_eval_ad(spec, fields, strings), like)
    return oracle.ADView._lift(N._func_at_ip(spec, F["ip"], F["elems"]), like)


def cdr_row(oracle, m, qdeg, u, *, funcs=None, transient=None, elems=None, time=0.0):
    """res(elem, off(c, dof)) and its derivative array -> (R [E][n], J [E][n][n]) in LID-position order (zero outside
    the c rows), plus the field dict.  c is the LAST variable of the mesh.  funcs may hold further deck strings
    (e.g. "bubble") that the module's functions name."""
    dim, nv = m["dim"], len(m["types"])
    coupled = nv > 1
    names = var_names(dim, coupled)
    assert len(names) == nv
    F = N.fields_at_points(oracle, m, qdeg, u, transient, elems)
    F["names"] = names
    E, n = F["lids"].shape
    w = F["wts"]
    fs = dict(FUNC_DEFAULTS)
    fs.update({k: v for k, v in (funcs or {}).items() if k not in NS_FUNC_NAMES or k == "density"})
    fields = field_dict(oracle, F, names, time)
    # what a deck string may name besides the fields: every other string or number of the deck
    strings = {k: (v if isinstance(v, str) else repr(float(v))) for k, v in fs.items() if isinstance(v, (str, int, float))}
    fv = {k: eval_function(oracle, fs[k], fields, strings, F) for k in FUNC_DEFAULTS}
    cv = nv - 1
    gc = F["grad"][cv]
    f = F["dot"][cv] + fv["reaction"] - fv["source"]
    for d, k in enumerate(["xvel", "yvel", "zvel"][:dim]):
        f = f + fv[k] * gc[d]
    kd = 1.0 / (fv["density"] * fv["specific heat"]) * fv["diffusion"]
    Fv, Fg = f * w, [kd * gc[d] * w for d in range(dim)]
    B, G, off = F["B"][cv], F["G"][cv], F["off"][cv]
    R, J = np.zeros((E, n)), np.zeros((E, n, n))
    rv = np.einsum("eq,ejq->ej", Fv.val, B)
    rdx = np.einsum("eqw,ejq->ejw", Fv.dx, B)
    for d in range(dim):
        rv = rv + np.einsum("eq,ejq->ej", Fg[d].val, G[..., d])
        rdx = rdx + np.einsum("eqw,ejq->ejw", Fg[d].dx, G[..., d])
    R[:, off] = rv
    J[:, off, :] = rdx
    return R, J, F


def assemble(oracle, m, qdeg, u, *, funcs=None, ns_params=(0, 0, 0), fixed=None, transient=None, rowptr=None,
             colind=None, time=0.0):
    """res / crs_vals of a cdr block (one variable) or of the coupled block (ux, pr, uy[, uz], c): the c row from cdr_row,
    the navierstokes rows from the oracle's navierstokes block on the same cells."""
    dim, nv = m["dim"], len(m["types"])
    R, J, F = cdr_row(oracle, m, qdeg, u, funcs=funcs, transient=transient, time=time)
    out = N.scatter(m, R, J, F["lids"], fixed, rowptr, colind, oracle)
    out["fields"] = F
    if nv == 1:
        return out
    ns, rows = N.sub_mesh(oracle, m, list(range(dim + 1)))
    nsf = {k: v for k, v in (funcs or {}).items() if k in NS_FUNC_NAMES}
    if dim == 2:
        nsf.pop("source uz", None)
    trn = None if transient is None else dict(transient, u_prev=transient["u_prev"][rows], u_stage=transient["u_stage"][rows])
    ref = oracle.assemble_block(ns, oracle.PHYS_NAVIERSTOKES, qdeg, u[rows], funcs=nsf, params=list(ns_params),
                                fixed=None if fixed is None else np.asarray(fixed)[rows], transient=trn)
    out["res"][rows] += ref["res"]
    ndof = m["ndof"]
    crs_rows = np.repeat(np.arange(ndof, dtype=np.int64), np.diff(out["rowptr"]))
    keys = crs_rows * ndof + np.asarray(out["colind"], dtype=np.int64)
    nrows = np.repeat(np.arange(len(rows), dtype=np.int64), np.diff(ref["rowptr"]))
    want = rows[nrows] * ndof + rows[np.asarray(ref["colind"], dtype=np.int64)]
    idx = np.searchsorted(keys, want)
    assert np.array_equal(keys[np.minimum(idx, len(keys) - 1)], want), "a navierstokes column is missing from the graph"
    np.add.at(out["crs_vals"], idx, ref["crs_vals"])
    out["ns_rows"], out["ns"] = rows, ref
    return out


def dense(ref, ndof):
    import scipy.sparse as sp
    return sp.csr_matrix((ref["crs_vals"], ref["colind"], ref["rowptr"]), shape=(ndof, ndof))


def l2_error(oracle, m, qdeg, u, v, true):
    """"L2 norm of the error" of variable v (postprocessManager.cpp:1255-1268); true: callable of the points [E][q][dim]."""
    pb = oracle.physical_basis_var(m["dim"], oracle.HGRAD, int(m["orders"][v]), qdeg, m["nodes"])
    ue = u[m["lids"][:, m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]]]
    uh = np.einsum("ef,efq->eq", ue, pb["basis"][..., 0])
    return float(np.sqrt(np.sum((uh - true(pb["ip"])) ** 2 * pb["wts"])))


def l2_projection(oracle, m, qdeg, v, data):
    """The L2 projection of data (callable of the points) onto variable v: consistent mass, direct solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    pb = oracle.physical_basis_var(m["dim"], oracle.HGRAD, int(m["orders"][v]), qdeg, m["nodes"])
    B, w = pb["basis"][..., 0], pb["wts"]
    rows = m["lids"][:, m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]].astype(np.int64)
    Me = np.einsum("eiq,ejq,eq->eij", B, B, w)
    be = np.einsum("eiq,eq->ei", B, data(pb["ip"]) * w)
    ndof = m["ndof"]
    card = rows.shape[1]
    M = sp.coo_matrix((Me.ravel(), (np.repeat(rows, card, axis=1).ravel(), np.tile(rows, (1, card)).ravel())),
                      shape=(ndof, ndof)).tocsr()
    rhs = np.zeros(ndof)
    np.add.at(rhs, rows, be)
    mine = np.unique(rows)
    out = np.zeros(ndof)
    out[mine] = spla.spsolve(M[mine][:, mine].tocsc(), rhs[mine])
    return out


BUBBLE_T = "-10.0*(x-0.2)*(x-0.2) - 10.0*(y-0.5)*(y-0.5)"
BUBBLE_NS = "-10.0*(x-2)*(x-2) - 10.0*(y-0.5)*(y-0.5)"
MANUFACTURED_SOURCE = ("(8*(pi*pi)+0.5*sin(2*pi*x)*sin(2*pi*y))*sin(2*pi*x)*sin(2*pi*y) + 2.0*2*pi*cos(2*pi*x)*sin(2*pi*y)"
                       " + 1.0*2*pi*sin(2*pi*x)*cos(2*pi*y)")
BE = dict(stage=0, butcher_A=np.array([[1.0]]), butcher_b=np.array([1.0]), bdf=np.array([1.0, -1.0]))


def newton(solve_step, u, iters, tol):
    """Newton from u: solve_step(u) -> (J csr with identity fixed rows, rhs = -res)."""
    import scipy.sparse.linalg as spla
    for it in range(iters):
        J, rhs = solve_step(u)
        if it > 0 and np.linalg.norm(rhs) < tol:
            break
        u = u + spla.spsolve(J.tocsc(), rhs)
    return u


def gold_manufactured(oracle, assemble_fn, ncell=(40, 40)):
    """regression/cdr/2D_manufactured: Q1, Newton from 0 (at most 4 steps), strong zero Dirichlet rows, 2x2 Gauss.
    assemble_fn(m, u, funcs, fixed, transient) -> (J csr, rhs)."""
    m = cdr_mesh(oracle, 2, ncell, 1, do_warp=False)
    fixed = (m["side_mask"] != 0).astype(np.uint8)
    funcs = {"source": MANUFACTURED_SOURCE, "xvel": 2.0, "yvel": 1.0, "reaction": "0.5*c*c"}
    u = newton(lambda u: assemble_fn(m, u, funcs, fixed, None), np.zeros(m["ndof"]), 4, 1e-12)
    return [l2_error(oracle, m, 2, u, 0, lambda x: np.sin(2 * np.pi * x[..., 0]) * np.sin(2 * np.pi * x[..., 1]))]


def gold_transient(oracle, assemble_fn, initial=None, ncell=(40, 40), nsteps=10):
    """regression/cdr/2D_transient: backward Euler, dt 1e-2; the initial state is the L2 projection of exp(bubble) with the
    boundary rows then set to 0.  initial(m) -> the projected state (default: the yardstick's own projection)."""
    m = cdr_mesh(oracle, 2, ncell, 1, do_warp=False)
    fixed = (m["side_mask"] != 0).astype(np.uint8)
    funcs = {"source": 0.0, "xvel": 10.0, "yvel": 0.0, "reaction": "0.5*c*c"}
    bub = lambda x: np.exp(-10.0 * (x[..., 0] - 0.2) ** 2 - 10.0 * (x[..., 1] - 0.5) ** 2)
    u = l2_projection(oracle, m, 2, 0, bub) if initial is None else initial(m)
    u[fixed != 0] = 0.0
    zero = lambda x: 0.0 * x[..., 0]
    errs = [l2_error(oracle, m, 2, u, 0, zero)]
    for _ in range(nsteps):
        tr = dict(BE, u_prev=u[:, None].copy(), dt=1e-2)

        def step(v, tr=tr):
            return assemble_fn(m, v, funcs, fixed, dict(tr, u_stage=v[:, None].copy()))
        u = newton(step, u.copy(), 10, 1e-10)
        errs.append(l2_error(oracle, m, 2, u, 0, zero))
    return errs


def gold_ns_coupled(oracle, assemble_fn, ncell=(50, 10)):
    """regression/cdr/2D_ns_coupled: 5x1 channel, Q1^4 + PSPG, ux = uy = c = 0 on top / bottom, coupled Newton from 0,
    direct solves."""
    m = coupled_mesh(oracle, 2, ncell, (1, 1, 1), do_warp=False, hi=[5.0, 1.0, 1.0])
    fixed = (((m["side_mask"] & 0b1100) != 0) & (m["dof_var"] != 1)).astype(np.uint8)
    funcs = {"source ux": 1.0, "source": "exp(bubble)", "diffusion": 0.01, "xvel": "ux", "yvel": "uy", "reaction": 0.0,
             "bubble": BUBBLE_NS}
    u = newton(lambda u: assemble_fn(m, u, funcs, fixed, None), np.zeros(m["ndof"]), 4, 1e-12)
    true = {0: lambda x: 0.5 * x[..., 1] * (1 - x[..., 1])}
    zero = lambda x: 0.0 * x[..., 0]
    return {nm: l2_error(oracle, m, 2, u, v, true.get(v, zero)) for v, nm in enumerate(["ux", "pr", "uy", "c"])}
