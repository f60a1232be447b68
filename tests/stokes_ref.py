"""The yardstick of the stokes module (MHA_PHYSICS_STOKES): stokes::volumeResidual restated on the numpy forward-AD
class of tests/oracle_lib.py.

TEST INFRASTRUCTURE (the checker), imported by tests/test_stokes.py and tests/test_stokes_gpu.py only.  It shares nothing
with the device code.

  * seeding: Workset::computeSolnTransientSeeded, seedwhat 1 (src/tools/workset.cpp:589-623), through
    ns_thermal_ref.fields_at_points;
  * the functions: numbers, ("sinprod", amp, freq), ("array", a), or deck strings in the coordinates
    (oracle_lib.deck_eval_ad through cdr_ref.eval_function);
  * stokes::volumeResidual (src/physics/stokes.cpp:178-438), 2-D and 3-D branches, with its quirks: the PSPG tau is
    h / (2 nu) in 2-D (:256) and h^2 / (2 nu) in 3-D (:402); the LSIC term is tested with the SUM of the derivatives of the
    pressure test function (:283, :432); "source pr" is evaluated and read by no term; the uz rows use their own offsets;
  * the scatter of assemblyManager.cpp:4031-4145 (ns_thermal_ref.scatter).

Variables: ux, pr, uy[, uz] (stokes.cpp:25-32).
"""
import numpy as np

import cdr_ref as C
import ns_thermal_ref as N
from ns_thermal_ref import RTOL, crs_err, rel_err, transient_state, var_rows, warp  # noqa: F401  (re-exported)

# reference defaults (stokes.cpp:58-62, :44-45)
FUNC_DEFAULTS = {"source ux": 0.0, "source pr": 0.0, "source uy": 0.0, "source uz": 0.0, "viscosity": 1.0}
PARAM_DEFAULTS = {"usePSPG": 0, "useLSIC": 0}


def var_names(dim):
    return ["ux", "pr", "uy"] + (["uz"] if dim == 3 else [])


def stokes_mesh(oracle, dim, ncell, orders, do_warp=True, hi=None):
    """orders = (velocity, pressure) -> mesh_multi of ux, pr, uy[, uz]."""
    ov, op = orders
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * (dim + 1), [ov, op] + [ov] * (dim - 1), hi=hi)
    return warp(m) if do_warp else m


def element_arrays(oracle, m, qdeg, u, *, funcs=None, params=None, transient=None, elems=None, time=0.0):
    """res(elem, pos) and its derivative array -> (R [E][n], J [E][n][n]) in LID-position order, plus the field dict."""
    AD = oracle.ADView
    dim = m["dim"]
    names = var_names(dim)
    assert len(m["types"]) == len(names)
    F = N.fields_at_points(oracle, m, qdeg, u, transient, elems)
    F["names"] = names
    E, n = F["lids"].shape
    w = F["wts"]
    fs = dict(FUNC_DEFAULTS)
    fs.update(funcs or {})
    P = dict(PARAM_DEFAULTS)
    P.update(params or {})
    assert set(P) == set(PARAM_DEFAULTS), set(P) - set(PARAM_DEFAULTS)
    fields = C.field_dict(oracle, F, names, time)
    strings = {k: (v if isinstance(v, str) else repr(float(v))) for k, v in fs.items() if isinstance(v, (str, int, float))}
    fv = {k: C.eval_function(oracle, fs[k], fields, strings, F).val for k in FUNC_DEFAULTS}
    visc = fv["viscosity"]
    src = [fv["source ux"], fv["source uy"], fv["source uz"]][:dim]
    vn, prn = [0, 2, 3][:dim], 1
    pr = F["val"][prn]
    R, J = np.zeros((E, n)), np.zeros((E, n, n))
    zero = AD(np.zeros_like(w), W=n)

    def add_rows(var, Fv, Fg):
        B, G, off = F["B"][var], F["G"][var], F["off"][var]
        rv = np.einsum("eq,ejq->ej", Fv.val, B)
        rdx = np.einsum("eqw,ejq->ejw", Fv.dx, B)
        for d in range(dim):
            if Fg[d] is None:
                continue
            rv = rv + np.einsum("eq,ejq->ej", Fg[d].val, G[..., d])
            rdx = rdx + np.einsum("eqw,ejq->ejw", Fg[d].dx, G[..., d])
        R[:, off] += rv
        J[:, off, :] += rdx

    for i in range(dim):
        gu = F["grad"][vn[i]]
        Fg = [(gu[d] * visc - (pr if d == i else 0.0)) * w for d in range(dim)]
        add_rows(vn[i], zero + (-src[i] * w), Fg)
    divu = zero
    for i in range(dim):
        divu = divu + F["grad"][vn[i]][i]
    add_rows(prn, divu * w, [None] * dim)
    hh = np.broadcast_to(F["h"][:, None], w.shape)
    if P["usePSPG"]:
        tau = (hh if dim == 2 else hh * hh) / (2.0 * visc)
        gp = F["grad"][prn]
        add_rows(prn, zero, [(gp[d] + src[d]) * (tau * w) for d in range(dim)])
    if P["useLSIC"]:
        tau = hh * hh / (2.0 * visc)
        S = divu * (tau * w)
        add_rows(prn, zero, [S] * dim)
    return R, J, F


def assemble(oracle, m, qdeg, u, *, funcs=None, params=None, fixed=None, transient=None, rowptr=None, colind=None,
             time=0.0):
    R, J, F = element_arrays(oracle, m, qdeg, u, funcs=funcs, params=params, transient=transient, time=time)
    out = N.scatter(m, R, J, F["lids"], fixed, rowptr, colind, oracle)
    out.update(local_res=-R, local_J=J, fields=F)
    return out


def residual_only(oracle, m, qdeg, u, **kw):
    """The residual as the scatter gives it (-res.val()), for finite differences."""
    return assemble(oracle, m, qdeg, u, **kw)["res"]


def host_assembler(oracle, qdeg, params=None):
    """assemble_fn of the gold drivers: yardstick assembly, host matrix with identity fixed rows."""
    import scipy.sparse as sp

    def fn(m, u, funcs, fixed, tr):
        ref = assemble(oracle, m, qdeg, u, funcs=funcs, params=params, fixed=fixed, transient=tr)
        v = ref["crs_vals"].copy()
        oracle.apply_dbc_diag(fixed, ref["rowptr"], ref["colind"], v)
        return sp.csr_matrix((v, ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2), ref["res"]
    return fn


def _channel(oracle, assemble_fn, orders):
    """4x4 unit square, quadrature 2, source ux = 1, ux = uy = 0 on bottom and top, one direct solve from 0 (the
    operator is linear).  -> the three "L2 norm of the error" values against ux = y (1 - y) / 2, pr = 0, uy = 0."""
    import scipy.sparse.linalg as spla
    m = stokes_mesh(oracle, 2, (4, 4), orders, do_warp=False)
    fixed = (((m["side_mask"] & 0b1100) != 0) & (m["dof_var"] != 1)).astype(np.uint8)
    J, rhs = assemble_fn(m, np.zeros(m["ndof"]), {"source ux": 1.0}, fixed, None)
    u = spla.spsolve(J.tocsc(), rhs)
    true = {0: lambda x: 0.5 * x[..., 1] * (1 - x[..., 1])}
    zero = lambda x: 0.0 * x[..., 0]
    return {nm: C.l2_error(oracle, m, 2, u, v, true.get(v, zero)) for v, nm in enumerate(["ux", "pr", "uy"])}


def gold_pspg(oracle, assemble_fn):
    """regression/stokes/2D_verification_pspg: Q1/Q1 with usePSPG (the assembler carries the parameter)."""
    return _channel(oracle, assemble_fn, (1, 1))


def gold_channel(oracle, assemble_fn):
    """regression/stokes/channel: Q2/Q1, no stabilisation; the exact solution lies in the space."""
    return _channel(oracle, assemble_fn, (2, 1))
