"""The yardstick of the shallowwater module (MHA_PHYSICS_SHALLOWWATER): shallowwater::volumeResidual restated on the
numpy forward-AD class of tests/oracle_lib.py.

TEST INFRASTRUCTURE (the checker), imported by tests/test_shallowwater.py and tests/test_shallowwater_gpu.py only.  It
shares nothing with the device code.

  * seeding: Workset::computeSolnTransientSeeded, seedwhat 1 (src/tools/workset.cpp:589-623), through
    ns_thermal_ref.fields_at_points;
  * the functions: numbers, ("sinprod", amp, freq), ("array", a), or deck strings in the coordinates;
  * shallowwater::volumeResidual (src/physics/shallowwater.cpp:118-153): the variable H holds the surface elevation xi,
    the depth is xi + bathymetry, the pressure term is written H*H - bath*bath; gravity 9.8 (:32); "viscosity",
    "Coriolis" are evaluated and read by no term;
  * the scatter of assemblyManager.cpp:4031-4145 (ns_thermal_ref.scatter).

Variables: H, Hu, Hv (shallowwater.cpp:24-26), 2-D.
"""
import numpy as np

import cdr_ref as C
import ns_thermal_ref as N
from ns_thermal_ref import RTOL, crs_err, rel_err, transient_state, var_rows, warp  # noqa: F401  (re-exported)

# reference defaults (shallowwater.cpp:47-55, :32)
FUNC_DEFAULTS = {"bathymetry": 1.0, "bathymetry_x": 0.0, "bathymetry_y": 0.0, "bottom friction": 1.0, "viscosity": 0.0,
                 "Coriolis": 0.0, "source H": 0.0, "source Hu": 0.0, "source Hv": 0.0}
GRAVITY = 9.8
NAMES = ["H", "Hu", "Hv"]
# transient Butcher tableau DIRK-1,2 (solverManager.cpp:552-558) with the one-step BDF weights
DIRK12 = dict(stage=0, butcher_A=np.array([[0.5]]), butcher_b=np.array([1.0]), bdf=np.array([1.0, -1.0]))
HUMP = "-100.0*(x-0.5)*(x-0.5) - 100*(y-0.5)*(y-0.5)"


def sw_mesh(oracle, ncell, order, do_warp=True):
    m = oracle.mesh_multi(2, ncell, [oracle.HGRAD] * 3, [order] * 3)
    return warp(m) if do_warp else m


def element_arrays(oracle, m, qdeg, u, *, funcs=None, gravity=GRAVITY, transient=None, elems=None, time=0.0):
    """res(elem, pos) and its derivative array -> (R [E][n], J [E][n][n]) in LID-position order, plus the field dict."""
    assert m["dim"] == 2 and len(m["types"]) == 3
    F = N.fields_at_points(oracle, m, qdeg, u, transient, elems)
    F["names"] = NAMES
    E, n = F["lids"].shape
    w = F["wts"]
    fs = dict(FUNC_DEFAULTS)
    fs.update(funcs or {})
    fields = C.field_dict(oracle, F, NAMES, time)
    strings = {k: (v if isinstance(v, str) else repr(float(v))) for k, v in fs.items() if isinstance(v, (str, int, float))}
    fv = {k: C.eval_function(oracle, fs[k], fields, strings, F).val for k in FUNC_DEFAULTS}
    bath, bath_x, bath_y = fv["bathymetry"], fv["bathymetry_x"], fv["bathymetry_y"]
    xi, Hu, Hv = F["val"]
    xi_dot, Hu_dot, Hv_dot = F["dot"]
    R, J = np.zeros((E, n)), np.zeros((E, n, n))

    def add_rows(var, Fv, Fx, Fy):
        B, G, off = F["B"][var], F["G"][var], F["off"][var]
        rv = np.einsum("eq,ejq->ej", Fv.val, B)
        rdx = np.einsum("eqw,ejq->ejw", Fv.dx, B)
        for d, Fd in enumerate((Fx, Fy)):
            rv = rv + np.einsum("eq,ejq->ej", Fd.val, G[..., d])
            rdx = rdx + np.einsum("eqw,ejq->ejw", Fd.dx, G[..., d])
        R[:, off] += rv
        J[:, off, :] += rdx

    # :124-129
    add_rows(0, (xi_dot - fv["source H"]) * w, (Hu * -1.0) * w, (Hv * -1.0) * w)
    # :131-134
    H = xi + bath
    uHu, uHv, vHv = Hu * Hu / H, Hu * Hv / H, Hv * Hv / H
    pres = (H * H - bath * bath) * (0.5 * gravity)
    # :136-141
    add_rows(1, (Hu_dot - xi * (gravity * bath_x) - fv["source Hu"]) * w, ((uHu + pres) * -1.0) * w, (uHv * -1.0) * w)
    # :143-149
    add_rows(2, (Hv_dot - xi * (gravity * bath_y) - fv["source Hv"]) * w, (uHv * -1.0) * w, ((vHv + pres) * -1.0) * w)
    return R, J, F


def assemble(oracle, m, qdeg, u, *, funcs=None, gravity=GRAVITY, fixed=None, transient=None, rowptr=None, colind=None,
             time=0.0):
    R, J, F = element_arrays(oracle, m, qdeg, u, funcs=funcs, gravity=gravity, transient=transient, time=time)
    out = N.scatter(m, R, J, F["lids"], fixed, rowptr, colind, oracle)
    out.update(local_res=-R, local_J=J, fields=F)
    return out


def host_assembler(oracle, qdeg):
    """assemble_fn of the gold driver: yardstick assembly, host matrix with identity fixed rows."""
    import scipy.sparse as sp

    def fn(m, u, funcs, fixed, tr):
        ref = assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
        v = ref["crs_vals"].copy()
        oracle.apply_dbc_diag(fixed, ref["rowptr"], ref["colind"], v)
        return sp.csr_matrix((v, ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2), ref["res"]
    return fn


def random_state(rng, m):
    """xi in [0.5, 1.5], Hu and Hv in [-1, 1]: with a bathymetry in [0.5, 1.5] the depth stays above 1."""
    u = rng.uniform(-1, 1, m["ndof"])
    rows = var_rows(m, 0)
    u[rows] = rng.uniform(0.5, 1.5, len(rows))
    return u


def droptest_mesh(oracle, ncell=(40, 40)):
    m = sw_mesh(oracle, ncell, 1, do_warp=False)
    # Hu strongly zero on left and right, Hv on top and bottom (side_mask bits: left 1, right 2, bottom 4, top 8)
    fixed = (((m["dof_var"] == 1) & ((m["side_mask"] & 0b0011) != 0)) |
             ((m["dof_var"] == 2) & ((m["side_mask"] & 0b1100) != 0))).astype(np.uint8)
    return m, fixed


def droptest_initial(oracle, m):
    """Initial conditions of the deck: the L2 projection of 1.0 + 0.1*exp(hump) onto H, zero Hu and Hv."""
    hump = lambda x: 1.0 + 0.1 * np.exp(-100.0 * (x[..., 0] - 0.5) ** 2 - 100.0 * (x[..., 1] - 0.5) ** 2)
    return C.l2_projection(oracle, m, 2, 0, hump)


def gold_droptest(oracle, assemble_fn, initial=None, step=None, ncell=(40, 40), nsteps=5, dt=1e-3):
    """regression/shallowwater/droptest: DIRK-1,2, dt 1e-3, five steps, Newton to 1e-12 per stage, direct solves.
    assemble_fn(m, u, funcs, fixed, transient) -> (J csr, rhs); initial(m) -> the projected state; step(m, fixed, u_prev,
    tr) -> the stage solution (default: Newton on assemble_fn).  -> {name: [error at step 0..nsteps]}, the final state."""
    m, fixed = droptest_mesh(oracle, ncell)
    u = droptest_initial(oracle, m) if initial is None else initial(m)
    u[fixed != 0] = 0.0
    zero = lambda x: 0.0 * x[..., 0]
    errs = {nm: [C.l2_error(oracle, m, 2, u, v, zero)] for v, nm in enumerate(NAMES)}
    for _ in range(nsteps):
        tr = dict(DIRK12, u_prev=u[:, None].copy(), dt=dt)
        if step is not None:
            u = step(m, fixed, u.copy(), tr)
        else:
            def newton_step(v, tr=tr):
                return assemble_fn(m, v, {}, fixed, dict(tr, u_stage=v[:, None].copy()))
            u = C.newton(newton_step, u.copy(), 20, 1e-12)
        # one stage with b = [1]: the step's solution is the stage solution
        for v, nm in enumerate(NAMES):
            errs[nm].append(C.l2_error(oracle, m, 2, u, v, zero))
    return errs, u


def read_gold(path):
    """-> {name: [(value string, time)]} in file order."""
    import re
    out = {}
    for nm, val, t in re.findall(r"L2 norm of the error for (\w+) = ([-0-9.e+]+)\s+\(time = ([-0-9.e+]+)\)", open(path).read()):
        out.setdefault(nm, []).append((val, float(t)))
    return out


def half_unit(s):
    """Half a unit of the last printed digit of the number string s ("0.00250518" -> 5e-9, "1.06644e-08" -> 5e-14)."""
    mant, _, exp = s.lower().partition("e")
    digits = len(mant.split(".")[1]) if "." in mant else 0
    return 0.5 * 10.0 ** (-digits + (int(exp) if exp else 0))
