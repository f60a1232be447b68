"""GPU tests of the shallowwater module ("shallowwater", MHA_PHYSICS_SHALLOWWATER): every case through the C ABI via
mrhyde_amd.Block, against the restatement in tests/shallowwater_ref.py (which tests/test_shallowwater.py pins against the
reference's droptest gold and a finite difference).

Shapes: 2-D 3x3 Q1 and Q2 on a warped mesh (nine elements: the last workgroup is ragged).  States: xi and the bathymetry in
[0.5, 1.5], Hu and Hv in [-1, 1], so D^2 - b^2 >= 0.75 and no cancellation stands between fp64 and the tolerance; the
transient states keep xi of every step and stage in the same range.  Tolerances: RTOL = 1e-12 on residuals relative to the
array's largest entry and, per CRS entry, 1e-12 max(|ref|, 1e-3 rowmax) (ns_thermal_ref.crs_err)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import shallowwater_ref as R
from shallowwater_ref import RTOL, rel_err
from test_cdr_gpu import _device_assembler, _torch, _untouched_after, configure, make_block, run_paths, time_kw
from test_jacobian_apply_gpu import check_products
from test_jacobian_diag_multi_gpu import check_case
from test_shallowwater import check_droptest

pytestmark = pytest.mark.gpu

SHAPES = [((3, 3), 1, 2), ((3, 3), 2, 4)]


def func_set(name, m, qdeg, rng):
    """defaults | constants plus a sinprod and an array | deck strings in the coordinates, bathymetry and its derivatives
    included.  The bathymetry stays in [0.5, 1.5]."""
    if name == "defaults":
        return {}
    if name == "constants":
        nq = (qdeg // 2 + 1) ** 2
        return {"bathymetry": ("array", rng.uniform(0.5, 1.5, (m["nelem"], nq))), "bathymetry_x": 0.3, "bathymetry_y": -0.2,
                "source H": 0.2, "source Hu": ("sinprod", 0.4, [1.0, 2.0]), "source Hv": -0.1, "viscosity": 3.0, "Coriolis": 2.0}
    return {"bathymetry": "1+0.5*sin(x)*cos(y)", "bathymetry_x": "0.5*cos(x)*cos(y)", "bathymetry_y": "-0.5*sin(x)*sin(y)",
            "source H": "x*y", "source Hu": "sin(x)", "source Hv": "x-y"}


def case(oracle, ncell, order, seed, transient):
    rng = np.random.default_rng(seed)
    m = R.sw_mesh(oracle, ncell, order)
    u = R.random_state(rng, m)
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    rows = R.var_rows(m, 0)
    if tr is not None:
        # the seeded state is alpha_u u + (1 - alpha_u) u_prev + A_10 / b_0 (u_stage_0 - u_prev): keep xi in [0.5, 1.5]
        # there by giving every xi array the same draw plus a small one of its own
        for k in ("u_prev", "u_stage"):
            tr[k][rows] = u[rows][:, None] + rng.uniform(-0.05, 0.05, tr[k][rows].shape)
    fixed = (((m["dof_var"] == 1) & ((m["side_mask"] & 0b0011) != 0)) |
             ((m["dof_var"] == 2) & ((m["side_mask"] & 0b1100) != 0))).astype(np.uint8)
    return rng, m, u, tr, fixed


@pytest.mark.parametrize("ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("fset", ["defaults", "constants", "coordinates"])
@pytest.mark.parametrize("transient", [False, True])
def test_shallowwater_matches_the_yardstick(oracle, ncell, order, qdeg, fset, transient):
    rng, m, u, tr, fixed = case(oracle, ncell, order, 151, transient)
    funcs = func_set(fset, m, qdeg, rng)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    xi = ref["fields"]["val"][0].val
    assert xi.min() > 0.3 and xi.max() < 1.7
    blk = make_block(m, "shallowwater", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    out = run_paths(blk, m, u, tr, ref)
    r3, v3 = out["row-gather"]
    for r in np.flatnonzero(fixed)[:30]:  # fixed rows: nothing written but the overwrite's zeros
        assert r3[r] == 0.0 and np.all(v3[ref["rowptr"][r]:ref["rowptr"][r + 1]] == 0.0)


def test_defaults_are_the_reference_defaults(oracle):
    """gravity 9.8 and bathymetry 1 (shallowwater.cpp:32, :47), not shallowwaterHybridized's g = 9.81; the parameter and the
    unread functions are accepted."""
    rng, m, u, tr, fixed = case(oracle, (3, 3), 1, 152, True)
    ref = R.assemble(oracle, m, 2, u, fixed=fixed, transient=tr)
    for other in (dict(gravity=9.81), dict(funcs={"bathymetry": 0.0})):
        assert rel_err(R.assemble(oracle, m, 2, u, fixed=fixed, transient=tr, **other)["res"], ref["res"]) > 1e-4
    blk = make_block(m, "shallowwater", 2, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    run_paths(blk, m, u, tr, ref)
    configure(blk, {"viscosity": 3.0, "Coriolis": 2.0, "bottom friction": 5.0, "flux left": 1.0, "Neumann source Hu": 1.0,
                    "bathymetry side": 2.0}, {"form_param": -1.0})  # accepted, and as in the reference read by no term
    run_paths(blk, m, u, tr, ref)
    blk.set_physics_parameter("gravity", 9.81)
    ref2 = R.assemble(oracle, m, 2, u, fixed=fixed, transient=tr, gravity=9.81, rowptr=ref["rowptr"], colind=ref["colind"])
    run_paths(blk, m, u, tr, ref2)


def test_matrix_free_products_and_diagonal(oracle):
    """apply_jacobian forward and transposed, apply_jacobian_multi with K = 3 and jacobian_diagonal against the assembled
    matrix applied on the host; fixed rows included."""
    rng, m, u, tr, fixed = case(oracle, (3, 3), 2, 153, True)
    funcs = func_set("constants", m, 4, rng)
    ref = R.assemble(oracle, m, 4, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, "shallowwater", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    assert fixed.any() and not fixed.all()
    check_products(blk, m, u, tr, fixed, ref, 12)
    check_case((blk, m, u, tr, fixed, ref), 212, (3,))


def test_gold_droptest_on_the_device(oracle):
    """assemble_jacres plus a host sparse solve per Newton step; the initial state from set_initial's projection system."""
    torch = _torch()
    fn, _ = _device_assembler(oracle, "shallowwater")

    def initial(m):
        g = oracle.build_graph(m["ndof"], m["lids"])
        blk = make_block(m, "shallowwater", 2, graph=g)
        blk.set_function("hump", R.HUMP)
        blk.set_function("initial H", "1.0 + 0.1*exp(hump)")
        blk.set_function("initial Hu", "0.0")
        blk.set_function("initial Hv", "0.0")
        rhs = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(g[1]), dtype=torch.float64, device="cuda")
        blk.set_initial(rhs, vals)
        M = sp.csr_matrix((vals.cpu().numpy(), g[1], g[0]), shape=(m["ndof"],) * 2)
        return spla.spsolve(M.tocsc(), rhs.cpu().numpy())

    errs, _ = R.gold_droptest(oracle, fn, initial=initial)
    check_droptest(errs)


def test_gold_droptest_through_the_newton_driver(oracle):
    """Stage by stage through mrhyde_amd.Newton (absolute tolerance 1e-12 on the residual's largest entry), the linear
    solves on the host."""
    torch = _torch()
    import mrhyde_amd
    state = {}

    def step(m, fixed, u_prev, tr):
        if "blk" not in state:
            g = oracle.build_graph(m["ndof"], m["lids"])
            state.update(blk=make_block(m, "shallowwater", 2, fixed=fixed, graph=g), g=g)
        blk, (rowptr, colind) = state["blk"], state["g"]
        nd = m["ndof"]
        kw = time_kw(blk, dict(tr, u_stage=u_prev[:, None].copy()))
        u = torch.tensor(u_prev, device="cuda")
        res = torch.zeros(nd, dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
        nw = mrhyde_amd.Newton(blk, max_iter=20, nl_abs_tol=1e-12, use_relative=False, use_absolute=True)
        solves = 0
        while True:
            action = nw.step(u, res, vals, **kw)
            if action == mrhyde_amd.NEWTON_DONE:
                break
            assert action == mrhyde_amd.NEWTON_SOLVE
            torch.cuda.synchronize()
            J = sp.csr_matrix((vals.cpu().numpy(), colind, rowptr), shape=(nd, nd))
            nw.update(u, torch.tensor(spla.spsolve(J.tocsc(), res.cpu().numpy()), device="cuda"))
            solves += 1
        st = nw.state()
        assert st["status"] == 0 and st["resnorm"] < 1e-12 and 1 <= solves < 20, st
        nw.close()
        return u.cpu().numpy()

    errs, _ = R.gold_droptest(oracle, None, step=step)
    check_droptest(errs)


def test_views_mass_initial_dirichlet_groups_and_flux(oracle):
    torch = _torch()
    import mrhyde_amd
    dim, ncell, order, qdeg = 2, (3, 3), 2, 4
    rng, m, u, tr, fixed = case(oracle, ncell, order, 154, True)
    nd, n = m["ndof"], m["lids"].shape[1]
    ref = R.assemble(oracle, m, qdeg, u, fixed=fixed, transient=tr)
    rowptr, colind = ref["rowptr"], ref["colind"]
    F = ref["fields"]
    blk = make_block(m, "shallowwater", qdeg, fixed=fixed, graph=(rowptr, colind), workset_size=4)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    for w in range(blk.num_worksets()):
        e0, e1 = 4 * w, min(4 * w + 4, m["nelem"])
        blk.workset_update(w)
        blk.workset_compute_solution(ud, kw["u_prev"], kw["u_stage"])
        for v, nm in enumerate(R.NAMES):
            assert rel_err(blk.workset_view_numpy(nm), F["val"][v].val[e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy(nm + "_t"), F["dot"][v].val[e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy("grad(%s)[x]" % nm), F["grad"][v][0].val[e0:e1]) < RTOL
    for wts in (None, [1.0, 0.0, 1.3]):
        mass = torch.zeros((m["nelem"], n, n), dtype=torch.float64, device="cuda")
        blk.get_mass(mass, wts)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), oracle.get_mass(m, qdeg, wts)) < RTOL
    # set_initial
    off = [np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]) for v in range(3)]
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, m["nodes"])
    x, y = pb["ip"][..., 0], pb["ip"][..., 1]
    init = {"H": ("1.0 + 0.1*exp(hump)", 1.0 + 0.1 * np.exp(-100.0 * (x - 0.5) ** 2 - 100 * (y - 0.5) ** 2)),
            "Hu": ("0.3+x*y", 0.3 + x * y), "Hv": ("x-2*y", x - 2 * y)}
    blk.set_function("hump", R.HUMP)
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    for v, nm in enumerate(R.NAMES):
        blk.set_function("initial " + nm, init[nm][0])
        oracle.project_rhs(m["lids"], off[v], init[nm][1][..., None], pb["basis"], pb["wts"], want_rhs)
    oracle.set_initial_mass(m["lids"], oracle.get_mass(m, qdeg), False, rowptr, colind, want_vals)
    rhs = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.set_initial(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    # set_dirichlet: strong rows of Hu on the left side
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], be, bs)
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    dip = 0.5 - sb["ip"][..., 1] + 0.25 * sb["normals"][..., 0]
    blk.set_function("Dirichlet Hu left", "0.5-y+0.25*nx")
    dvals, mass = oracle.dirichlet_boundary(n, off[1], dip, sb["basis"][..., None], sb["wts"], None)
    oracle.set_dirichlet_group(be, m["lids"], fixed, dvals, mass, False, rowptr, colind, want_vals, want_rhs)
    blk.add_dirichlet_group("left", "Hu", be, bs)
    oracle.set_dirichlet_identity(m["lids"], fixed, rowptr, colind, want_vals)
    rhs, vals = torch.zeros_like(rhs), torch.zeros_like(vals)
    blk.set_dirichlet(rhs, vals)
    torch.cuda.synchronize()
    assert np.abs(want_rhs).max() > 0
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    # a Neumann group adds nothing (shallowwater::boundaryResidual is empty), compute_flux gives zeros
    te, ts = oracle.boundary_sides(dim, ncell, "top")
    gid = blk.add_boundary_group("top", mrhyde_amd.BC_NEUMANN, te, ts)
    res = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.assemble_boundary(ud, res, vals, **kw)
    yv = torch.zeros(nd, dtype=torch.float64, device="cuda")
    blk.apply_boundary_jacobian(ud, torch.ones(nd, dtype=torch.float64, device="cuda"), yv, **kw)
    torch.cuda.synchronize()
    assert bool((res == 0.0).all()) and bool((vals == 0.0).all()) and bool((yv == 0.0).all())
    nqs = oracle.side_sizes(dim, qdeg)[1]
    flux = torch.full((len(te), nqs), 4.0, dtype=torch.float64, device="cuda")
    dfl = torch.full((len(te), nqs, n), 4.0, dtype=torch.float64, device="cuda")
    blk.compute_flux(gid, ud, flux, dfl, **kw)
    torch.cuda.synchronize()
    assert bool((flux == 0.0).all()) and bool((dfl == 0.0).all())


def test_refusals_leave_the_outputs_untouched(oracle):
    torch = _torch()
    import mrhyde_amd
    rng, m, u, _, _ = case(oracle, (3, 3), 1, 155, False)
    blk = make_block(m, "shallowwater", 2)
    _, colind = blk.get_graph()
    nd, nnz = m["ndof"], len(colind)
    ud = torch.tensor(u, device="cuda")
    blk.set_function("bathymetry", "1+0.1*H")
    for kw in (dict(path=mrhyde_amd.PATH_POINT_ENGINE), dict(path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True), {}):
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, **kw), nd, nnz)
        assert "functions of the solution fields are built for the thermal module" in msg
    d = torch.full((nd,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.jacobian_diagonal(ud, d, overwrite=True)
    torch.cuda.synchronize()
    assert ei.value.code == 1 and bool((d == 7.0).all())
    blk.set_function("bathymetry", 1.0)
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, path=2), nd, nnz)  # MHA_PATH_ROW_OWNER
    assert "assembly path 2 is not available for this physics module" in msg
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, deterministic=True), nd, nnz)
    assert "MHA_ASSEMBLE_DETERMINISTIC" in msg
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.set_physics_parameter("g", 9.81)  # shallowwaterHybridized's name for it
    assert ei.value.code == 1 and "has no parameter 'g'" in str(ei.value)
    H = oracle.HGRAD
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(3, quadrature=2, physics="shallowwater", variables=[(H, 1)] * 3)
    assert ei.value.code == 1 and "shallowwater needs H, Hu, Hv in 2-D" in str(ei.value)
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=2, physics="shallowwater", variables=[(H, 1)] * 2)
    assert ei.value.code == 1 and "shallowwater needs H, Hu, Hv in 2-D" in str(ei.value)
