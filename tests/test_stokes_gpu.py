"""GPU tests of the stokes module ("stokes", MHA_PHYSICS_STOKES): every case through the C ABI via mrhyde_amd.Block, against
the restatement in tests/stokes_ref.py (which tests/test_stokes.py pins against the reference's golds and a finite
difference), and against the navierstokes module on the device where the two operators coincide.

Shapes: 2-D 3x3 Q1/Q1 and Q2/Q1 (nine elements: the last workgroup is ragged), 3-D 2x2x2 Q1/Q1 and Q2/Q1 (89 dofs: a
workgroup per element, Kc = 1 in the multi-vector product); the meshes are warped.  Tolerances: RTOL = 1e-12 on residuals
relative to the array's largest entry and, per CRS entry, 1e-12 max(|ref|, 1e-3 rowmax) (ns_thermal_ref.crs_err); the
products and the diagonal as tests/test_jacobian_apply_gpu.py and tests/test_jacobian_diag_multi_gpu.py hold navierstokes."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import shallowwater_ref as W
import stokes_ref as R
from stokes_ref import RTOL, crs_err, rel_err
from test_cdr_gpu import _device_assembler, _torch, _untouched_after, configure, make_block, run_paths, time_kw
from test_jacobian_apply_gpu import check_products
from test_jacobian_diag_multi_gpu import check_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
SHAPES = [(2, (3, 3), (1, 1), 2), (2, (3, 3), (2, 1), 4), (3, (2, 2, 2), (1, 1), 2), (3, (2, 2, 2), (2, 1), 4)]
OPTIONS = [dict(usePSPG=0, useLSIC=0), dict(usePSPG=1, useLSIC=0), dict(usePSPG=0, useLSIC=1), dict(usePSPG=1, useLSIC=1)]
FREQ = [1.0, 2.0, 0.5]


def func_set(name, dim, m, qdeg, rng):
    """defaults | constants plus a sinprod and an array | deck strings in the coordinates.  "source pr" is set in the two
    latter: no term reads it (stokes.cpp:59, :78)."""
    if name == "defaults":
        return {}
    if name == "constants":
        nq = (qdeg // 2 + 1) ** dim
        f = {"source ux": 0.3, "source uy": ("sinprod", 1.0, FREQ[:dim]), "source pr": 5.0,
             "viscosity": ("array", rng.uniform(0.5, 1.5, (m["nelem"], nq)))}
        if dim == 3:
            f["source uz"] = -0.2
        return f
    f = {"source ux": "sin(x)*y", "source uy": "x-y", "source pr": "x*y", "viscosity": "0.7+0.1*x*y"}
    if dim == 3:
        f["source uz"] = "z*x+0.1"
    return f


def fixed_rows(m):
    """strong rows on bottom and top: the velocities, not the pressure"""
    return (((m["side_mask"] & 0b1100) != 0) & (m["dof_var"] != 1)).astype(np.uint8)


def case(oracle, dim, ncell, orders, seed, transient):
    rng = np.random.default_rng(seed)
    m = R.stokes_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    return rng, m, u, tr, fixed_rows(m)


@pytest.mark.parametrize("dim,ncell,orders,qdeg", SHAPES)
@pytest.mark.parametrize("fset", ["defaults", "constants", "coordinates"])
@pytest.mark.parametrize("transient", [False, True])
def test_stokes_matches_the_yardstick(oracle, dim, ncell, orders, qdeg, fset, transient):
    """Residual and CRS values on every assembly path, for no stabilisation, PSPG, LSIC and both."""
    rng, m, u, tr, fixed = case(oracle, dim, ncell, orders, 141, transient)
    if orders == (2, 1) and dim == 3:
        assert m["lids"].shape[1] == 89
    funcs = func_set(fset, dim, m, qdeg, rng)
    graph = oracle.build_graph(m["ndof"], m["lids"])
    blk = make_block(m, "stokes", qdeg, fixed=fixed, graph=graph)
    configure(blk, funcs)
    for params in OPTIONS:
        ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, fixed=fixed, transient=tr, rowptr=graph[0], colind=graph[1])
        configure(blk, {}, params)
        out = run_paths(blk, m, u, tr, ref)
        r3, v3 = out["row-gather"]
        for r in np.flatnonzero(fixed)[:30]:  # fixed rows: nothing written but the overwrite's zeros
            assert r3[r] == 0.0 and np.all(v3[graph[0][r]:graph[0][r + 1]] == 0.0)


def assemble_on_device(blk, m, u, nnz, tr=None):
    torch = _torch()
    import mrhyde_amd
    kw = time_kw(blk, tr)
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy(), vals.cpu().numpy()


@pytest.mark.parametrize("dim,ncell,orders,qdeg", SHAPES)
def test_stokes_equals_navierstokes_at_zero_velocity(oracle, dim, ncell, orders, qdeg):
    """Two point functions: at ux = uy = uz = 0 the convective term and its derivative vanish; steady, density 1, no
    stabilisation, fix_uz_offsets = 1 in 3-D.  And the stokes operator is linear: the same CRS values at another state."""
    rng, m, u, _, fixed = case(oracle, dim, ncell, orders, 142, False)
    u[m["dof_var"] != 1] = 0.0
    funcs = func_set("constants", dim, m, qdeg, rng)
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    got = {}
    for phys, params in (("stokes", {}), ("navierstokes", dict(fix_uz_offsets=1) if dim == 3 else {})):
        blk = make_block(m, phys, qdeg, fixed=fixed, graph=(rowptr, colind))
        configure(blk, funcs, params)
        got[phys] = assemble_on_device(blk, m, u, len(colind))
        if phys == "stokes":
            other = assemble_on_device(blk, m, rng.uniform(-1, 1, m["ndof"]), len(colind))
    assert np.abs(got["stokes"][0]).max() > 0 and rel_err(got["stokes"][0], got["navierstokes"][0]) < RTOL
    assert crs_err(got["stokes"][1], dict(crs_vals=got["navierstokes"][1], rowptr=rowptr)) < RTOL
    assert rel_err(other[1], got["stokes"][1]) < RTOL and rel_err(other[0], got["stokes"][0]) > 1e-3


@pytest.mark.parametrize("dim,ncell,orders,qdeg,transient", [(2, (3, 3), (2, 1), 4, True), (3, (2, 2, 2), (2, 1), 4, False)])
def test_matrix_free_products_and_diagonal(oracle, dim, ncell, orders, qdeg, transient):
    """apply_jacobian forward and transposed, apply_jacobian_multi with K = 3 and jacobian_diagonal against the assembled
    matrix applied on the host; fixed rows included."""
    rng, m, u, tr, fixed = case(oracle, dim, ncell, orders, 143, transient)
    funcs = func_set("constants", dim, m, qdeg, rng)
    params = dict(usePSPG=1, useLSIC=1)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, fixed=fixed, transient=tr)
    blk = make_block(m, "stokes", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    assert fixed.any() and not fixed.all()
    check_products(blk, m, u, tr, fixed, ref, 11)
    check_case((blk, m, u, tr, fixed, ref), 211, (3,))
    if dim == 3:
        assert m["lids"].shape[1] == 89 and 1 <= blk.info("jacobian_apply_vectors") <= 3


def read(name):
    return W.read_gold(os.path.join(GOLD, name))


def test_gold_2d_verification_pspg_on_the_device(oracle):
    fn, _ = _device_assembler(oracle, "stokes", dict(usePSPG=1))
    got = R.gold_pspg(oracle, fn)
    for k, ((s, t),) in read("stokes_2D_verification_pspg.gold").items():
        print(k, got[k], s)
        assert abs(got[k] - float(s)) <= W.half_unit(s), (k, got[k], s)


def test_gold_channel_on_the_device(oracle):
    fn, _ = _device_assembler(oracle, "stokes")
    got = R.gold_channel(oracle, fn)
    gold = read("stokes_channel.gold")
    assert sorted(gold) == ["pr", "ux", "uy"]
    for k in gold:
        print(k, got[k])
        assert got[k] < 1e-12, (k, got[k])


def test_views_mass_initial_dirichlet_groups_and_flux(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(144)
    dim, ncell, orders, qdeg = 2, (3, 3), (2, 1), 4
    m = R.stokes_mesh(oracle, dim, ncell, orders)
    nd, n = m["ndof"], m["lids"].shape[1]
    u = rng.uniform(-1, 1, nd)
    tr = R.transient_state(rng, nd)
    fixed = fixed_rows(m)
    ref = R.assemble(oracle, m, qdeg, u, fixed=fixed, transient=tr)
    rowptr, colind = ref["rowptr"], ref["colind"]
    F = ref["fields"]
    names = R.var_names(dim)
    blk = make_block(m, "stokes", qdeg, fixed=fixed, graph=(rowptr, colind), workset_size=4)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    # the workset views
    for w in range(blk.num_worksets()):
        e0, e1 = 4 * w, min(4 * w + 4, m["nelem"])
        blk.workset_update(w)
        blk.workset_compute_solution(ud, kw["u_prev"], kw["u_stage"])
        for v, nm in enumerate(names):
            assert rel_err(blk.workset_view_numpy(nm), F["val"][v].val[e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy(nm + "_t"), F["dot"][v].val[e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy("grad(%s)[y]" % nm), F["grad"][v][1].val[e0:e1]) < RTOL
    # the mass of every variable
    for wts in (None, [1.0, 0.0, 1.3]):
        mass = torch.zeros((m["nelem"], n, n), dtype=torch.float64, device="cuda")
        blk.get_mass(mass, wts)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), oracle.get_mass(m, qdeg, wts)) < RTOL
    # set_initial: (initial <var>, basis) per variable and the mass of every variable
    off = [np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]) for v in range(3)]
    pbs = [oracle.physical_basis_var(dim, oracle.HGRAD, int(m["orders"][v]), qdeg, m["nodes"]) for v in range(3)]
    init = {"ux": ("0.3+x*y", lambda x, y: 0.3 + x * y), "pr": ("1+sin(x)*y", lambda x, y: 1 + np.sin(x) * y),
            "uy": ("x-2*y", lambda x, y: x - 2 * y)}
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    for v, nm in enumerate(names):
        text, f = init[nm]
        blk.set_function("initial " + nm, text)
        data = f(pbs[v]["ip"][..., 0], pbs[v]["ip"][..., 1])
        oracle.project_rhs(m["lids"], off[v], data[..., None], pbs[v]["basis"], pbs[v]["wts"], want_rhs)
    oracle.set_initial_mass(m["lids"], oracle.get_mass(m, qdeg), False, rowptr, colind, want_vals)
    rhs = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.set_initial(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    # set_dirichlet: strong rows of ux and uy on the bottom side
    be, bs = oracle.boundary_sides(dim, ncell, "bottom")
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    dirichlet = {"ux": ("0.5-x+0.25*ny", lambda x, y, ny: 0.5 - x + 0.25 * ny), "uy": ("2+x*x", lambda x, y, ny: 2 + x * x)}
    for v, nm in enumerate(names):
        if nm not in dirichlet:
            continue
        text, f = dirichlet[nm]
        sb = oracle.physical_side_basis(dim, int(m["orders"][v]), qdeg, m["nodes"], be, bs)
        dip = f(sb["ip"][..., 0], sb["ip"][..., 1], sb["normals"][..., 1])
        blk.set_function("Dirichlet %s bottom" % nm, text)
        dvals, mass = oracle.dirichlet_boundary(n, off[v], dip, sb["basis"][..., None], sb["wts"], None)
        oracle.set_dirichlet_group(be, m["lids"], fixed, dvals, mass, False, rowptr, colind, want_vals, want_rhs)
        blk.add_dirichlet_group("bottom", nm, be, bs)
    oracle.set_dirichlet_identity(m["lids"], fixed, rowptr, colind, want_vals)
    rhs, vals = torch.zeros_like(rhs), torch.zeros_like(vals)
    blk.set_dirichlet(rhs, vals)
    torch.cuda.synchronize()
    assert np.abs(want_rhs).max() > 0
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    # a Neumann group adds nothing (stokes::boundaryResidual is empty), compute_flux gives zeros
    le, ls = oracle.boundary_sides(dim, ncell, "left")
    gid = blk.add_boundary_group("left", mrhyde_amd.BC_NEUMANN, le, ls)
    res = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.assemble_boundary(ud, res, vals, **kw)
    y = torch.zeros(nd, dtype=torch.float64, device="cuda")
    blk.apply_boundary_jacobian(ud, torch.ones(nd, dtype=torch.float64, device="cuda"), y, **kw)
    torch.cuda.synchronize()
    assert bool((res == 0.0).all()) and bool((vals == 0.0).all()) and bool((y == 0.0).all())
    nqs = oracle.side_sizes(dim, qdeg)[1]
    flux = torch.full((len(le), nqs), 4.0, dtype=torch.float64, device="cuda")
    dfl = torch.full((len(le), nqs, n), 4.0, dtype=torch.float64, device="cuda")
    blk.compute_flux(gid, ud, flux, dfl, **kw)
    torch.cuda.synchronize()
    assert bool((flux == 0.0).all()) and bool((dfl == 0.0).all())
    # the generic Flux condition on pr
    te, ts = oracle.boundary_sides(dim, ncell, "right")
    sb = oracle.physical_side_basis(dim, orders[1], qdeg, m["nodes"], te, ts)
    x, yy, nx = sb["ip"][..., 0], sb["ip"][..., 1], sb["normals"][..., 0]
    want = np.zeros(nd)
    oracle.flux_condition(te, m["lids"], off[1], 1.5 + x * nx - 2 * yy, sb["wts"], sb["basis"][..., None], want, fixed=fixed)
    b2 = make_block(m, "stokes", qdeg, fixed=fixed)
    b2.set_function("Flux pr right", "1.5 + x*nx - 2*y")
    b2.add_flux_group("right", "pr", te, ts)
    res = torch.zeros(nd, dtype=torch.float64, device="cuda")
    b2.assemble_boundary(ud, res, None, compute_jacobian=False)
    torch.cuda.synchronize()
    assert np.abs(want).max() > 0 and rel_err(res.cpu().numpy(), want) < RTOL


def test_refusals_leave_the_outputs_untouched(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(145)
    m = R.stokes_mesh(oracle, 2, (3, 3), (1, 1))
    blk = make_block(m, "stokes", 2)
    _, colind = blk.get_graph()
    nd, nnz = m["ndof"], len(colind)
    ud = torch.tensor(rng.uniform(-1, 1, nd), device="cuda")
    # a deck string that reads a solution field: the standing refusal of the modules without such a form
    blk.set_function("viscosity", "1+ux*ux")
    for kw in (dict(path=mrhyde_amd.PATH_POINT_ENGINE), dict(path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True), {}):
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, **kw), nd, nnz)
        assert "functions of the solution fields are built for the thermal module" in msg
    y = torch.full((nd,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.apply_jacobian(ud, torch.ones_like(y), y, overwrite=True)
    torch.cuda.synchronize()
    assert ei.value.code == 1 and bool((y == 7.0).all())
    blk.set_function("viscosity", 1.0)
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, path=2), nd, nnz)  # MHA_PATH_ROW_OWNER
    assert "assembly path 2 is not available for this physics module" in msg
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, deterministic=True), nd, nnz)
    assert "MHA_ASSEMBLE_DETERMINISTIC" in msg
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.set_physics_parameter("useSUPG", 1)
    assert ei.value.code == 1 and "has no parameter 'useSUPG'" in str(ei.value)
    H = oracle.HGRAD
    for dim, nv in ((2, 2), (2, 4), (3, 3)):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            mrhyde_amd.Block(dim, quadrature=2, physics="stokes", variables=[(H, 1)] * nv)
        assert ei.value.code == 1 and "stokes needs ux, pr, uy" in str(ei.value)
