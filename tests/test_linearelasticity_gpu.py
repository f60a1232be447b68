"""GPU tests of the linearelasticity block (MHA_PHYSICS_LINEARELASTICITY, "linearelasticity"): every case through the C
ABI via mrhyde_amd.Block, against the restatement of the reference's loop nests in tests/linearelasticity_ref.py (which
tests/test_linearelasticity.py pins against the reference's golds).  Helpers and bounds are those of
tests/test_ns_thermal_gpu.py, the same engine's tests."""
import numpy as np
import pytest

import linearelasticity_ref as R
from linearelasticity_ref import RTOL, crs_err, rel_err
from test_ns_thermal_gpu import _torch, _untouched_after, check_all, configure, make_block, run_gpu, time_kw

pytestmark = pytest.mark.gpu

PHYS = "linearelasticity"
# 2-D 4x3: 12 elements at 8 per workgroup leave a partial last workgroup; 3-D Q2: 81 dofs, one element per workgroup and
# the multi-tile Jacobian phase
CASES = [(2, (4, 3), 1), (2, (4, 3), 2), (3, (3, 2, 2), 1), (3, (2, 2, 2), 2)]
SIDE_BIT = {"left": 0, "right": 1, "bottom": 2, "top": 3, "back": 4, "front": 5}


def funcs_for(oracle, m, qdeg, dim):
    """lambda a closed form and mu an array, both non-constant in x; non-zero sources of three kinds."""
    ip = oracle.physical_basis_var(dim, oracle.HGRAD, 1, qdeg, m["nodes"])["ip"]
    f = {"lambda": ("sinprod", 1.7, [0.9, 1.1, 0.7][:dim]), "mu": ("array", 0.8 + 0.3 * ip[..., 0]), "source dx": 0.3,
         "source dy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim])}
    if dim == 3:
        f["source dz"] = -0.2
    return f


def fixed_rows(m):
    """strong-Dirichlet rows on two sides, every component"""
    return ((m["side_mask"] & 0b1100) != 0).astype(np.uint8)


@pytest.mark.parametrize("dim,ncell,order", CASES)
@pytest.mark.parametrize("mode", ["steady", "transient"])
def test_volume_terms_match_the_restatement_on_every_path(oracle, dim, ncell, order, mode):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(71)
    m = R.le_mesh(oracle, dim, ncell, order)
    qdeg = 2 * order
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = fixed_rows(m)
    tr = R.transient_state(rng, m["ndof"]) if mode == "transient" else None
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, {})
    out = run_gpu(blk, m, u, tr, len(ref["colind"]), local=True)
    check_all(out, ref)
    # two paths against each other: the atomic point engine and the row gather
    assert rel_err(out["res"], out["res3"]) < RTOL and crs_err(out["crs_vals"], dict(ref, crs_vals=out["crs_vals3"])) < RTOL
    for r in np.flatnonzero(fixed)[:30]:
        assert out["res3"][r] == 0.0 and np.all(out["crs_vals3"][ref["rowptr"][r]:ref["rowptr"][r + 1]] == 0.0)
    with pytest.raises(mrhyde_amd.MhaError) as ei:  # bit-reproducible mode: the affine thermal row-owner path only
        z = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), z, torch.zeros(len(ref["colind"]), dtype=torch.float64, device="cuda"),
                            deterministic=True, **time_kw(blk, tr))
    assert ei.value.code == 1 and "MHA_ASSEMBLE_DETERMINISTIC" in str(ei.value)


def test_incplanestress_and_deck_strings_in_the_coordinates(oracle):
    rng = np.random.default_rng(72)
    dim, ncell, order, qdeg = 2, (4, 3), 2, 4
    m = R.le_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params={"incplanestress": 1}, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, {"incplanestress": 1})
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)
    plain = R.assemble(oracle, m, qdeg, u, funcs=funcs, transient=tr, rowptr=ref["rowptr"], colind=ref["colind"])
    assert rel_err(plain["res"], ref["res"]) > 1e-3  # the option changes the operator
    # same block, the option off again, lambda and a source as deck strings: the interpreter instantiation of the engine
    text = dict(funcs, **{"lambda": "1.7*sin(0.9*x)*sin(1.1*y)", "source dy": "sin(x)*sin(2*y)"})
    configure(blk, text, {"incplanestress": 0})
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), plain)


def test_deck_string_source_in_3d(oracle):
    rng = np.random.default_rng(73)
    dim, ncell, order, qdeg = 3, (3, 2, 2), 1, 2
    m = R.le_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    funcs = dict(funcs_for(oracle, m, qdeg, dim), **{"source dz": "0.4*x*y-z", "mu": "0.8+0.3*x"})
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, {})
    check_all(run_gpu(blk, m, u, None, len(ref["colind"]), local=True), ref)


@pytest.mark.parametrize("adjoint,lump", [(True, False), (False, True), (True, True)])
def test_adjoint_and_lumped_scatter_options(oracle, adjoint, lump):
    """assemblyManager.cpp:4124-4133: isAdjoint_ -> every column of a row gets res(row).dx(row); lump_mass_ -> every column's
    value lands on the diagonal.  Reference: the restatement's element arrays scattered with that rule."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(74)
    dim, ncell, order, qdeg = 2, (4, 3), 1, 2
    m = R.le_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = fixed_rows(m)
    tr = R.transient_state(rng, m["ndof"])
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    rowptr, colind = ref["rowptr"], ref["colind"]
    expect = np.zeros(len(colind))
    n = m["lids"].shape[1]
    for e, L in enumerate(m["lids"]):
        Je = ref["local_J"][e]
        for i in range(n):
            r = L[i]
            if fixed[r]:
                continue
            lo, hi = rowptr[r], rowptr[r + 1]
            for j in range(n):
                v = Je[i, i] if adjoint else Je[i, j]
                c = r if lump else L[j]
                expect[lo + np.searchsorted(colind[lo:hi], c)] += v
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs, {})
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.full((len(colind),), 9.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, overwrite=True, adjoint=adjoint, lump_mass=lump,
                        **time_kw(blk, tr))
    torch.cuda.synchronize()
    assert blk.info("last_path") == mrhyde_amd.PATH_ROW_GATHER
    # The operator has no mass term and the translation (1, ..., 1) is a rigid-body mode: lumping alone sums every row to
    # zero, so the lumped diagonal is round-off of sums of entries of the size of the unlumped ones.  The error is
    # measured against that size (the adjoint forms sum n copies of the diagonal entry and are of that size themselves).
    scale = np.abs(ref["crs_vals"]).max()
    assert np.abs(expect).max() > (1e-3 * scale if adjoint else 0.0)
    got = vals.cpu().numpy()
    print("adjoint", adjoint, "lump", lump, np.abs(got - expect).max() / scale)
    assert np.abs(got - expect).max() / scale < RTOL
    if lump:  # everything but the diagonal is zero
        rows = np.repeat(np.arange(m["ndof"]), np.diff(rowptr))
        assert np.all(got[rows != colind] == 0.0)
    assert rel_err(res.cpu().numpy(), ref["res"]) < RTOL


@pytest.mark.parametrize("dim,ncell,order", CASES)
def test_get_mass(oracle, dim, ncell, order):
    torch = _torch()
    m = R.le_mesh(oracle, dim, ncell, order)
    qdeg = 2 * order
    blk = make_block(m, PHYS, qdeg)
    E, n = m["lids"].shape
    for w in (None, [1.0, 1.3, 0.7][:dim]):
        mass = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
        blk.get_mass(mass, w)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), R.get_mass(oracle, m, qdeg, w)) < RTOL


def test_set_initial_and_set_dirichlet_with_rows_on_every_component(oracle):
    torch = _torch()
    rng = np.random.default_rng(75)
    dim, ncell, order, qdeg = 2, (4, 3), 1, 2
    m = R.le_mesh(oracle, dim, ncell, order)
    nd, n = m["ndof"], m["lids"].shape[1]
    rowptr, colind = oracle.build_graph(nd, m["lids"])
    fixed = (((m["side_mask"] >> SIDE_BIT["left"]) & 1) == 1).astype(np.uint8)   # dx and dy rows of the left side
    assert all(fixed[m["dof_var"] == v].sum() > 0 for v in range(dim))
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(rowptr, colind))
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, m["nodes"])
    # set_initial: (initial d*, basis) per component and the mass of every component
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    init = {"dx": "0.3+x*y", "dy": rng.uniform(-1, 1, pb["wts"].shape)}
    for v, name in enumerate(R.NAMES[:dim]):
        f = init[name]
        data = R.func_at(oracle, f, pb["ip"]) if isinstance(f, str) else f
        blk.set_function("initial " + name, f if isinstance(f, str) else torch.tensor(f, device="cuda"))
        off = m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]
        oracle.project_rhs(m["lids"], off, data[..., None], pb["basis"], pb["wts"], want_rhs)
    oracle.set_initial_mass(m["lids"], R.get_mass(oracle, m, qdeg), False, rowptr, colind, want_vals)
    rhs = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.set_initial(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    for v in range(dim):
        assert np.abs(want_rhs[m["dof_var"] == v]).max() > 0
    # set_dirichlet: strong rows of both components on the left side
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], be, bs)
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    dirichlet = {"dx": rng.uniform(-2, 2, sb["wts"].shape), "dy": "0.5-y+0.25*nx"}
    for v, name in enumerate(R.NAMES[:dim]):
        f = dirichlet[name]
        dip = R.func_at(oracle, f, sb["ip"], nrm=sb["normals"]) if isinstance(f, str) else f
        blk.set_function("Dirichlet %s left" % name, f if isinstance(f, str) else torch.tensor(f, device="cuda"))
        off = m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]
        dvals, mass = oracle.dirichlet_boundary(n, off, dip, sb["basis"][..., None], sb["wts"], None)
        oracle.set_dirichlet_group(be, m["lids"], fixed, dvals, mass, False, rowptr, colind, want_vals, want_rhs)
        blk.add_dirichlet_group("left", name, be, bs)
    oracle.set_dirichlet_identity(m["lids"], fixed, rowptr, colind, want_vals)
    rhs, vals = torch.zeros_like(rhs), torch.zeros_like(vals)
    blk.set_dirichlet(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    for v in range(dim):
        assert np.abs(want_rhs[(m["dof_var"] == v) & (fixed == 1)]).max() > 0


def test_flux_group_on_dy(oracle):
    torch = _torch()
    rng = np.random.default_rng(76)
    dim, ncell, order, qdeg = 2, (4, 3), 2, 4
    m = R.le_mesh(oracle, dim, ncell, order)
    be, bs = oracle.boundary_sides(dim, ncell, "top")
    sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], be, bs)
    expr = "1.5 + x*nx - 2*y*ny + 0.5*sin(3*x+y)"
    flux = R.func_at(oracle, expr, sb["ip"], nrm=sb["normals"])
    off = m["offsets"][m["varptr"][1]:m["varptr"][2]]
    fixed = np.zeros(m["ndof"], np.uint8)
    fixed[m["lids"][be[0], off[0]]] = 1
    want = np.zeros(m["ndof"])
    oracle.flux_condition(be, m["lids"], off, flux, sb["wts"], sb["basis"][..., None], want, fixed=fixed)
    blk = make_block(m, PHYS, qdeg, fixed=fixed)
    blk.set_function("Flux dy top", expr)
    blk.add_flux_group("top", "dy", be, bs)
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    blk.assemble_boundary(torch.tensor(rng.uniform(-1, 1, m["ndof"]), device="cuda"), res, compute_jacobian=False)
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert rel_err(r, want) < RTOL
    assert len(np.flatnonzero(r)) > 0 and set(np.flatnonzero(r)) <= set(np.flatnonzero(m["dof_var"] == 1))


def test_per_variable_workset_views(oracle):
    torch = _torch()
    rng = np.random.default_rng(77)
    dim, ncell, order, qdeg = 2, (4, 3), 2, 4
    m = R.le_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, transient=tr)
    F = ref["fields"]
    ws = 5
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]), workset_size=ws)
    configure(blk, funcs, {})
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    assert blk.num_worksets() == 3
    w = 1
    e0, e1 = ws * w, min(ws * w + ws, m["nelem"])
    blk.workset_update(w)
    blk.workset_compute_solution(ud, kw["u_prev"], kw["u_stage"])
    blk.workset_compute_residual(ud, True, kw["u_prev"], kw["u_stage"])
    for v, name in enumerate(R.NAMES[:dim]):
        assert rel_err(blk.workset_view_numpy("basis " + name)[..., 0], F["B"][e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("basis_grad " + name), F["G"][e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy(name), F["val"][v].val[e0:e1]) < RTOL
        for d, c in enumerate("xy"):
            assert rel_err(blk.workset_view_numpy("grad(%s)[%s]" % (name, c)), F["grad"][v][d].val[e0:e1]) < RTOL
    assert rel_err(blk.workset_view_numpy("res"), -ref["local_res"][e0:e1]) < RTOL
    assert rel_err(blk.workset_view_numpy("res.dx"), ref["local_J"][e0:e1]) < RTOL


# 3-D Q2: 81 rows per entry, the form of the boundary kernel that gives an entry the whole workgroup (32 rows and fewer:
# one wavefront per entry)
BOUNDARY_CASES = [(2, (4, 3), 1, "left", "top"), (2, (4, 3), 2, "right", "bottom"), (3, (2, 2, 2), 1, "front", "left"),
                  (3, (2, 2, 1), 2, "back", "right")]


@pytest.mark.parametrize("dim,ncell,order,nside,wside", BOUNDARY_CASES)
@pytest.mark.parametrize("form_param", [1.0, -1.0])
def test_traction_and_weak_dirichlet_groups(oracle, dim, ncell, order, nside, wside, form_param):
    """Neumann on one side with different data per component, weak Dirichlet on another with non-zero data, penalty 7,
    accumulated on top of a volume assembly; some rows fixed."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(78)
    m = R.le_mesh(oracle, dim, ncell, order)
    qdeg = 2 * order
    nd = m["ndof"]
    u = rng.uniform(-1, 1, nd)
    tr = R.transient_state(rng, nd)
    fixed = (((m["side_mask"] >> SIDE_BIT["bottom" if "bottom" not in (nside, wside) else "top"]) & 1) == 1).astype(np.uint8)
    funcs = dict(funcs_for(oracle, m, qdeg, dim), mu="0.8+0.3*x")  # at the side points: closed form / deck string
    params = dict(form_param=form_param, penalty=7.0)
    ne, ns = oracle.boundary_sides(dim, ncell, nside)
    we, ws = oracle.boundary_sides(dim, ncell, wside)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    ndata = [0.4, "0.2+x*y-nx", rng.uniform(-1, 1, (len(ne), nqs))][:dim]
    wdata = [rng.uniform(-1, 1, (len(we), nqs)), ("sinprod", 0.7, [1.0, 2.0, 0.5][:dim]), "0.3-x+0.5*y"][:dim]
    as_spec = lambda d: ("array", d) if isinstance(d, np.ndarray) else d
    vol = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    kwb = dict(fixed=fixed, funcs=funcs, params=params, transient=tr)
    bnd = dict(vol, res=np.zeros(nd), crs_vals=np.zeros(len(vol["crs_vals"])))
    bnd = R.add_boundary(oracle, m, qdeg, u, bnd, ne, ns, R.BC_NEUMANN, [as_spec(d) for d in ndata], **kwb)
    bnd = R.add_boundary(oracle, m, qdeg, u, bnd, we, ws, R.BC_WEAK_DIRICHLET, [as_spec(d) for d in wdata], **kwb)
    ref = dict(vol, res=vol["res"] + bnd["res"], crs_vals=vol["crs_vals"] + bnd["crs_vals"])
    assert rel_err(ref["res"], vol["res"]) > 1e-3 and rel_err(ref["crs_vals"], vol["crs_vals"]) > 1e-3
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    for d, name in enumerate(R.NAMES[:dim]):
        for key, f in (("Neumann %s %s" % (name, nside), ndata[d]), ("Dirichlet %s %s" % (name, wside), wdata[d])):
            blk.set_function(key, torch.tensor(f, device="cuda") if isinstance(f, np.ndarray) else f)
    blk.add_boundary_group(nside, mrhyde_amd.BC_NEUMANN, ne, ns)
    blk.add_boundary_group(wside, mrhyde_amd.BC_WEAK_DIRICHLET, we, ws)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    res = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(ref["colind"]), dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    blk.assemble_boundary(ud, res, vals, **kw)
    torch.cuda.synchronize()
    e1, e2 = rel_err(res.cpu().numpy(), ref["res"]), crs_err(vals.cpu().numpy(), ref)
    print("res", e1, "crs", e2)
    assert e1 < RTOL and e2 < RTOL
    # residual only: the matrix is left alone
    res2 = torch.zeros_like(res)
    blk.assemble_boundary(ud, res2, None, compute_jacobian=False, **kw)
    torch.cuda.synchronize()
    assert rel_err(res2.cpu().numpy(), bnd["res"]) < RTOL
    for r in np.flatnonzero(fixed)[:30]:
        assert res2[r].item() == 0.0


def test_options_that_are_not_built_are_refused(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(79)
    dim, ncell, order, qdeg = 2, (4, 3), 1, 2
    m = R.le_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs)
    nd, nnz = m["ndof"], len(ref["colind"])
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, {})
    ud = torch.tensor(u, device="cuda")
    # settings of the reference's constructor whose terms are not built
    for name, value in (("use crystal elasticity", 1), ("Biot", 1), ("use Lame parameters", 0)):
        msg = _untouched_after(lambda r, v: blk.set_physics_parameter(name, value), nd, nnz)
        assert name in msg
    for name, value in (("use crystal elasticity", 0), ("Biot", 0), ("use Lame parameters", 1)):
        blk.set_physics_parameter(name, value)  # the values that leave them off are accepted
    # the bit-reproducible mode and deck strings that read solution fields
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, deterministic=True), nd, nnz)
    assert "MHA_ASSEMBLE_DETERMINISTIC" in msg
    # the interface condition and computeFlux
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    msg = _untouched_after(lambda r, v: blk.add_boundary_group("left", mrhyde_amd.BC_INTERFACE, be, bs), nd, nnz)
    assert "MHA_BC_INTERFACE" in msg and blk.num_boundary_groups() == 0
    gid = blk.add_boundary_group("left", mrhyde_amd.BC_NEUMANN, be, bs)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    flux = torch.full((len(be), nqs), 4.0, dtype=torch.float64, device="cuda")
    msg = _untouched_after(lambda r, v: blk.compute_flux(gid, ud, flux), nd, nnz)
    assert "computeFlux" in msg and bool((flux == 4.0).all())
    # nothing above changed the block: it still assembles the restatement's operator
    check_all(run_gpu(blk, m, u, None, nnz, local=True), ref)
    blk.set_function("mu", "0.5+dx*dx")
    for kw in (dict(path=mrhyde_amd.PATH_POINT_ENGINE), dict(path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True)):
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, **kw), nd, nnz)
        assert "thermal module" in msg
    # the variable list: dim HGRAD variables; an `e` variable on the block would ask for the thermoelastic term
    H = oracle.HGRAD
    for d, variables, order_text in ((2, [(H, 1)] * 3, "dx, dy,"), (3, [(H, 1)] * 4, "dx, dy, dz,"), (3, [(H, 1)] * 2, "dx, dy, dz,"),
                                     (2, [(H, 1), (oracle.HVOL, 0)], "dx, dy,")):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            mrhyde_amd.Block(d, quadrature=2, physics=PHYS, variables=variables)
        assert ei.value.code == 1 and order_text in str(ei.value) and "thermoelastic" in str(ei.value)
