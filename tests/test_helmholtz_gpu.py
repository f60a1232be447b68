"""GPU tests of the helmholtz module ("helmholtz", MHA_PHYSICS_HELMHOLTZ): every case through the C ABI via
mrhyde_amd.Block, against the restatement in tests/helmholtz_ref.py (which tests/test_helmholtz.py pins against the
reference's gold and a central difference).

Shapes, all on warped meshes: 2-D Q1 3x3 q2 (eight elements per workgroup, compile-time point count; nine elements leave
the last workgroup partly filled), 2-D Q2 2x2 q4, 3-D Q1 2x2x2 q2, 3-D Q2 2x2x1 q4 (the large-element form; 54 rows per
side entry: the boundary kernel's workgroup-per-entry form, the others take its wavefront-per-entry form).
Tolerances: RTOL = 1e-12 on residuals relative to the array's largest entry and, per CRS entry,
1e-12 max(|ref|, 1e-3 rowmax) (ns_thermal_ref.crs_err); the matrix-free products and the diagonal as
tests/test_jacobian_apply_gpu.py and tests/test_jacobian_diag_multi_gpu.py check them; the gold as "%.6g" strings."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cdr_ref
import helmholtz_ref as H
from helmholtz_ref import RTOL, crs_err, rel_err
from test_cdr_gpu import _torch, configure, make_block, run_paths, time_kw
from test_helmholtz import constants, fmt
from test_jacobian_apply import matrix_of, product_error, draw_x
from test_jacobian_apply_gpu import apply, check_products
from test_jacobian_diag_multi_gpu import check_case

pytestmark = pytest.mark.gpu

SHAPES = [(2, (3, 3), 1, 2), (2, (2, 2), 2, 4), (3, (2, 2, 2), 1, 2), (3, (2, 2, 1), 2, 4)]
MHA_ERR_INVALID = 1


def gold_strings(dim):
    """the gold deck's strings with its named helpers (3-D: the z pair as the x pair, plus a z term)"""
    f = dict(H.GOLD_FUNCS)
    if dim == 3:
        f.update({"c2r_z": "x*x-1.0+0.25*z", "c2i_z": "2.0*x-z"})
    return f


FUNC_SETS = {"defaults": lambda dim: {}, "constants": constants, "gold": gold_strings}
SIDE_ALPHA = {"robin_alpha_r": "0.3+x", "robin_alpha_i": "y-0.2"}


def case(oracle, dim, ncell, order, seed, transient):
    rng = np.random.default_rng(seed)
    m = H.helmholtz_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = H.transient_state(rng, m["ndof"]) if transient else None
    fixed = ((m["side_mask"] & 0b0001) != 0).astype(np.uint8)  # strong Dirichlet rows on the left side, both variables
    return rng, m, u, tr, fixed


def tensors(m, nnz, rfill=0.0, vfill=0.0):
    torch = _torch()
    return (torch.full((m["ndof"],), rfill, dtype=torch.float64, device="cuda"),
            torch.full((nnz,), vfill, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("fset", list(FUNC_SETS))
@pytest.mark.parametrize("transient", [False, True])
def test_volume_matches_the_yardstick(oracle, dim, ncell, order, qdeg, fset, transient):
    """residual and CRS values on every assembly path the block takes, steady and with transient seeding; strong
    Dirichlet rows get nothing but the overwrite's zeros"""
    rng, m, u, tr, fixed = case(oracle, dim, ncell, order, 81, transient)
    funcs = FUNC_SETS[fset](dim)
    ref = H.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    if fset == "defaults":  # the reference's defaults: residual and matrix are zero
        assert np.all(ref["res"] == 0.0) and np.all(ref["crs_vals"] == 0.0)
    else:
        assert np.abs(ref["res"]).max() > 0.0 and np.abs(ref["crs_vals"]).max() > 0.0
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    if fset == "constants":  # accepted, and read by no built term
        for k, name in enumerate(H.UNUSED_FUNCS):
            blk.set_function(name, 1.5 + k)
    out = run_paths(blk, m, u, tr, ref)
    r3, v3 = out["row-gather"]
    for r in np.flatnonzero(fixed)[:30]:
        assert r3[r] == 0.0 and np.all(v3[ref["rowptr"][r]:ref["rowptr"][r + 1]] == 0.0)
    if fset != "defaults":
        J = sp.csr_matrix((out["atomic"][1], ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2).tocsr()
        free = [np.array([r for r in H.var_rows(m, v) if not fixed[r]]) for v in range(2)]
        for a in range(2):
            for b in range(2):  # every row of one variable couples to both variables
                assert abs(J[free[a]][:, H.var_rows(m, b)]).max() > 0.0


def side_groups(oracle, m):
    return [(nm,) + tuple(oracle.boundary_sides(m["dim"], m["ncell"], nm)) for nm in H.SIDE_NAMES[m["dim"]]]


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("fset,transient", [("all ten", False), ("all ten", True), ("alpha zero", False), ("defaults", False)])
def test_robin_groups_match_the_yardstick(oracle, dim, ncell, order, qdeg, fset, transient):
    """one Neumann group per side name -- entries of every local side id, 4 in 2-D and 6 in 3-D -- with all ten side
    functions non-zero, with robin_alpha_* = 0, and with every function zero (the four N (grad N . n) blocks alone)"""
    torch = _torch()
    import mrhyde_amd
    rng, m, u, tr, fixed = case(oracle, dim, ncell, order, 82, transient)
    fixed = ((m["side_mask"] & 0b1000) != 0).astype(np.uint8)  # top: shares rows with the left and right groups
    if fset == "all ten":
        funcs = dict(gold_strings(dim), **SIDE_ALPHA)
    elif fset == "alpha zero":
        funcs = {k: v for k, v in constants(dim).items() if not k.startswith("robin")}
    else:
        funcs = {}
    groups = side_groups(oracle, m)
    assert sorted(int(g[2][0]) for g in groups) == list(range(2 * dim))
    vol = H.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    rowptr, colind = vol["rowptr"], vol["colind"]
    side = dict(res=np.zeros(m["ndof"]), crs_vals=np.zeros(len(colind)), rowptr=rowptr, colind=colind)
    for _, be, bs in groups:
        add = H.assemble_sides(oracle, m, qdeg, u, be, bs, funcs=funcs, fixed=fixed, transient=tr, rowptr=rowptr, colind=colind)
        side["res"] += add["res"]
        side["crs_vals"] += add["crs_vals"]
    assert np.abs(side["crs_vals"]).max() > 0.0
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs)
    for nm, be, bs in groups:
        blk.add_boundary_group(nm, mrhyde_amd.BC_NEUMANN, be, bs)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    # the groups alone
    res, vals = tensors(m, len(colind))
    blk.assemble_boundary(ud, res, vals, **kw)
    torch.cuda.synchronize()
    r, v = res.cpu().numpy(), vals.cpu().numpy()
    e1, e2 = rel_err(r, side["res"]), crs_err(v, side)
    print("groups alone: res", e1, "crs", e2)
    assert e1 < RTOL and e2 < RTOL
    assert np.all(r[fixed == 1] == 0.0)
    for row in np.flatnonzero(fixed)[:30]:
        assert np.all(v[rowptr[row]:rowptr[row + 1]] == 0.0)
    # the four N (grad N . n) blocks: non-zero between all four variable pairs, so a dropped block cannot pass
    J = sp.csr_matrix((v, colind, rowptr), shape=(m["ndof"],) * 2).tocsr()
    Jr = H.dense(side, m["ndof"]).tocsr()
    free = [np.array([row for row in H.var_rows(m, k) if not fixed[row]]) for k in range(2)]
    for a in range(2):
        for b in range(2):
            assert abs(J[free[a]][:, H.var_rows(m, b)]).max() > 0.0 and abs(Jr[free[a]][:, H.var_rows(m, b)]).max() > 0.0
    # on top of the volume terms, and the residual alone
    ref = dict(vol, res=vol["res"] + side["res"], crs_vals=vol["crs_vals"] + side["crs_vals"])
    res, vals = tensors(m, len(colind), 7.0, -3.0)
    blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    blk.assemble_boundary(ud, res, vals, **kw)
    torch.cuda.synchronize()
    e1, e2 = rel_err(res.cpu().numpy(), ref["res"]), crs_err(vals.cpu().numpy(), ref)
    print("volume + groups: res", e1, "crs", e2)
    assert e1 < RTOL and e2 < RTOL
    res2, _ = tensors(m, 1)
    blk.assemble_boundary(ud, res2, None, compute_jacobian=False, **kw)
    torch.cuda.synchronize()
    assert rel_err(res2.cpu().numpy(), side["res"]) < RTOL


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("fset,transient", [("constants", False), ("gold", True)])
def test_matrix_free_products_and_diagonal(oracle, dim, ncell, order, qdeg, fset, transient):
    """apply_jacobian, its transpose, apply_jacobian_multi (K = 3) and jacobian_diagonal against the yardstick's matrix and
    the crs_vals the same block assembles"""
    rng, m, u, tr, fixed = case(oracle, dim, ncell, order, 83, transient)
    funcs = FUNC_SETS[fset](dim)
    ref = H.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    check_products(blk, m, u, tr, fixed, ref, 5)
    check_case((blk, m, u, tr, fixed, ref), 205, (3,))


def test_views_and_get_mass(oracle):
    torch = _torch()
    rng = np.random.default_rng(84)
    dim, order, qdeg = 2, 2, 4
    m = H.helmholtz_mesh(oracle, dim, (4, 3), order)
    u = rng.uniform(-1, 1, m["ndof"])
    funcs = gold_strings(dim)
    R, J, F = H.volume_arrays(oracle, m, qdeg, u, funcs=funcs)
    ws = 5
    blk = make_block(m, "helmholtz", qdeg, workset_size=ws)
    configure(blk, funcs)
    blk.set_time_integration(False)
    ud = torch.tensor(u, device="cuda")
    assert blk.num_worksets() == 3
    for w in (1, 2):  # a full workset and the ragged last one
        e0, e1 = ws * w, min(ws * w + ws, m["nelem"])
        blk.workset_update(w)
        blk.workset_compute_solution(ud)
        blk.workset_compute_residual(ud, True)
        for v, name in enumerate(("ureal", "uimag")):
            assert rel_err(blk.workset_view_numpy("basis " + name)[..., 0], F["B"][v][e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy("basis_grad " + name), F["G"][v][e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy(name), F["val"][v].val[e0:e1]) < RTOL
            for d, c in enumerate("xy"):
                assert rel_err(blk.workset_view_numpy("grad(%s)[%s]" % (name, c)), F["grad"][v][d].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("res"), R[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("res.dx"), J[e0:e1]) < RTOL
    E, n = m["lids"].shape
    for w in (None, [1.3, 0.7]):
        mass = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
        blk.get_mass(mass, w)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), oracle.get_mass(m, qdeg, w)) < RTOL


def test_set_initial_set_dirichlet_and_the_flux_condition(oracle):
    """what comes with the layout: the L2-projection systems of initial and strong Dirichlet data per variable, and the
    generic Flux condition"""
    torch = _torch()
    rng = np.random.default_rng(85)
    dim, ncell, order, qdeg = 2, (4, 3), 2, 4
    m = H.helmholtz_mesh(oracle, dim, ncell, order)
    nd, n = m["ndof"], m["lids"].shape[1]
    rowptr, colind = oracle.build_graph(nd, m["lids"])
    fixed = ((m["side_mask"] & 1) == 1).astype(np.uint8)
    names = ("ureal", "uimag")
    off = [np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]) for v in range(2)]
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(rowptr, colind))
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    init = {"ureal": "0.3+x*y", "uimag": "1+sin(x)*y"}
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, m["nodes"])
    for v, name in enumerate(names):
        data = H.func_at(oracle, init[name], pb["ip"], None, {})
        blk.set_function("initial " + name, init[name])
        oracle.project_rhs(m["lids"], off[v], data[..., None], pb["basis"], pb["wts"], want_rhs)
    oracle.set_initial_mass(m["lids"], oracle.get_mass(m, qdeg), False, rowptr, colind, want_vals)
    rhs, vals = tensors(m, len(colind))
    blk.set_initial(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    dirichlet = {"ureal": "0.5-y+0.25*nx", "uimag": "2+y*y"}
    sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], be, bs)
    for v, name in enumerate(names):
        dip = H.func_at(oracle, dirichlet[name], sb["ip"], None, {}, nrm=sb["normals"])
        blk.set_function("Dirichlet %s left" % name, dirichlet[name])
        dvals, mass = oracle.dirichlet_boundary(n, off[v], dip, sb["basis"][..., None], sb["wts"], None)
        oracle.set_dirichlet_group(be, m["lids"], fixed, dvals, mass, False, rowptr, colind, want_vals, want_rhs)
        blk.add_dirichlet_group("left", name, be, bs)
    oracle.set_dirichlet_identity(m["lids"], fixed, rowptr, colind, want_vals)
    rhs, vals = tensors(m, len(colind))
    blk.set_dirichlet(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    for v in range(2):
        assert np.abs(want_rhs[(m["dof_var"] == v) & (fixed == 1)]).max() > 0
    te, ts = oracle.boundary_sides(dim, ncell, "top")
    expr = "1.5 + x*nx - 2*y*ny + 0.5*sin(3*x+y)"
    sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], te, ts)
    flux = H.func_at(oracle, expr, sb["ip"], None, {}, nrm=sb["normals"])
    for v in range(2):
        want = np.zeros(nd)
        oracle.flux_condition(te, m["lids"], off[v], flux, sb["wts"], sb["basis"][..., None], want, fixed=fixed)
        b2 = make_block(m, "helmholtz", qdeg, fixed=fixed)
        b2.set_function("Flux %s top" % names[v], expr)
        b2.add_flux_group("top", names[v], te, ts)
        res, _ = tensors(m, 1)
        b2.assemble_boundary(torch.tensor(rng.uniform(-1, 1, nd), device="cuda"), res, compute_jacobian=False)
        torch.cuda.synchronize()
        r = res.cpu().numpy()
        assert rel_err(r, want) < RTOL
        assert len(np.flatnonzero(r)) > 0 and set(np.flatnonzero(r)) <= set(np.flatnonzero(m["dof_var"] == v))


def test_newton_converges_in_one_step(oracle):
    """the problem is linear: one solve, then the residual is at rounding and the driver reports convergence"""
    torch = _torch()
    import mrhyde_amd
    dim, ncell, order, qdeg = SHAPES[0]
    rng, m, _, _, _ = case(oracle, dim, ncell, order, 86, False)
    nd = m["ndof"]
    fixed = ((m["side_mask"] & 0b1101) != 0).astype(np.uint8)
    funcs = gold_strings(dim)
    rowptr, colind = oracle.build_graph(nd, m["lids"])
    gD = 0.3 * rng.uniform(-1, 1, nd)
    u0 = np.where(fixed != 0, gD, 0.0)
    ref = H.assemble(oracle, m, qdeg, u0, funcs=funcs, fixed=fixed, rowptr=rowptr, colind=colind)
    Jr, rhs = H.with_identity_rows(ref, fixed, nd)
    u_ref = u0 + spla.spsolve(Jr.tocsc(), rhs)
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs)
    u = torch.zeros(nd, dtype=torch.float64, device="cuda")
    blk.dirichlet_lift(u, torch.tensor(gD, device="cuda"))
    res, vals = tensors(m, len(colind))
    nw = mrhyde_amd.Newton(blk, max_iter=5, nl_tol=1e-9)
    solves = 0
    while True:
        action = nw.step(u, res, vals)
        if action == mrhyde_amd.NEWTON_DONE:
            break
        assert action == mrhyde_amd.NEWTON_SOLVE
        torch.cuda.synchronize()
        J = sp.csr_matrix((vals.cpu().numpy(), colind, rowptr), shape=(nd, nd))
        nw.update(u, torch.tensor(spla.spsolve(J.tocsc(), res.cpu().numpy()), device="cuda"))
        solves += 1
    st = nw.state()
    assert solves == 1 and st["status"] == 0 and st["resnorm_scaled"] < 1e-9
    assert np.abs(u.cpu().numpy() - u_ref).max() < 1e-10 * np.abs(u_ref).max()


def refused(call):
    import mrhyde_amd
    with pytest.raises(mrhyde_amd.MhaError) as e:
        call()
    assert e.value.code == MHA_ERR_INVALID, e.value


def test_refusals_leave_the_outputs_untouched(oracle):
    torch = _torch()
    import mrhyde_amd
    dim, ncell, order, qdeg = SHAPES[0]
    rng, m, u, tr, fixed = case(oracle, dim, ncell, order, 87, False)
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, constants(dim))
    ud = torch.tensor(u, device="cuda")
    res, vals = tensors(m, len(colind), 7.0, -3.0)

    def untouched():
        torch.cuda.synchronize()
        return bool((res == 7.0).all()) and bool((vals == -3.0).all())
    # fractional != 0 (its volume form names 13 functions); 0 is accepted
    refused(lambda: blk.set_physics_parameter("fractional", 1))
    blk.set_physics_parameter("fractional", 0)
    # MHA_PATH_ROW_OWNER and the deterministic mode
    for ow in (False, True):
        refused(lambda: blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_ROW_OWNER, overwrite=ow))
        refused(lambda: blk.assemble_jacres(ud, res, vals, deterministic=True, overwrite=ow))
        assert untouched()
    # weak-Dirichlet and interface groups
    be, bs = oracle.boundary_sides(dim, ncell, "right")
    refused(lambda: blk.add_boundary_group("right", mrhyde_amd.BC_WEAK_DIRICHLET, be, bs))
    refused(lambda: blk.add_boundary_group("right", mrhyde_amd.BC_INTERFACE, be, bs))
    assert blk.num_boundary_groups() == 0
    # computeFlux is empty in the reference: zeros
    gid = blk.add_boundary_group("right", mrhyde_amd.BC_NEUMANN, be, bs)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    flux = torch.full((len(be), nqs), 3.25, dtype=torch.float64, device="cuda")
    dflux = torch.full((len(be), nqs, m["lids"].shape[1]), 3.25, dtype=torch.float64, device="cuda")
    blk.compute_flux(gid, ud, flux, dflux)
    torch.cuda.synchronize()
    assert bool((flux == 0.0).all()) and bool((dflux == 0.0).all())
    # one of the ten functions as a volume integration-point array while a group exists
    nq = oracle.ref_sizes(dim, order, qdeg)[1]
    blk.set_function("c2r_x", torch.tensor(rng.uniform(1, 2, (m["nelem"], nq)), device="cuda"))
    refused(lambda: blk.assemble_boundary(ud, res, vals))
    assert untouched()
    blk.set_function("c2r_x", 1.3)
    blk.assemble_boundary(ud, res, vals)  # ... and with the constant back it runs
    assert not untouched()
    res, vals = tensors(m, len(colind), 7.0, -3.0)
    # deck strings that read the solution fields: every assembly path, the products and the diagonal
    blk.set_function("omega2r", "1+ureal*ureal")
    for path in (mrhyde_amd.PATH_AUTO, mrhyde_amd.PATH_POINT_ENGINE, mrhyde_amd.PATH_LOCAL_THEN_SCATTER, mrhyde_amd.PATH_ROW_GATHER):
        for ow in (False, True):
            refused(lambda: blk.assemble_jacres(ud, res, vals, path=path, overwrite=ow))
    assert untouched()
    y = torch.full((m["ndof"],), 3.25, dtype=torch.float64, device="cuda")
    refused(lambda: blk.apply_jacobian(ud, ud, y, overwrite=True))
    refused(lambda: blk.jacobian_diagonal(ud, y, overwrite=True))
    Y = torch.full((3, m["ndof"]), 3.25, dtype=torch.float64, device="cuda")
    refused(lambda: blk.apply_jacobian_multi(ud, torch.ones_like(Y), Y, overwrite=True))
    torch.cuda.synchronize()
    assert bool((y == 3.25).all()) and bool((Y == 3.25).all())
    blk.set_function("source_r_side", "uimag")
    blk.set_function("omega2r", 2.1)
    refused(lambda: blk.assemble_boundary(ud, res, vals))
    assert untouched()


def test_shapes_the_module_refuses(oracle):
    import mrhyde_amd
    Hg = oracle.HGRAD
    # two different orders: the reference indexes uimag's basis with ureal's loop index
    refused(lambda: mrhyde_amd.Block(2, quadrature=4, physics="helmholtz", variables=[(Hg, 2), (Hg, 1)]))
    refused(lambda: mrhyde_amd.Block(3, quadrature=2, physics="helmholtz", variables=[(Hg, 1), (Hg, 2)]))
    # one variable, three variables, a wrong basis type
    refused(lambda: mrhyde_amd.Block(2, quadrature=2, physics="helmholtz", variables=[(Hg, 1)]))
    refused(lambda: mrhyde_amd.Block(2, quadrature=2, physics="helmholtz", variables=[(Hg, 1)] * 3))
    refused(lambda: mrhyde_amd.Block(2, quadrature=2, physics="helmholtz", variables=[(Hg, 1), (oracle.HVOL, 1)]))
    # 1-D
    with pytest.raises(mrhyde_amd.MhaError):
        mrhyde_amd.Block(1, quadrature=2, physics="helmholtz", variables=[(Hg, 1), (Hg, 1)])
    mrhyde_amd.Block(2, quadrature=2, physics="helmholtz", variables=[(Hg, 1), (Hg, 1)]).close()


def test_the_gold_on_the_device(oracle):
    """regression/helmholtz/manufactured_solution: the GPU assembles the volume terms and the `right` group of the
    100 x 100 deck, the host solves once"""
    torch = _torch()
    import mrhyde_amd

    def assemble(m, u, funcs, fixed, side):
        rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
        blk = make_block(m, "helmholtz", 2, fixed=fixed, graph=(rowptr, colind))
        configure(blk, funcs)
        blk.add_boundary_group("right", mrhyde_amd.BC_NEUMANN, *side)
        ud = torch.tensor(u, device="cuda")
        res, vals = tensors(m, len(colind), 7.0, -3.0)
        blk.assemble_jacres(ud, res, vals, overwrite=True)
        blk.assemble_boundary(ud, res, vals)
        torch.cuda.synchronize()
        v = vals.cpu().numpy()
        oracle.apply_dbc_diag(fixed, rowptr, colind, v)
        return sp.csr_matrix((v, colind, rowptr), shape=(m["ndof"],) * 2), res.cpu().numpy()
    got = H.gold_manufactured(oracle, assemble)
    assert [fmt(v) for v in got] == ["0.000517267", "0.000222348"], got


def test_existing_modules_still_dispatch(oracle):
    """the widened switch keys (dim * 100 + id): a thermal 2-D and a navierstokes + cdr 3-D assembly through
    MHA_PATH_POINT_ENGINE and a matrix-free product, against the yardsticks and the block's own assembled matrix"""
    torch = _torch()
    import mrhyde_amd
    from test_cdr_gpu import coupled_fixed, coupled_funcs
    rng = np.random.default_rng(88)
    cases = []
    m = cdr_ref.cdr_mesh(oracle, 2, (3, 3), 2)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = ((m["side_mask"] & 0b0011) != 0).astype(np.uint8)
    src = ("sinprod", 2.0, [1.0, 2.0])
    ref = oracle.assemble_thermal(2, 2, 4, m["nodes"], m["lids"], m["offsets"], u, fixed=fixed, diff=0.9, source=src)
    cases.append(("thermal", m, 4, u, fixed, {"thermal diffusion": 0.9, "thermal source": src}, {}, ref))
    m = cdr_ref.coupled_mesh(oracle, 3, (2, 2, 2), (1, 1, 1))
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = coupled_fixed(m)
    funcs = coupled_funcs(3, True)
    ref = cdr_ref.assemble(oracle, m, 2, u, funcs=funcs, ns_params=(1, 1, 0), fixed=fixed)
    cases.append(("navierstokes+cdr", m, 2, u, fixed, funcs, dict(useSUPG=1, usePSPG=1), ref))
    for phys, m, qdeg, u, fixed, funcs, params, ref in cases:
        blk = make_block(m, phys, qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
        configure(blk, funcs, params)
        blk.set_time_integration(False)
        ud = torch.tensor(u, device="cuda")
        res, vals = tensors(m, len(ref["colind"]))
        blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_POINT_ENGINE)
        torch.cuda.synchronize()
        assert blk.info("last_path") == mrhyde_amd.PATH_POINT_ENGINE
        assert rel_err(res.cpu().numpy(), ref["res"]) < RTOL and crs_err(vals.cpu().numpy(), ref) < RTOL, phys
        A = matrix_of(ref, fixed, vals.cpu().numpy())
        x = draw_x(rng, m["ndof"])
        for transpose in (False, True):
            y = apply(blk, u, x, transpose, kw={})
            assert product_error(y, A, x, transpose) <= RTOL, (phys, transpose)
