"""GPU tests of the matrix-free boundary-group products: y += A_b x, y += A_b^T x (mha_apply_boundary_jacobian) and
d += diag(A_b) (mha_boundary_jacobian_diagonal), A_b the matrix mha_assemble_boundary(MHA_ASSEMBLE_JACOBIAN) adds into
crs_vals.  Every case builds its block and groups as the named existing test of the module's assembly kernel does and takes
two matrices: A_dev, the crs_vals the same block assembles into zeros, and A_ref, the oracle's / yardstick's boundary matrix
that test compares against.  Criteria and helpers are those of the volume products (tests/test_jacobian_apply.py,
tests/test_jacobian_diag_multi.py): per row |y_i - (A x)_i| <= RTOL sum_j |A_ij| |x_j| with RTOL = 1e-12, rows whose bound
is zero exactly zero; the diagonal at |x_j| = 1."""
import ctypes

import numpy as np
import pytest

import helmholtz_ref as H
import linearelasticity_ref as LE
from test_boundary_gpu import LATE_MODULE_CASES, _groups, warped
from test_boundary_gpu import make_block as thermal_block
from test_cdr_gpu import _torch, configure, make_block, time_kw
from test_jacobian_apply import draw_x, matrix_of, product_error
from test_jacobian_diag_multi import diagonal_error

pytestmark = pytest.mark.gpu

RTOL = 1e-12  # tests/test_jacobian_apply_gpu.py
assert RTOL == H.RTOL == LE.RTOL
MHA_ERR_INVALID = 1
SENTINEL = 3.25
LDS_LIMIT = 64 * 1024


def _dev(a):
    return _torch().tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def product(blk, ud, x, transpose, kw, y=None):
    """One boundary product -> (numpy, the device vector); y starts at zero unless given."""
    torch = _torch()
    y = torch.zeros(len(x), dtype=torch.float64, device="cuda") if y is None else y
    blk.apply_boundary_jacobian(ud, _dev(x), y, transpose=transpose, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy(), y


def diagonal(blk, ud, kw, n):
    torch = _torch()
    d = torch.zeros(n, dtype=torch.float64, device="cuda")
    blk.boundary_jacobian_diagonal(ud, d, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def check_all(blk, u, kw, fixed, rowptr, colind, vals_ref, seed):
    """Products, adjoint identity, diagonal and accumulation of the block's groups against A_ref and A_dev."""
    torch = _torch()
    rng = np.random.default_rng(seed)
    n, nnz = len(u), len(colind)
    graph = dict(rowptr=rowptr, colind=colind, crs_vals=vals_ref)
    ud = _dev(u)
    res = torch.zeros(n, dtype=torch.float64, device="cuda")
    vals = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    blk.assemble_boundary(ud, res, vals, **kw)
    torch.cuda.synchronize()
    vals_b = vals.cpu().numpy()
    A_ref, A_dev = matrix_of(graph, fixed), matrix_of(graph, fixed, vals_b)
    assert abs(A_ref).max() > 0.0 and abs(A_dev).max() > 0.0
    x, w = draw_x(rng, n), draw_x(rng, n)
    figures, ys = {}, {}
    for name, vec, transpose in (("forward", x, False), ("transposed", w, True)):
        ys[name], ydev = product(blk, ud, vec, transpose, kw)
        figures[name] = (product_error(ys[name], A_ref, vec, transpose), product_error(ys[name], A_dev, vec, transpose))
        print(name, "error / bound: yardstick %.3e  device matrix %.3e" % figures[name])
        # a second call on the same y: 2 A_b x
        y2, _ = product(blk, ud, vec, transpose, kw, y=ydev)
        figures[name + " twice"] = (product_error(y2, 2.0 * A_ref, vec, transpose), product_error(y2, 2.0 * A_dev, vec, transpose))
    lhs, rhs = float(w @ ys["forward"]), float(x @ ys["transposed"])
    scale = float(np.abs(w) @ (abs(A_ref) @ np.abs(x)))
    print("adjoint identity: |w.Ax - x.A^T w| / sum|w||A||x| = %.3e" % (abs(lhs - rhs) / scale))
    d = diagonal(blk, ud, kw, n)
    figures["diagonal"] = (diagonal_error(d, A_ref), diagonal_error(d, A_dev))
    print("diagonal error / bound: yardstick %.3e  device matrix %.3e" % figures["diagonal"])
    lds = blk.info("boundary_apply_lds_bytes")
    print("boundary_apply_lds_bytes", lds)
    # volume product first, the boundary product on the same y: (A_vol + A_b) x, both parts assembled by the device
    volres = torch.zeros(n, dtype=torch.float64, device="cuda")
    volvals = torch.full((nnz,), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, volres, volvals, overwrite=True, **kw)
    torch.cuda.synchronize()
    A_sum = matrix_of(graph, fixed, volvals.cpu().numpy() + vals_b)
    for name, vec, transpose in (("volume + boundary", x, False), ("volume + boundary, transposed", w, True)):
        y = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
        blk.apply_jacobian(ud, _dev(vec), y, transpose=transpose, overwrite=True, **kw)
        ysum, _ = product(blk, ud, vec, transpose, kw, y=y)
        figures[name] = (product_error(ysum, A_sum, vec, transpose),) * 2
        print(name, "error / bound of the summed matrix %.3e" % figures[name][0])
    for name, (e_ref, e_dev) in figures.items():
        assert e_ref <= RTOL and e_dev <= RTOL, (name, e_ref, e_dev)
    assert abs(lhs - rhs) <= RTOL * scale
    assert 0 < lds <= LDS_LIMIT
    if fixed is not None and np.any(fixed):
        assert np.all(ys["forward"][np.asarray(fixed) != 0] == 0.0) and np.all(d[np.asarray(fixed) != 0] == 0.0)
    return A_ref, ys, x, w


def untouched(blk, ud, kw=None, n=None):
    """Both calls on sentinel vectors: OK, and every entry bit for bit the sentinel."""
    torch = _torch()
    n = len(ud) if n is None else n
    for call in (lambda y: blk.apply_boundary_jacobian(ud, ud, y, **(kw or {})),
                 lambda y: blk.apply_boundary_jacobian(ud, ud, y, transpose=True, **(kw or {})),
                 lambda y: blk.boundary_jacobian_diagonal(ud, y, **(kw or {}))):
        y = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
        call(y)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all())


def refused(blk, ud, kw=None, text=None):
    """Both calls raise MHA_ERR_INVALID and leave the sentinel."""
    torch = _torch()
    import mrhyde_amd
    msgs = []
    for call in (lambda y: blk.apply_boundary_jacobian(ud, ud, y, **(kw or {})),
                 lambda y: blk.apply_boundary_jacobian(ud, ud, y, transpose=True, **(kw or {})),
                 lambda y: blk.boundary_jacobian_diagonal(ud, y, **(kw or {}))):
        y = torch.full((len(ud),), SENTINEL, dtype=torch.float64, device="cuda")
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            call(y)
        torch.cuda.synchronize()
        assert ei.value.code == MHA_ERR_INVALID, ei.value
        assert bool((y == SENTINEL).all())
        if text:
            assert text in str(ei.value)
        msgs.append(str(ei.value))
    return msgs


# ---- thermal: tests/test_boundary_gpu.py ---------------------------------------------------------------------------
# (2,1,2,(5,4)): 5 and 4 entries per side -- the last workgroup of four waves partly filled; 25 and 27 dofs
THERMAL_SHAPES = [(2, 1, 2, (5, 4)), (2, 4, 8, (3, 2)), (3, 2, 4, (2, 3, 2))]


@pytest.mark.parametrize("dim,order,qdeg,ncell", THERMAL_SHAPES)
@pytest.mark.parametrize("mode", ["steady", "transient", "sf-1"])
def test_thermal_weak_dirichlet_groups(oracle, dim, order, qdeg, ncell, mode):
    """test_boundary_jacres_matches_oracle's block: two Neumann sides (nothing), the other sides weak Dirichlet, 10 % of
    the rows fixed."""
    torch = _torch()
    m = warped(oracle, dim, order, ncell)
    rng = np.random.default_rng(21)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = (rng.uniform(size=m["ndof"]) < 0.1).astype(np.uint8)
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    nqs = oracle.side_sizes(dim, qdeg)[1]
    groups = _groups(oracle, dim, ncell, rng, nqs)
    sf = -1.0 if mode == "sf-1" else 1.0
    tr = None
    if mode == "transient":
        A, b, bdf = np.array([[0.5, 0.0], [0.3, 0.7]]), np.array([0.4, 0.6]), np.array([1.5, -2.0, 0.5])
        tr = dict(u_prev=rng.uniform(-1, 1, (m["ndof"], 2)), u_stage=rng.uniform(-1, 1, (m["ndof"], 2)), stage=1,
                  butcher_A=A, butcher_b=b, bdf=bdf, dt=0.05)
    vals_ref, res_ref = np.zeros(rowptr[-1]), np.zeros(m["ndof"])
    weak_only = np.zeros(rowptr[-1])
    for name, bc, be, bs, data in groups:
        oracle.assemble_thermal_boundary(dim, order, qdeg, m["nodes"], m["lids"], m["offsets"], u, be, bs, bc, data,
                                         rowptr=rowptr, colind=colind, crs_vals=vals_ref, res=res_ref, fixed=fixed,
                                         transient=tr, diff=1.7, form_param=sf)
        if bc == 2:
            oracle.assemble_thermal_boundary(dim, order, qdeg, m["nodes"], m["lids"], m["offsets"], u, be, bs, bc, data,
                                             rowptr=rowptr, colind=colind, crs_vals=weak_only, res=np.zeros(m["ndof"]),
                                             fixed=fixed, transient=tr, diff=1.7, form_param=sf)
    assert np.array_equal(vals_ref, weak_only)  # the Neumann sides have no Jacobian
    blk = thermal_block(m, dim, order, qdeg, fixed=fixed, graph=(rowptr, colind))
    blk.set_function("thermal diffusion", 1.7)
    blk.set_physics_parameter("form_param", sf)
    keep = []
    for name, bc, be, bs, data in groups:
        blk.add_boundary_group(name, bc, be, bs)
        fname = ("Neumann e " if bc == 1 else "Dirichlet e ") + name
        if data[0] == "const":
            blk.set_function(fname, data[1])
        elif data[0] == "sinprod":
            blk.set_function(fname, data)
        else:
            keep.append(torch.tensor(data[1], device="cuda"))
            blk.set_function(fname, keep[-1])
    kw = {}
    if tr is not None:
        blk.set_time_integration(True, 2, 2, 1, tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
        kw = dict(u_prev=torch.tensor(tr["u_prev"], device="cuda"), u_stage=torch.tensor(tr["u_stage"], device="cuda"))
    check_all(blk, u, kw, fixed, rowptr, colind, vals_ref, 301)


def test_thermal_interface_group_with_the_trace_as_an_array(oracle):
    """test_thermal_compute_flux_and_interface_branch's block: MHA_BC_INTERFACE with "aux e <side>" per point."""
    torch = _torch()
    import mrhyde_amd
    dim, order, qdeg, ncell = 3, 1, 2, (3, 2, 2)
    m = warped(oracle, dim, order, ncell)
    rng = np.random.default_rng(5)
    u = rng.uniform(-1, 1, m["ndof"])
    name = "right"
    be, bs = oracle.boundary_sides(dim, ncell, name)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    lam = rng.uniform(-1, 1, (len(be), nqs))
    kappa = 1.7
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    blk = thermal_block(m, dim, order, qdeg, graph=(rowptr, colind))
    blk.set_function("thermal diffusion", kappa)
    blk.add_boundary_group(name, mrhyde_amd.BC_INTERFACE, be, bs)
    lam_d = torch.tensor(lam, device="cuda")
    blk.set_function("aux e " + name, lam_d)
    vals_ref, res_ref = np.zeros(rowptr[-1]), np.zeros(m["ndof"])
    oracle.assemble_thermal_boundary(dim, order, qdeg, m["nodes"], m["lids"], m["offsets"], u, be, bs, 2, ("array", lam),
                                     rowptr=rowptr, colind=colind, crs_vals=vals_ref, res=res_ref, diff=kappa)
    check_all(blk, u, {}, None, rowptr, colind, vals_ref, 302)


# ---- linearelasticity: tests/test_linearelasticity_gpu.py -----------------------------------------------------------
from test_linearelasticity_gpu import BOUNDARY_CASES, SIDE_BIT, funcs_for  # noqa: E402


@pytest.mark.parametrize("dim,ncell,order,nside,wside", BOUNDARY_CASES)
@pytest.mark.parametrize("form_param", [1.0, -1.0])
def test_linearelasticity_nitsche_group(oracle, dim, ncell, order, nside, wside, form_param):
    """test_traction_and_weak_dirichlet_groups' block: traction on one side (adds exactly nothing), Nitsche on another,
    penalty 7, transient, one side's rows fixed.  3-D Q2: 81 rows, the workgroup-per-entry form."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(78)
    m = LE.le_mesh(oracle, dim, ncell, order)
    qdeg = 2 * order
    nd = m["ndof"]
    u = rng.uniform(-1, 1, nd)
    tr = LE.transient_state(rng, nd)
    fixed = (((m["side_mask"] >> SIDE_BIT["bottom" if "bottom" not in (nside, wside) else "top"]) & 1) == 1).astype(np.uint8)
    funcs = dict(funcs_for(oracle, m, qdeg, dim), mu="0.8+0.3*x")
    params = dict(form_param=form_param, penalty=7.0)
    ne, ns = oracle.boundary_sides(dim, ncell, nside)
    we, ws = oracle.boundary_sides(dim, ncell, wside)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    ndata = [0.4, "0.2+x*y-nx", rng.uniform(-1, 1, (len(ne), nqs))][:dim]
    wdata = [rng.uniform(-1, 1, (len(we), nqs)), ("sinprod", 0.7, [1.0, 2.0, 0.5][:dim]), "0.3-x+0.5*y"][:dim]
    as_spec = lambda d: ("array", d) if isinstance(d, np.ndarray) else d
    rowptr, colind = oracle.build_graph(nd, m["lids"])
    kwb = dict(fixed=fixed, funcs=funcs, params=params, transient=tr)
    bnd = dict(rowptr=rowptr, colind=colind, res=np.zeros(nd), crs_vals=np.zeros(len(colind)))
    bnd = LE.add_boundary(oracle, m, qdeg, u, bnd, ne, ns, LE.BC_NEUMANN, [as_spec(d) for d in ndata], **kwb)
    assert np.all(bnd["crs_vals"] == 0.0)  # traction: no Jacobian
    bnd = LE.add_boundary(oracle, m, qdeg, u, bnd, we, ws, LE.BC_WEAK_DIRICHLET, [as_spec(d) for d in wdata], **kwb)
    blk = make_block(m, "linearelasticity", qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs, params)
    for d, name in enumerate(LE.NAMES[:dim]):
        for key, f in (("Neumann %s %s" % (name, nside), ndata[d]), ("Dirichlet %s %s" % (name, wside), wdata[d])):
            blk.set_function(key, torch.tensor(f, device="cuda") if isinstance(f, np.ndarray) else f)
    kw = time_kw(blk, tr)
    # the traction group alone adds exactly nothing
    blk.add_boundary_group(nside, mrhyde_amd.BC_NEUMANN, ne, ns)
    untouched(blk, _dev(u), kw)
    blk.add_boundary_group(wside, mrhyde_amd.BC_WEAK_DIRICHLET, we, ws)
    check_all(blk, u, kw, fixed, rowptr, colind, bnd["crs_vals"], 303)
    if m["lids"].shape[1] > 32:
        assert m["lids"].shape[1] == 81


# ---- helmholtz: tests/test_helmholtz_gpu.py --------------------------------------------------------------------------
from test_helmholtz_gpu import SHAPES, SIDE_ALPHA, gold_strings, side_groups  # noqa: E402


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("transient", [False, True])
def test_helmholtz_robin_groups(oracle, dim, ncell, order, qdeg, transient):
    """test_robin_groups_match_the_yardstick's block with the "all ten" functions: one Robin group per side name, the top
    rows fixed.  3-D Q2: 54 rows, the workgroup-per-entry form."""
    import mrhyde_amd
    rng = np.random.default_rng(82)
    m = H.helmholtz_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = H.transient_state(rng, m["ndof"]) if transient else None
    fixed = ((m["side_mask"] & 0b1000) != 0).astype(np.uint8)
    funcs = dict(gold_strings(dim), **SIDE_ALPHA)
    groups = side_groups(oracle, m)
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    side = dict(crs_vals=np.zeros(len(colind)), rowptr=rowptr, colind=colind)
    for _, be, bs in groups:
        add = H.assemble_sides(oracle, m, qdeg, u, be, bs, funcs=funcs, fixed=fixed, transient=tr, rowptr=rowptr, colind=colind)
        side["crs_vals"] += add["crs_vals"]
    blk = make_block(m, "helmholtz", qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs)
    for nm, be, bs in groups:
        blk.add_boundary_group(nm, mrhyde_amd.BC_NEUMANN, be, bs)
    kw = time_kw(blk, tr)
    A_ref, _, _, _ = check_all(blk, u, kw, fixed, rowptr, colind, side["crs_vals"], 304)
    free = [np.array([row for row in H.var_rows(m, k) if not fixed[row]]) for k in range(2)]
    for a in range(2):
        for b in range(2):  # all four variable-pair blocks: a dropped block cannot pass
            assert abs(A_ref[free[a]][:, H.var_rows(m, b)]).max() > 0.0


# ---- shallowwaterHybridized: tests/test_swhdg_gpu.py -----------------------------------------------------------------
@pytest.mark.parametrize("order,qdeg,ncell", [(1, 2, (4, 3)), (2, 4, (3, 2))])
@pytest.mark.parametrize("bc,roe", [(10, 1), (10, 0), (11, 1), (12, 1)])
def test_shallowwater_hybridized_all_sides(oracle, order, qdeg, ncell, bc, roe):
    """test_boundary_residual_matches_oracle's block: all four sides of every element, per-point trace and far-field
    arrays.  C(q) depends on u: the product must change with it."""
    torch = _torch()
    from test_multi_gpu import make_block as swh_block, warp
    from test_oracle_swhdg import all_element_sides
    rng = np.random.default_rng(61)
    HG = oracle.HGRAD
    m = warp(oracle.mesh_multi(2, ncell, [HG, HG, HG], [order] * 3))
    u = rng.uniform(-1, 1, m["ndof"])
    u[m["dof_var"] == 0] = rng.uniform(1.0, 2.0, (m["dof_var"] == 0).sum())
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    be, bs = all_element_sides(ncell)
    nqs = oracle.side_sizes(2, qdeg)[1]
    shp = (len(be), nqs)
    aux = np.dstack([rng.uniform(1.0, 2.0, shp), rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp)])
    ff = np.dstack([rng.uniform(1.0, 2.0, shp), rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp)])
    vals_ref, res_ref = np.zeros(rowptr[-1]), np.zeros(m["ndof"])
    oracle.assemble_block_boundary(m, oracle.PHYS_SHALLOWWATER_HYBRIDIZED, qdeg, u, be, bs, bc, 0.0, rowptr=rowptr,
                                   colind=colind, crs_vals=vals_ref, res=res_ref, params=[9.81, roe], aux=aux, farfield=ff)
    blk = swh_block(m, "shallowwaterHybridized", qdeg, graph=(rowptr, colind))
    blk.set_physics_parameter("Roe-like stabilization", roe)
    blk.add_boundary_group("skeleton", bc, be, bs)
    keep = []
    for i, v in enumerate(("H", "Hux", "Huy")):
        t = torch.tensor(np.ascontiguousarray(aux[..., i]), device="cuda")
        f = torch.tensor(np.ascontiguousarray(ff[..., i]), device="cuda")
        keep += [t, f]
        blk.set_function("aux %s skeleton" % v, t)
        blk.set_function("Far-field %s skeleton" % v, f)
    _, ys, x, _ = check_all(blk, u, {}, None, rowptr, colind, vals_ref, 305)
    # The slip term divides by H of the interior state: its derivative moves with u.  The interface flux F(Shat) . n +
    # Stab(Shat)(S - Shat) and the far-field term A+(Shat)(S - Shat) - A-(Shat)(Sinf - Shat) are affine in S -- their
    # matrices are functions of the trace state alone -- so there the product must NOT move.
    u2 = u.copy()
    u2[m["dof_var"] == 0] += 0.25
    y2, _ = product(blk, _dev(u2), x, False, {})
    change = np.abs(y2 - ys["forward"]).max() / np.abs(ys["forward"]).max()
    print("relative change of A_b x with u: %.3e" % change)
    assert change > 1e-3 if bc == 12 else change <= RTOL


# ---- nothing to do ---------------------------------------------------------------------------------------------------
def test_blocks_whose_groups_have_no_jacobian_and_a_block_without_groups(oracle):
    torch = _torch()
    import mrhyde_amd
    import cdr_ref
    rng = np.random.default_rng(306)
    dim, ncell = 2, (3, 2)
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    # porousMixed with a weak-Dirichlet group on p: data on the u rows
    m = oracle.mesh_multi(dim, ncell, [oracle.HVOL, oracle.HDIV], [0, 1])
    blk = make_block(m, "porousMixed", 2)
    blk.add_boundary_group("left", mrhyde_amd.BC_WEAK_DIRICHLET, be, bs)
    blk.set_function("Dirichlet p left", 1.5)
    untouched(blk, _dev(rng.uniform(-1, 1, m["ndof"])))
    # cdr: boundaryResidual is empty
    m = cdr_ref.cdr_mesh(oracle, dim, ncell, 1)
    blk = make_block(m, "cdr", 2)
    blk.add_boundary_group("left", mrhyde_amd.BC_NEUMANN, be, bs)
    untouched(blk, _dev(rng.uniform(-1, 1, m["ndof"])))
    # helmholtz without groups
    m = H.helmholtz_mesh(oracle, dim, ncell, 1)
    blk = make_block(m, "helmholtz", 2)
    assert blk.num_boundary_groups() == 0
    untouched(blk, _dev(rng.uniform(-1, 1, m["ndof"])))
    assert blk.info("boundary_apply_lds_bytes") == 0


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(oracle):
    torch = _torch()
    import mrhyde_amd
    lib = mrhyde_amd.load_library()
    dim, ncell, order, qdeg = SHAPES[0]
    rng = np.random.default_rng(307)
    m = H.helmholtz_mesh(oracle, dim, ncell, order)
    blk = make_block(m, "helmholtz", qdeg)
    configure(blk, dict(gold_strings(dim), **SIDE_ALPHA))
    for nm, be, bs in side_groups(oracle, m):
        blk.add_boundary_group(nm, mrhyde_amd.BC_NEUMANN, be, bs)
    ud = _dev(rng.uniform(-1, 1, m["ndof"]))
    y = torch.full((m["ndof"],), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    # flags: MHA_ASSEMBLE_OVERWRITE, MHA_ASSEMBLE_DETERMINISTIC and any other bit; the diagonal takes no flag at all
    for flags in (2, 16, 2 | 32, 16 | 32, 1, 64):
        assert lib.mha_apply_boundary_jacobian(blk._h, flags, p(ud), None, None, p(ud), p(y)) == MHA_ERR_INVALID
    for flags in (2, 16, 32, 1):
        assert lib.mha_boundary_jacobian_diagonal(blk._h, flags, p(ud), None, None, p(y)) == MHA_ERR_INVALID
    # null vectors
    for args in ((None, p(y)), (p(ud), None)):
        for flags in (0, 32):
            assert lib.mha_apply_boundary_jacobian(blk._h, flags, p(ud), None, None, *args) == MHA_ERR_INVALID
    assert lib.mha_boundary_jacobian_diagonal(blk._h, 0, p(ud), None, None, None) == MHA_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    # a side function as a volume-shaped array: the module's own validation, before the first group writes
    nq = oracle.ref_sizes(dim, order, qdeg)[1]
    arr = torch.tensor(rng.uniform(1, 2, (m["nelem"], nq)), device="cuda")
    blk.set_function("c2r_x", arr)
    refused(blk, ud, text="c2r_x")
    blk.set_function("c2r_x", 1.3)
    blk.apply_boundary_jacobian(ud, ud, y)  # ... and with the constant back it runs
    torch.cuda.synchronize()
    assert not bool((y == SENTINEL).all())


@pytest.mark.parametrize("physics,nvars,bc,text", LATE_MODULE_CASES)
def test_group_added_before_its_module_is_selected_is_refused(oracle, physics, nvars, bc, text):
    """test_group_added_before_its_module_is_selected_is_refused_at_assembly, for the products."""
    torch = _torch()
    import mrhyde_amd
    dim, ncell = 2, (2, 2)
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * nvars, [1] * nvars)
    blk = mrhyde_amd.Block(dim, quadrature=2, physics=None, variables=[(oracle.HGRAD, 1)] * nvars)
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], None)
    blk.set_orientation(m["orient"])
    blk.set_graph()
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    blk.add_boundary_group("left", getattr(mrhyde_amd, bc), be, bs)
    assert mrhyde_amd.load_library().mha_physics_select(blk._h, mrhyde_amd.ALL_PHYSICS_IDS[physics]) == 0
    ud = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    for msg in refused(blk, ud):
        assert text in msg and physics + ":" in msg and "'left'" in msg
