"""GPU tests of the matrix-free Jacobian products y (+)= A x and y (+)= A^T x (mha_apply_jacobian, Block.apply_jacobian;
kernels/jacobian_apply.hip) for the modules of the point engine.

Expected values (tests/test_jacobian_apply.py): A = the CRS matrix of the CPU oracle or of the Python yardstick that pins
the module, fixed rows zeroed; the product with scipy.sparse in fp64.  Per row
    |y_i - (A x)_i| <= RTOL sum_j |A_ij| |x_j|,   RTOL = 1e-12 (the one the reference modules export),
with |x_j| in [0.5, 1.5] and random signs; the same against the matrix the device's own assemble_jacres stores; and the
adjoint identity w^T (A x) = x^T (A^T w) to RTOL sum_ij |w_i| |A_ij| |x_j| from the forward and the transposed call.

Shapes: the smallest at which each mechanism is reached (warped meshes, random u): 9 elements leave the last workgroup
partly filled, the 89-dof navierstokes element has more dofs than a wavefront has lanes, porousMixed carries orientation
signs on both sides of the product, the 2x2x1 thermoelastic Q2/Q1 block is the largest LDS footprint."""
import numpy as np
import pytest

import cdr_ref
import linearelasticity_ref
import ns_thermal_ref
import thermoelastic_ref
from ns_thermal_ref import rel_err, transient_state, warp
from test_cdr_gpu import FUNC_SETS, _torch, configure, coupled_fixed, coupled_funcs, make_block, time_kw
from test_jacobian_apply import draw_x, expected_product, matrix_of, product_error

pytestmark = pytest.mark.gpu
RTOL = 1e-12
assert RTOL == cdr_ref.RTOL == linearelasticity_ref.RTOL == thermoelastic_ref.RTOL == ns_thermal_ref.RTOL
MHA_ERR_INVALID = 1
SENTINEL = 3.25


def _dev(a):
    return _torch().tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def apply(blk, u, x, transpose, tr=None, y=None, overwrite=True, kw=None):
    """One product -> numpy; y starts as a sentinel unless given."""
    torch = _torch()
    kw = time_kw(blk, tr) if kw is None else kw
    y = torch.full((len(u),), SENTINEL, dtype=torch.float64, device="cuda") if y is None else y
    blk.apply_jacobian(_dev(u), _dev(x), y, transpose=transpose, overwrite=overwrite, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def check_products(blk, m, u, tr, fixed, ref, seed):
    """Forward and transposed product against the yardstick's matrix and the device's own; the adjoint identity."""
    torch = _torch()
    rng = np.random.default_rng(seed)
    n, nnz = m["ndof"], len(ref["colind"])
    kw = time_kw(blk, tr)
    res = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((nnz,), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(_dev(u), res, vals, overwrite=True, **kw)  # MHA_PATH_AUTO
    A_ref, A_dev = matrix_of(ref, fixed), matrix_of(ref, fixed, vals.cpu().numpy())
    x, w = draw_x(rng, n), draw_x(rng, n)
    figures, ys = {}, {}
    for name, vec, transpose in (("forward", x, False), ("transposed", w, True)):
        ys[name] = apply(blk, u, vec, transpose, kw=kw)
        figures[name] = (product_error(ys[name], A_ref, vec, transpose), product_error(ys[name], A_dev, vec, transpose))
        print(name, "error / bound: yardstick %.3e  device matrix %.3e" % figures[name])
    lhs, rhs = float(w @ ys["forward"]), float(x @ ys["transposed"])
    scale = float(np.abs(w) @ (abs(A_ref) @ np.abs(x)))
    print("adjoint identity: |w.Ax - x.A^T w| / sum|w||A||x| = %.3e" % (abs(lhs - rhs) / scale))
    assert blk.info("jacobian_apply_waves") >= 1 and blk.info("jacobian_apply_lds_bytes") <= 160 * 1024
    for name, (e_ref, e_dev) in figures.items():
        assert e_ref <= RTOL and e_dev <= RTOL, (name, e_ref, e_dev)
    assert abs(lhs - rhs) <= RTOL * scale
    if fixed is not None:
        assert np.all(ys["forward"][np.asarray(fixed) != 0] == 0.0)  # overwrite: exact zeros on fixed rows
    return ys, x, w


NS_FUNCS = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5]), "source uz": -0.2, "viscosity": 0.05,
            "density": 1.3}


def ns_case(oracle, dim, ncell, params, transient, seed=91, fixed_rows=True):
    rng = np.random.default_rng(seed)
    H = oracle.HGRAD
    m = warp(oracle.mesh_multi(dim, ncell, [H] * (dim + 1), [2, 1] + [2] * (dim - 1)))
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = (((m["side_mask"] & 0b1100) != 0) & (m["dof_var"] != 1)).astype(np.uint8) if fixed_rows else None
    tr = transient_state(rng, m["ndof"]) if transient else None
    funcs = {k: ((v[0], v[1], v[2][:dim]) if isinstance(v, tuple) else v) for k, v in NS_FUNCS.items()}
    if dim == 2:
        funcs.pop("source uz")
    ref = oracle.assemble_block(m, oracle.PHYS_NAVIERSTOKES, 4, u, funcs=funcs, params=params, fixed=fixed, transient=tr)
    blk = make_block(m, "navierstokes", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, dict(zip(("useSUPG", "usePSPG", "fix_uz_offsets"), params)))
    return blk, m, u, tr, fixed, ref


@pytest.mark.parametrize("transient", [False, True])
def test_navierstokes_2d_q2q1(oracle, transient):
    """3x3 cells, SUPG + PSPG; steady, and stage 1 of a two-stage scheme (alpha_u != 1, alpha_t != 0).  Nine elements: the
    last workgroup is partly filled."""
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (3, 3), [1, 1, 0], transient)
    check_products(blk, m, u, tr, fixed, ref, 1)
    assert m["nelem"] % blk.info("jacobian_apply_waves") != 0 or blk.info("jacobian_apply_waves") == 1


@pytest.mark.parametrize("fix_uz", [0, 1])
def test_navierstokes_3d_89_dofs_on_one_wave(oracle, fix_uz):
    blk, m, u, tr, fixed, ref = ns_case(oracle, 3, (2, 2, 2), [1, 1, fix_uz], False)
    assert m["lids"].shape[1] == 89
    ys, x, w = check_products(blk, m, u, tr, fixed, ref, 2)
    if not fix_uz:  # the reference's uz-offset quirk lives in the point function: the uz rows of A stay empty
        assert np.all(ys["forward"][m["dof_var"] == 3] == 0.0)


def porous_case(oracle, dim, ncell, seed=92):
    rng = np.random.default_rng(seed)
    m = warp(oracle.mesh_multi(dim, ncell, [oracle.HVOL, oracle.HDIV], [0, 1]))
    flip = rng.uniform(size=m["ndof"]) < 0.3  # orientation signs flipped consistently per global face dof
    u0 = m["varptr"][1]
    for e in range(m["nelem"]):
        for f in range(2 * dim):
            if flip[m["lids"][e, m["offsets"][u0 + f]]]:
                m["orient"][e, u0 + f] *= -1
    return rng, m, rng.uniform(-1, 1, m["ndof"])


@pytest.mark.parametrize("dim,ncell", [(2, (3, 3)), (3, (2, 2, 2))])
@pytest.mark.parametrize("transient", [False, True])
def test_porous_mixed_with_orientation_signs(oracle, dim, ncell, transient):
    rng, m, u = porous_case(oracle, dim, ncell)
    tr = transient_state(rng, m["ndof"]) if transient else None
    funcs = {"source": ("sinprod", 2.0, [1.1, 0.7, 1.9][:dim]), "Kinv_xx": 1.3, "Kinv_yy": 0.7, "Kinv_zz": 2.1,
             "total_mobility": 1.9}
    ref = oracle.assemble_block(m, oracle.PHYS_POROUS_MIXED, 2, u, funcs=funcs, transient=tr)
    blk = make_block(m, "porousMixed", 2, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    check_products(blk, m, u, tr, None, ref, 3)


def test_porous_mixed_heterogeneous_permeability(oracle):
    """Element data replace the Kinv_* functions (EXPR = 3); the yardstick takes the same values as per-point arrays."""
    dim, ncell = 2, (3, 3)
    rng, m, u = porous_case(oracle, dim, ncell, 93)
    E, nq = m["nelem"], oracle.ref_sizes(dim, 1, 2)[1]
    data = np.stack([rng.uniform(0.2, 5.0, E), rng.uniform(-1, 1, E)], 1)  # two columns: column 0 is read
    kinv = np.repeat(1.0 / data[:, :1], nq, axis=1)
    funcs = {"source": ("sinprod", 2.0, [1.1, 0.7]), "total_mobility": 1.9}
    ref = oracle.assemble_block(m, oracle.PHYS_POROUS_MIXED, 2, u,
                                funcs=dict(funcs, Kinv_xx=("array", kinv), Kinv_yy=("array", kinv), Kinv_zz=("array", kinv)))
    blk = make_block(m, "porousMixed", 2, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    blk.set_element_data(data)
    blk.set_physics_parameter("use permeability data", 1)
    check_products(blk, m, u, None, None, ref, 4)


def test_cdr_functions_of_the_fields(oracle):
    """The "fields" function set of tests/test_cdr_gpu.py (reaction '0.5*c*c + ...', EXPR = 2), transient."""
    rng = np.random.default_rng(94)
    m = cdr_ref.cdr_mesh(oracle, 2, (3, 2), 2)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = transient_state(rng, m["ndof"])
    fixed = ((m["side_mask"] & 0b0011) != 0).astype(np.uint8)
    funcs = FUNC_SETS["fields"](2)
    ref = cdr_ref.assemble(oracle, m, 4, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, "cdr", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    check_products(blk, m, u, tr, fixed, ref, 5)


def test_navierstokes_cdr_velocity_from_the_fields(oracle):
    """navierstokes+cdr 2-D with xvel 'ux', yvel 'uy' and reaction '0.5*c*c'."""
    rng = np.random.default_rng(95)
    m = cdr_ref.coupled_mesh(oracle, 2, (3, 2), (2, 1, 2))
    u = rng.uniform(-1, 1, m["ndof"])
    tr = transient_state(rng, m["ndof"])
    fixed = coupled_fixed(m)
    funcs = coupled_funcs(2)
    assert funcs["xvel"] == "ux" and funcs["yvel"] == "uy"
    ref = cdr_ref.assemble(oracle, m, 4, u, funcs=funcs, ns_params=(1, 1, 0), fixed=fixed, transient=tr)
    blk = make_block(m, "navierstokes+cdr", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, dict(useSUPG=1, usePSPG=1))
    check_products(blk, m, u, tr, fixed, ref, 6)


def test_thermal_q2_deck_strings_in_the_coordinates(oracle):
    """thermal through its point function (EXPR = 1), against the oracle."""
    rng = np.random.default_rng(96)
    m = warp(oracle.mesh_multi(2, (3, 3), [oracle.HGRAD], [2]))
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = (m["side_mask"] != 0).astype(np.uint8)
    tr = transient_state(rng, m["ndof"])
    funcs = {"thermal source": "2*sin(pi*x)*y", "thermal diffusion": "1.2+0.3*x*y", "density": 0.8, "specific heat": 1.4}
    ref = oracle.assemble_block(m, oracle.PHYS_THERMAL, 4, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, "thermal", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    check_products(blk, m, u, tr, fixed, ref, 7)


def test_thermal_q2_nonlinear_diffusion(oracle):
    """'thermal diffusion' = '1+e*e' (EXPR = 2), against oracle_lib.assemble_thermal_fields."""
    rng = np.random.default_rng(97)
    m = warp(oracle.mesh_multi(2, (3, 3), [oracle.HGRAD], [2]))
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = (m["side_mask"] != 0).astype(np.uint8)
    funcs = {"thermal source": "2*sin(pi*x)*y + 0.1*e", "thermal diffusion": "1+e*e"}
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    ref = oracle.assemble_thermal_fields(2, 2, 4, m["nodes"], m["lids"], m["offsets"], u, funcs, fixed=fixed, rowptr=rowptr,
                                         colind=colind)
    ref = dict(ref, rowptr=rowptr, colind=colind)
    blk = make_block(m, "thermal", 4, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs)
    check_products(blk, m, u, None, fixed, ref, 8)


def test_thermoelastic_3d_q2q1_largest_lds_footprint(oracle):
    """linearelasticity + thermal, Q2 displacements with Q1 e, one cell layer of 2x2x1."""
    rng = np.random.default_rng(98)
    m = thermoelastic_ref.coupled_mesh(oracle, 3, (2, 2, 1), (2, 1))
    u = rng.uniform(-1, 1, m["ndof"])
    tr = transient_state(rng, m["ndof"])
    fixed = ((m["side_mask"] & 0b1100) != 0).astype(np.uint8)
    funcs = {"lambda": ("sinprod", 1.7, [0.9, 1.1, 0.7]), "mu": 0.8, "source dx": 0.3, "source dz": -0.2,
             "thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5]), "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3}
    params = {"alpha_T": 0.35, "T_ambient": 0.3}
    ref = thermoelastic_ref.assemble(oracle, m, 4, u, funcs=funcs, params=params, fixed=fixed, transient=tr)
    blk = make_block(m, "linearelasticity+thermal", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    check_products(blk, m, u, tr, fixed, ref, 9)
    print("LDS per workgroup", blk.info("jacobian_apply_lds_bytes"), "waves", blk.info("jacobian_apply_waves"))


def test_linearelasticity_2d_plane_stress(oracle):
    rng = np.random.default_rng(99)
    m = linearelasticity_ref.le_mesh(oracle, 2, (3, 3), 2)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = ((m["side_mask"] & 0b1100) != 0).astype(np.uint8)
    funcs = {"lambda": ("sinprod", 1.7, [0.9, 1.1]), "mu": 0.8, "source dx": 0.3}
    ref = linearelasticity_ref.assemble(oracle, m, 4, u, funcs=funcs, params={"incplanestress": 1}, fixed=fixed)
    blk = make_block(m, "linearelasticity", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, {"incplanestress": 1})
    check_products(blk, m, u, None, fixed, ref, 10)


def test_navierstokes_thermal_2d_with_buoyancy(oracle):
    rng = np.random.default_rng(100)
    m = ns_thermal_ref.coupled_mesh(oracle, 2, (3, 2), (2, 1, 2))
    u = rng.uniform(-1, 1, m["ndof"])
    tr = transient_state(rng, m["ndof"])
    fixed = coupled_fixed(m)
    funcs = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0]), "viscosity": 0.05, "density": 1.3,
             "thermal source": ("sinprod", 3.0, [2.0, 1.0]), "thermal diffusion": 1.7, "specific heat": 1.4}
    params = dict(useSUPG=1, usePSPG=1, beta=0.7, T_ambient=0.3)
    ref = ns_thermal_ref.assemble(oracle, m, 4, u, funcs=funcs, params=params, fixed=fixed, transient=tr)
    blk = make_block(m, "navierstokes+thermal", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    check_products(blk, m, u, tr, fixed, ref, 11)


def test_fixed_rows_and_accumulation(oracle):
    """Forward + accumulate leaves fixed rows alone; transposed reads x as zero there; two accumulating calls give twice
    the first."""
    torch = _torch()
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (3, 3), [1, 1, 0], False, seed=101)
    rng = np.random.default_rng(12)
    n = m["ndof"]
    A = matrix_of(ref, fixed)
    x = draw_x(rng, n)
    fx = fixed != 0
    assert fx.any() and not fx.all()
    y = torch.full((n,), 5.5, dtype=torch.float64, device="cuda")
    got = apply(blk, u, x, False, y=y, overwrite=False)
    assert np.all(got[fx] == 5.5)  # the sentinel
    assert np.all(got[~fx] != 5.5)
    x2 = x.copy()
    x2[fx] = rng.uniform(50, 100, int(fx.sum()))  # entries the transposed product must not read
    e2 = product_error(apply(blk, u, x2, True), A, x, True)
    print("transposed with x changed on fixed rows: error / bound %.3e" % e2)
    assert e2 <= RTOL
    for transpose in (False, True):
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        y1 = apply(blk, u, x, transpose, y=y, overwrite=False).copy()
        y2 = apply(blk, u, x, transpose, y=y, overwrite=False)
        print("accumulate, transpose =", transpose, rel_err(y2, 2 * y1))
        assert rel_err(y2, 2 * y1) < 1e-14 and np.abs(y1).max() > 0


def test_single_element_mesh(oracle):
    """e_count below the wavefronts per workgroup.  One wavefront adds to every row once: the transposed product with x
    changed on fixed rows is bit-identical."""
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (1, 1), [1, 1, 0], True, seed=102)
    assert m["nelem"] == 1
    ys, x, w = check_products(blk, m, u, tr, fixed, ref, 13)
    assert blk.info("jacobian_apply_waves") > 1
    w2 = w.copy()
    w2[fixed != 0] = -17.0
    assert np.array_equal(apply(blk, u, w2, True, tr), ys["transposed"])


def test_forward_product_is_the_derivative_of_the_residual(oracle):
    """Independent of any Jacobian: the central difference of the device's residual-only assembly at u +- eps x (eps and
    threshold of tests/test_full_size_gpu.py's finite-difference test); res holds -R."""
    torch = _torch()
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (3, 3), [1, 1, 0], False, seed=103)
    n = m["ndof"]
    x = draw_x(np.random.default_rng(14), n)
    eps = 1e-5
    rp_ = torch.zeros(n, dtype=torch.float64, device="cuda")
    rm_ = torch.zeros_like(rp_)
    blk.assemble_jacres(_dev(u + eps * x), rp_, None, compute_jacobian=False, overwrite=True)
    blk.assemble_jacres(_dev(u - eps * x), rm_, None, compute_jacobian=False, overwrite=True)
    fd = -(rp_ - rm_).cpu().numpy() / (2 * eps)
    Jx = apply(blk, u, x, False)
    err = np.abs(fd - Jx).max() / np.abs(Jx).max()
    print("finite difference: %.3e" % err)
    assert err < 1e-7


def test_refusals_leave_y_untouched(oracle):
    torch = _torch()
    import mrhyde_amd
    from mrhyde_amd.api import _check, _ptr
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (1, 1), [0, 0, 0], False, seed=104)
    n = m["ndof"]
    ud, xd = _dev(u), _dev(np.ones(n))
    y = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    lib = mrhyde_amd.load_library()

    def refused(call):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            call()
        torch.cuda.synchronize()
        assert ei.value.code == MHA_ERR_INVALID, ei.value
        assert np.all(y.cpu().numpy() == SENTINEL)

    # an unknown flag bit (here MHA_ASSEMBLE_JACOBIAN, and a bit nothing defines), with and without the known ones
    for flags in (1, 64, 2 | 32 | 4):
        refused(lambda: _check(lib.mha_apply_jacobian(blk._h, flags, _ptr(ud), None, None, _ptr(xd), _ptr(y))))
    refused(lambda: _check(lib.mha_apply_jacobian(blk._h, 2, _ptr(ud), None, None, None, _ptr(y))))  # null x
    # no graph
    nb = mrhyde_amd.Block(2, quadrature=4, physics="navierstokes", variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
    nb.set_mesh(m["nodes"], m["lids"], m["offsets"], n, None)
    nb.set_orientation(m["orient"])
    refused(lambda: nb.apply_jacobian(ud, xd, y, overwrite=True))
    # a function that reads the solution fields on a module without that form
    le = linearelasticity_ref.le_mesh(oracle, 2, (2, 2), 1)
    lb = make_block(le, "linearelasticity", 2)
    lb.set_function("lambda", "1+dx*dx")
    yl = y[:le["ndof"]]
    assert le["ndof"] <= n
    refused(lambda: lb.apply_jacobian(_dev(np.zeros(le["ndof"])), _dev(np.ones(le["ndof"])), yl, overwrite=True))
    refused(lambda: lb.apply_jacobian(_dev(np.zeros(le["ndof"])), _dev(np.ones(le["ndof"])), yl, transpose=True, overwrite=True))
    # and the block still works afterwards
    got = apply(blk, u, np.ones(n), False)
    assert product_error(got, matrix_of(ref, fixed), np.ones(n)) <= RTOL


def test_last_kernel_ms_under_set_timing(oracle):
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (3, 3), [1, 1, 0], False, seed=105)
    blk.set_timing(True)
    apply(blk, u, np.ones(m["ndof"]), False)
    t = blk.last_kernel_ms()
    assert 0.0 < t < 1000.0
