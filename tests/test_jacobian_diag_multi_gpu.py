"""GPU tests of the matrix-free Jacobian diagonal d (+)= diag(A) (mha_jacobian_diagonal, Block.jacobian_diagonal;
kernels/jacobian_diagonal.hip) and of the multi-vector products Y_k (+)= A X_k, A^T X_k (mha_apply_jacobian_multi,
Block.apply_jacobian_multi; kernels/jacobian_apply_multi.hip) for the modules of the point engine.

Expected values: A = the CRS matrix of the CPU oracle or of the Python yardstick that pins the module, fixed rows zeroed
(tests/test_jacobian_apply.py), and the matrix the device's own assemble_jacres stores.
  products, per vector and row   |Y_ki - (A X_k)_i| <= RTOL sum_j |A_ij| |X_kj|      (the single product's criterion)
  diagonal, per row              |d_i - A_ii|       <= RTOL sum_j |A_ij|             (tests/test_jacobian_diag_multi.py)
RTOL = 1e-12, the one the reference modules export.  The diagonal's bound is the product's at |x_j| = 1: the diagonal sums
a subset of the terms that product sums, and the product meets the bound with |x_j| >= 0.5.  Without any assembled matrix:
d_i = (A e_i)_i from the single product for five random free rows.

Shapes: the case builders of tests/test_jacobian_apply_gpu.py -- the smallest at which each mechanism is reached."""
import numpy as np
import pytest

import cdr_ref
import linearelasticity_ref
import ns_thermal_ref
import thermoelastic_ref
from ns_thermal_ref import transient_state, warp
from test_cdr_gpu import FUNC_SETS, _torch, configure, make_block, time_kw
from test_jacobian_apply import draw_x, matrix_of, product_error
from test_jacobian_apply_gpu import _dev, apply, ns_case, porous_case
from test_jacobian_diag_multi import diagonal_error

pytestmark = pytest.mark.gpu
RTOL = 1e-12
assert RTOL == cdr_ref.RTOL == linearelasticity_ref.RTOL == thermoelastic_ref.RTOL == ns_thermal_ref.RTOL
MHA_ERR_INVALID = 1
SENTINEL = 3.25
PAD = -7.75  # what the padding between vectors holds
LIMIT = 160 * 1024


def matrices(blk, u, kw, fixed, ref):
    """-> (the yardstick's matrix, the matrix the device's own assemble_jacres stores)."""
    torch = _torch()
    res = torch.full((len(u),), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((len(ref["colind"]),), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(_dev(u), res, vals, overwrite=True, **kw)  # MHA_PATH_AUTO
    return matrix_of(ref, fixed), matrix_of(ref, fixed, vals.cpu().numpy())


def diagonal(blk, u, kw, d=None, overwrite=True):
    torch = _torch()
    d = torch.full((len(u),), SENTINEL, dtype=torch.float64, device="cuda") if d is None else d
    blk.jacobian_diagonal(_dev(u), d, overwrite=overwrite, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def multi(blk, u, X, transpose, kw, pad=0, Y=None, overwrite=True):
    """Y_k for the rows of X (numpy [K, n]) -> numpy [K, n + pad]; the leading dimension is n + pad, the padding of X and
    of a Y not given holds PAD."""
    torch = _torch()
    K, n = X.shape
    Xd = torch.full((K, n + pad), PAD, dtype=torch.float64, device="cuda")
    Xd[:, :n] = _dev(X)
    if Y is None:
        Y = torch.full((K, n + pad), PAD, dtype=torch.float64, device="cuda")
        Y[:, :n] = SENTINEL
    blk.apply_jacobian_multi(_dev(u), Xd[:, :n], Y[:, :n], transpose=transpose, overwrite=overwrite, **kw)
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def check_diagonal(blk, u, kw, fixed, A_ref, A_dev, seed):
    d = diagonal(blk, u, kw)
    e_ref, e_dev = diagonal_error(d, A_ref), diagonal_error(d, A_dev)
    want = A_ref.diagonal()
    nz = want != 0.0
    print("diagonal error / bound: yardstick %.3e  device matrix %.3e;  max |d_i - A_ii| / |A_ii| = %.3e"
          % (e_ref, e_dev, (np.abs(d - want)[nz] / np.abs(want[nz])).max()))
    assert 1 <= blk.info("jacobian_diag_waves") <= 8 and 0 < blk.info("jacobian_diag_lds_bytes") <= LIMIT
    assert e_ref <= RTOL and e_dev <= RTOL, (e_ref, e_dev)
    if fixed is not None:
        assert np.all(d[np.asarray(fixed) != 0] == 0.0)
    # without any assembled matrix: d_i = (A e_i)_i for five random free rows
    rng = np.random.default_rng(seed)
    bound = np.asarray(abs(A_ref).sum(axis=1)).ravel()
    free = np.flatnonzero(bound > 0)
    for i in rng.choice(free, 5, replace=False):
        ei = np.zeros(len(u))
        ei[i] = 1.0
        got = apply(blk, u, ei, False, kw=kw)[i]
        print("row %d: d_i %.16e  (A e_i)_i %.16e" % (i, d[i], got))
        assert abs(d[i] - got) <= RTOL * bound[i]
    return d


def check_multi(blk, u, kw, fixed, A_ref, A_dev, seed, Ks):
    """Forward and transposed for every K of Ks, each vector against both matrices."""
    rng = np.random.default_rng(seed)
    n = len(u)
    out = {}
    for K in Ks:
        X = np.stack([draw_x(rng, n) for _ in range(K)])
        for transpose in (False, True):
            Y = multi(blk, u, X, transpose, kw)
            errs = [(product_error(Y[k], A_ref, X[k], transpose), product_error(Y[k], A_dev, X[k], transpose)) for k in range(K)]
            kc = blk.info("jacobian_apply_vectors")
            print("K = %d %s (Kc %d, waves %d, LDS %d B): error / bound per vector, yardstick | device matrix: %s"
                  % (K, "transposed" if transpose else "forward", kc, blk.info("jacobian_apply_waves"),
                     blk.info("jacobian_apply_lds_bytes"), "  ".join("%.2e|%.2e" % e for e in errs)))
            assert 1 <= kc <= min(K, 8) and blk.info("jacobian_apply_waves") >= 1
            assert blk.info("jacobian_apply_lds_bytes") <= LIMIT
            for k, (e_ref, e_dev) in enumerate(errs):
                assert e_ref <= RTOL and e_dev <= RTOL, (K, transpose, k, e_ref, e_dev)
            if fixed is not None and not transpose:
                assert np.all(Y[:, np.asarray(fixed) != 0] == 0.0)  # overwrite: exact zeros on fixed rows
            out[K, transpose] = Y
    return out


def check_case(case, seed, Ks):
    blk, m, u, tr, fixed, ref = case
    kw = time_kw(blk, tr)
    A_ref, A_dev = matrices(blk, u, kw, fixed, ref)
    d = check_diagonal(blk, u, kw, fixed, A_ref, A_dev, seed)
    return d, check_multi(blk, u, kw, fixed, A_ref, A_dev, seed + 1000, Ks), (A_ref, A_dev, kw)


@pytest.mark.parametrize("transient", [False, True])
def test_navierstokes_2d_q2q1(oracle, transient):
    """3x3 cells, SUPG + PSPG; steady, and stage 1 of a two-stage scheme.  Nine elements: the last workgroup is partly
    filled.  K = 3 is no power of two, K = 11 takes a second pass with a remainder."""
    case = ns_case(oracle, 2, (3, 3), [1, 1, 0], transient)
    assert case[4].any() and not case[4].all()
    check_case(case, 201, (1, 3, 8, 11))


@pytest.mark.parametrize("fix_uz", [0, 1])
def test_navierstokes_3d_89_dofs(oracle, fix_uz):
    """More dofs than lanes, and the shape at which the LDS limits Kc."""
    case = ns_case(oracle, 3, (2, 2, 2), [1, 1, fix_uz], False)
    blk, m = case[0], case[1]
    assert m["lids"].shape[1] == 89
    d, Y, _ = check_case(case, 202, (8,))
    assert 1 <= blk.info("jacobian_apply_vectors") <= 8
    assert blk.info("jacobian_apply_lds_bytes") <= LIMIT and blk.info("jacobian_diag_lds_bytes") <= LIMIT
    if not fix_uz:  # the reference's uz-offset quirk lives in the point function: the uz rows of A stay empty
        uz = m["dof_var"] == 3
        assert uz.any() and np.all(d[uz] == 0.0) and np.all(Y[8, False][:, uz] == 0.0)


@pytest.mark.parametrize("dim,ncell", [(2, (3, 3)), (3, (2, 2, 2))])
def test_porous_mixed_with_orientation_signs(oracle, dim, ncell):
    """The signs cancel in d and appear on both sides of the products."""
    rng, m, u = porous_case(oracle, dim, ncell)
    assert (m["orient"] < 0).any()
    tr = transient_state(rng, m["ndof"])
    funcs = {"source": ("sinprod", 2.0, [1.1, 0.7, 1.9][:dim]), "Kinv_xx": 1.3, "Kinv_yy": 0.7, "Kinv_zz": 2.1,
             "total_mobility": 1.9}
    ref = oracle.assemble_block(m, oracle.PHYS_POROUS_MIXED, 2, u, funcs=funcs, transient=tr)
    blk = make_block(m, "porousMixed", 2, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    check_case((blk, m, u, tr, None, ref), 203, (3,))


def test_porous_mixed_heterogeneous_permeability(oracle):
    """Element data replace the Kinv_* functions (EXPR = 3)."""
    dim, ncell = 2, (3, 3)
    rng, m, u = porous_case(oracle, dim, ncell, 93)
    E, nq = m["nelem"], oracle.ref_sizes(dim, 1, 2)[1]
    data = np.stack([rng.uniform(0.2, 5.0, E), rng.uniform(-1, 1, E)], 1)
    kinv = np.repeat(1.0 / data[:, :1], nq, axis=1)
    funcs = {"source": ("sinprod", 2.0, [1.1, 0.7]), "total_mobility": 1.9}
    ref = oracle.assemble_block(m, oracle.PHYS_POROUS_MIXED, 2, u,
                                funcs=dict(funcs, Kinv_xx=("array", kinv), Kinv_yy=("array", kinv), Kinv_zz=("array", kinv)))
    blk = make_block(m, "porousMixed", 2, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    blk.set_element_data(data)
    blk.set_physics_parameter("use permeability data", 1)
    check_case((blk, m, u, None, None, ref), 204, (3,))


def test_cdr_functions_of_the_fields(oracle):
    """The "fields" function set of tests/test_cdr_gpu.py (EXPR = 2), transient."""
    rng = np.random.default_rng(94)
    m = cdr_ref.cdr_mesh(oracle, 2, (3, 2), 2)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = transient_state(rng, m["ndof"])
    fixed = ((m["side_mask"] & 0b0011) != 0).astype(np.uint8)
    funcs = FUNC_SETS["fields"](2)
    ref = cdr_ref.assemble(oracle, m, 4, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, "cdr", 4, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    check_case((blk, m, u, tr, fixed, ref), 205, (3,))


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
    check_case((blk, m, u, None, fixed, ref), 206, (3,))


def test_thermoelastic_3d_q2q1_largest_lds_footprint(oracle):
    """linearelasticity + thermal, Q2 displacements with Q1 e (two variable orders on one block), 2x2x1 cells."""
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
    check_case((blk, m, u, tr, fixed, ref), 207, (8,))
    print("diagonal: LDS per workgroup", blk.info("jacobian_diag_lds_bytes"), "waves", blk.info("jacobian_diag_waves"))


# ---- the call contract, on shape 1 ----------------------------------------------------------------------------------

def test_padding_accumulation_and_one_vector(oracle):
    """ld = nrows + 5 with a sentinel in the padding of X and Y: the padding of Y is bit-unchanged, overwriting or not.
    Accumulation: Y ends at start + product.  K = 1 meets the single call's criterion, as the single call does."""
    torch = _torch()
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (3, 3), [1, 1, 0], True, seed=211)
    kw = time_kw(blk, tr)
    A, _ = matrices(blk, u, kw, fixed, ref)
    rng = np.random.default_rng(212)
    n, K, pad = m["ndof"], 3, 5
    X = np.stack([draw_x(rng, n) for _ in range(K)])
    fx = fixed != 0
    for transpose in (False, True):
        M = A.T.tocsr() if transpose else A
        Y = multi(blk, u, X, transpose, kw, pad=pad)
        assert np.all(Y[:, n:] == PAD)
        for k in range(K):
            assert product_error(Y[k, :n], A, X[k], transpose) <= RTOL
        start = rng.uniform(-2, 2, (K, n))
        Yd = torch.full((K, n + pad), PAD, dtype=torch.float64, device="cuda")
        Yd[:, :n] = _dev(start)
        got = multi(blk, u, X, transpose, kw, pad=pad, Y=Yd, overwrite=False)
        assert np.all(got[:, n:] == PAD)
        for k in range(K):
            want, bound = start[k] + M @ X[k], abs(M) @ np.abs(X[k]) + np.abs(start[k])
            err = (np.abs(got[k, :n] - want) / bound).max()
            print("accumulate, transpose = %s, vector %d: %.3e" % (transpose, k, err))
            assert err <= RTOL
        if not transpose:
            assert np.array_equal(got[:, :n][:, fx], start[:, fx])  # forward: fixed rows of Y_k are left alone
        # one vector: the single call's criterion, for the single call too
        y1 = multi(blk, u, X[:1], transpose, kw)[0]
        ys = apply(blk, u, X[0], transpose, kw=kw)
        assert blk.info("jacobian_apply_waves") >= 1
        assert product_error(y1, A, X[0], transpose) <= RTOL and product_error(ys, A, X[0], transpose) <= RTOL
    # the diagonal accumulates too
    d0 = rng.uniform(-2, 2, n)
    d = diagonal(blk, u, kw, d=_dev(d0), overwrite=False)
    bound = np.asarray(abs(A).sum(axis=1)).ravel() + np.abs(d0)
    assert (np.abs(d - (d0 + A.diagonal())) / bound).max() <= RTOL
    assert np.array_equal(d[fx], d0[fx])


def test_refusals_leave_y_and_d_untouched(oracle):
    torch = _torch()
    import mrhyde_amd
    from mrhyde_amd.api import _check, _ptr
    blk, m, u, tr, fixed, ref = ns_case(oracle, 2, (3, 3), [1, 1, 0], False, seed=213)
    n, K = m["ndof"], 3
    kw = time_kw(blk, tr)
    _, A_before = matrices(blk, u, kw, fixed, ref)
    ud = _dev(u)
    X = torch.ones((K, n), dtype=torch.float64, device="cuda")
    Y = torch.full((K, n), SENTINEL, dtype=torch.float64, device="cuda")
    d = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    lib = mrhyde_amd.load_library()

    def refused(call):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            call()
        torch.cuda.synchronize()
        assert ei.value.code == MHA_ERR_INVALID, ei.value
        assert np.all(Y.cpu().numpy() == SENTINEL) and np.all(d.cpu().numpy() == SENTINEL)

    c_multi = lambda flags, nvec, x, ldx, y, ldy: _check(lib.mha_apply_jacobian_multi(
        blk._h, flags, _ptr(ud), None, None, nvec, _ptr(x), ldx, _ptr(y), ldy))
    # ---- the diagonal: any flag but MHA_ASSEMBLE_OVERWRITE (here MHA_ASSEMBLE_JACOBIAN, MHA_APPLY_TRANSPOSE, a bit
    # nothing defines), a null d
    for flags in (1, 32, 64, 2 | 32):
        refused(lambda: _check(lib.mha_jacobian_diagonal(blk._h, flags, _ptr(ud), None, None, _ptr(d))))
    refused(lambda: _check(lib.mha_jacobian_diagonal(blk._h, 2, _ptr(ud), None, None, None)))
    # ---- the products: flags, nvec < 1, short leading dimensions, null pointers
    for flags in (1, 64, 2 | 32 | 4):
        refused(lambda: c_multi(flags, K, X, n, Y, n))
    for nvec in (0, -1):
        refused(lambda: c_multi(2, nvec, X, n, Y, n))
    refused(lambda: c_multi(2, K, X, n - 1, Y, n))
    refused(lambda: c_multi(2, K, X, n, Y, n - 1))
    refused(lambda: c_multi(2, K, None, n, Y, n))
    refused(lambda: c_multi(2, K, X, n, None, n))
    # ---- Python tensors: not 2-D, not contiguous in the last dimension, different shapes
    refused(lambda: blk.apply_jacobian_multi(ud, X[0], Y[0], overwrite=True))
    Xt = torch.ones((n, K), dtype=torch.float64, device="cuda").t()
    assert Xt.shape == X.shape and Xt.stride(1) != 1
    refused(lambda: blk.apply_jacobian_multi(ud, Xt, Y, overwrite=True))
    Yt = torch.full((n, K), SENTINEL, dtype=torch.float64, device="cuda")
    refused(lambda: blk.apply_jacobian_multi(ud, X, Yt.t(), overwrite=True))
    assert np.all(Yt.cpu().numpy() == SENTINEL)
    refused(lambda: blk.apply_jacobian_multi(ud, X[:2], Y, overwrite=True))
    # ---- no graph
    nb = mrhyde_amd.Block(2, quadrature=4, physics="navierstokes", variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
    nb.set_mesh(m["nodes"], m["lids"], m["offsets"], n, None)
    nb.set_orientation(m["orient"])
    refused(lambda: nb.apply_jacobian_multi(ud, X, Y, overwrite=True))
    refused(lambda: nb.jacobian_diagonal(ud, d, overwrite=True))
    # ---- the module's own validation: a function that reads the solution fields on a module without that form
    le = linearelasticity_ref.le_mesh(oracle, 2, (2, 2), 1)
    nl = le["ndof"]
    assert nl <= n
    lb = make_block(le, "linearelasticity", 2)
    lb.set_function("lambda", "1+dx*dx")
    ul = _dev(np.zeros(nl))
    for transpose in (False, True):
        refused(lambda: lb.apply_jacobian_multi(ul, X[:, :nl], Y[:, :nl], transpose=transpose, overwrite=True))
    refused(lambda: lb.jacobian_diagonal(ul, d[:nl], overwrite=True))
    # ---- the Restore guard: after the refusals a plain assembly gives the matrix it gave before, and both calls work
    lb.set_function("lambda", 1.7)
    lres = torch.zeros(nl, dtype=torch.float64, device="cuda")
    lvals = torch.zeros(len(lb.get_graph()[1]), dtype=torch.float64, device="cuda")
    lb.assemble_jacres(ul, lres, lvals, overwrite=True)
    torch.cuda.synchronize()
    assert np.abs(lvals.cpu().numpy()).max() > 0  # an assembly, not a product into nowhere
    _, A_after = matrices(blk, u, kw, fixed, ref)
    assert np.array_equal(A_after.toarray(), A_before.toarray())
    got = multi(blk, u, np.ones((K, n)), False, kw)
    assert all(product_error(got[k], A_before, np.ones(n)) <= RTOL for k in range(K))
    assert diagonal_error(diagonal(blk, u, kw), A_before) <= RTOL
