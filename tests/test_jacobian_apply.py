"""CPU side of the matrix-free Jacobian products (mha_apply_jacobian, Block.apply_jacobian): the flag constants against
the header, the Python signature, and the expected-value helpers the GPU tests (tests/test_jacobian_apply_gpu.py) share --
checked here against a dense product on an oracle matrix.

Expected values: A = a CRS matrix of the oracle / the Python yardsticks with its fixed rows zeroed; the product in fp64
with scipy.sparse.  Criterion per row:  |y_i - (A x)_i| <= RTOL sum_j |A_ij| |x_j|  (transposed: the same with A^T)."""
import inspect
import os
import re

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draw_x(rng, n):
    """|x_j| in [0.5, 1.5] with random signs: the bound's denominator is at least half the row's largest entry."""
    return rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)


def matrix_of(ref, fixed=None, vals=None):
    """The CRS arrays of `ref` (or `vals` on its graph) as a scipy matrix with the fixed rows zeroed."""
    n = len(ref["rowptr"]) - 1
    A = sp.csr_matrix((np.asarray(ref["crs_vals"] if vals is None else vals, dtype=np.float64), ref["colind"], ref["rowptr"]),
                      shape=(n, n))
    if fixed is not None:
        A = sp.diags(1.0 - np.asarray(fixed, dtype=np.float64)) @ A
    return A.tocsr()


def expected_product(A, x, transpose=False):
    """-> (A x or A^T x, the row bounds sum_j |A_ij| |x_j| of that product)."""
    M = A.T.tocsr() if transpose else A
    return M @ x, abs(M) @ np.abs(x)


def product_error(y, A, x, transpose=False):
    """Largest |y_i - (A x)_i| / sum_j |A_ij| |x_j| over the rows; rows whose bound is zero must be exactly zero."""
    want, bound = expected_product(A, x, transpose)
    d = np.abs(np.asarray(y) - want)
    zero = bound == 0.0
    if np.any(d[zero] != 0.0):
        return np.inf
    return float((d[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


def test_flag_constants_equal_the_header():
    import mrhyde_amd
    text = open(os.path.join(ROOT, "include", "mrhyde_amd.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert mrhyde_amd.api.ASSEMBLE_OVERWRITE == val("MHA_ASSEMBLE_OVERWRITE")
    assert mrhyde_amd.api.APPLY_TRANSPOSE == val("MHA_APPLY_TRANSPOSE")
    # a bit of its own: none of the assembly flags
    others = [val("MHA_ASSEMBLE_" + k) for k in ("JACOBIAN", "OVERWRITE", "ADJOINT", "LUMP_MASS", "DETERMINISTIC")]
    assert all(mrhyde_amd.api.APPLY_TRANSPOSE & o == 0 for o in others)
    assert re.search(r"int\s+mha_apply_jacobian\(mha_context \*ctx, int flags, const double \*u_dev, const double \*u_prev_dev,\s*"
                     r"const double \*u_stage_dev, const double \*x_dev, double \*y_dev\);", text)
    assert "mha_apply_jacobian" in mrhyde_amd.api.EXPORTS


def test_block_apply_jacobian_signature():
    import mrhyde_amd
    sig = inspect.signature(mrhyde_amd.Block.apply_jacobian)
    assert list(sig.parameters) == ["self", "u", "x", "y", "transpose", "overwrite", "u_prev", "u_stage"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["transpose"] is False and d["overwrite"] is False and d["u_prev"] is None and d["u_stage"] is None


def test_expected_value_helper_against_a_dense_product(oracle):
    """The helper on an oracle matrix (navierstokes Q2/Q1, 2x2 cells, fixed boundary rows) against numpy's dense product."""
    rng = np.random.default_rng(90)
    H = oracle.HGRAD
    m = oracle.mesh_multi(2, (2, 2), [H] * 3, [2, 1, 2])
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = ((m["side_mask"] != 0) & (m["dof_var"] != 1)).astype(np.uint8)
    # the oracle leaves fixed rows empty itself: assemble WITHOUT them so that the helper's zeroing is what is checked
    ref = oracle.assemble_block(m, oracle.PHYS_NAVIERSTOKES, 4, u, funcs={"viscosity": 0.05}, params=[1, 1, 0])
    n = m["ndof"]
    D = np.zeros((n, n))
    for r in range(n):
        for k in range(ref["rowptr"][r], ref["rowptr"][r + 1]):
            D[r, ref["colind"][k]] += ref["crs_vals"][k]
    assert np.abs(D[fixed != 0]).max() > 0
    D[fixed != 0] = 0.0
    A = matrix_of(ref, fixed)
    x = draw_x(rng, n)
    assert np.all((np.abs(x) >= 0.5) & (np.abs(x) <= 1.5)) and (x < 0).any() and (x > 0).any()
    for tr in (False, True):
        Dm = D.T if tr else D
        want, bound = expected_product(A, x, tr)
        assert np.abs(want - Dm @ x).max() <= 1e-14 * np.abs(Dm).max() * n
        assert np.abs(bound - np.abs(Dm) @ np.abs(x)).max() <= 1e-14 * np.abs(Dm).max() * n
        assert product_error(Dm @ x, A, x, tr) < 1e-14
        # the bound is at least half the row's largest entry, and a wrong entry is seen
        rowmax = np.abs(Dm).max(axis=1)
        assert np.all(bound >= 0.5 * rowmax)
        bad = Dm @ x
        k = int(np.argmax(rowmax))
        bad[k] += 1e-9 * rowmax[k]
        assert product_error(bad, A, x, tr) > 1e-10
    # forward: fixed rows are exactly zero and anything there is an error; transposed: x on fixed rows does not matter
    y = D @ x
    assert np.all(y[fixed != 0] == 0.0)
    y[np.flatnonzero(fixed)[0]] = 1e-30
    assert product_error(y, A, x) == np.inf
    x2 = x.copy()
    x2[fixed != 0] = 77.0
    assert np.array_equal(expected_product(A, x2, True)[0], expected_product(A, x, True)[0])
