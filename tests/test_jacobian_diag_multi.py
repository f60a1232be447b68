"""CPU side of the matrix-free Jacobian diagonal and multi-vector products (mha_jacobian_diagonal,
mha_apply_jacobian_multi; Block.jacobian_diagonal, Block.apply_jacobian_multi): the prototypes and the constant against
the header, the Python signatures, and the expected-value helper of the diagonal that the GPU tests
(tests/test_jacobian_diag_multi_gpu.py) share -- checked here against a dense matrix of the oracle.

Criterion of the diagonal, per row:  |d_i - A_ii| <= RTOL sum_j |A_ij|  -- the single product's row bound at |x_j| = 1
(tests/test_jacobian_apply.py); the diagonal sums a subset of the terms that product sums."""
import inspect
import os
import re

import numpy as np

from test_jacobian_apply import matrix_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def diagonal_error(d, A):
    """Largest |d_i - A_ii| / sum_j |A_ij| over the rows; rows whose bound is zero must be exactly zero, else inf."""
    want = A.diagonal()
    bound = np.asarray(abs(A).sum(axis=1)).ravel()
    err = np.abs(np.asarray(d) - want)
    zero = bound == 0.0
    if np.any(err[zero] != 0.0):
        return np.inf
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


def test_prototypes_and_constant_equal_the_header():
    import mrhyde_amd
    text = open(os.path.join(ROOT, "include", "mrhyde_amd.h")).read()
    assert re.search(r"int\s+mha_jacobian_diagonal\(mha_context \*ctx, int flags, const double \*u_dev, const double \*u_prev_dev,\s*"
                     r"const double \*u_stage_dev, double \*d_dev\);", text)
    assert re.search(r"int\s+mha_apply_jacobian_multi\(mha_context \*ctx, int flags, const double \*u_dev, const double \*u_prev_dev,\s*"
                     r"const double \*u_stage_dev, int nvec, const double \*x_dev, int64_t ldx,\s*"
                     r"double \*y_dev, int64_t ldy\);", text)
    assert int(re.search(r"#define\s+MHA_APPLY_MAX_VECTORS\s+(\d+)", text).group(1)) == mrhyde_amd.api.APPLY_MAX_VECTORS == 8
    assert "mha_jacobian_diagonal" in mrhyde_amd.api.EXPORTS and "mha_apply_jacobian_multi" in mrhyde_amd.api.EXPORTS
    # the documentation no longer lists the two as missing
    assert not re.search(r"Not built:[^/]*(diag\(A\)|several right-hand sides)", text)


def test_block_method_signatures():
    import mrhyde_amd
    sig = inspect.signature(mrhyde_amd.Block.jacobian_diagonal)
    assert list(sig.parameters) == ["self", "u", "d", "overwrite", "u_prev", "u_stage"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["overwrite"] is False and d["u_prev"] is None and d["u_stage"] is None
    sig = inspect.signature(mrhyde_amd.Block.apply_jacobian_multi)
    assert list(sig.parameters) == ["self", "u", "X", "Y", "transpose", "overwrite", "u_prev", "u_stage"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["transpose"] is False and d["overwrite"] is False and d["u_prev"] is None and d["u_stage"] is None


def test_diagonal_helper_against_a_dense_matrix(oracle):
    """The helper on an oracle matrix (navierstokes Q2/Q1, 2x2 cells, fixed boundary rows) against a dense copy."""
    rng = np.random.default_rng(190)
    H = oracle.HGRAD
    m = oracle.mesh_multi(2, (2, 2), [H] * 3, [2, 1, 2])
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = ((m["side_mask"] != 0) & (m["dof_var"] != 1)).astype(np.uint8)
    # assembled WITHOUT the fixed rows, so that the zeroing of matrix_of is part of what is checked
    ref = oracle.assemble_block(m, oracle.PHYS_NAVIERSTOKES, 4, u, funcs={"viscosity": 0.05}, params=[1, 1, 0])
    n = m["ndof"]
    D = np.zeros((n, n))
    for r in range(n):
        for k in range(ref["rowptr"][r], ref["rowptr"][r + 1]):
            D[r, ref["colind"][k]] += ref["crs_vals"][k]
    assert np.abs(np.diag(D)[fixed != 0]).max() > 0
    D[fixed != 0] = 0.0
    A = matrix_of(ref, fixed)
    d = np.diag(D).copy()
    bound = np.abs(D).sum(axis=1)
    assert diagonal_error(d, A) < 1e-14
    assert np.all(d[fixed != 0] == 0.0) and np.all(bound[fixed != 0] == 0.0)
    # a wrong entry is seen at the size the criterion works at
    free = np.flatnonzero(bound > 0)
    k = int(free[np.argmax(bound[free])])
    bad = d.copy()
    bad[k] += 1e-9 * bound[k]
    assert diagonal_error(bad, A) > 1e-10
    k = int(free[np.argmin(bound[free])])
    bad = d.copy()
    bad[k] -= 1e-9 * bound[k]
    assert diagonal_error(bad, A) > 1e-10
    # anything on a fixed row is an error
    bad = d.copy()
    bad[np.flatnonzero(fixed)[0]] = 1e-30
    assert diagonal_error(bad, A) == np.inf
