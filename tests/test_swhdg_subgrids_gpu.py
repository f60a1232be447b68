"""HDG subgrids of m x m sub-elements per macro element on the device: mha_swhdg_subgrid_blocks (plain kernel) against the
numpy restatement of tests/swhdg_subgrid_ref.py, mha_swhdg_condensed_subgrid (fused: assembly + dense solve in LDS + Schur
product on the matrix cores) against the restatement AND against the condensation of the plain kernel's blocks, the
sub-iteration driver on a subgrid layout, the scatter into the macro trace system, one size test and the refusals."""
import numpy as np
import pytest

import swhdg_subgrid_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-12          # uncondensed blocks against the restatement: the bound of test_hdg_element_blocks_match_oracle
TOL_SMALL = 1e-10     # condensed m <= 2 against the restatement: the bound of the one-element fused test
# Condensed S, g, du at m = 3 and m = 4: per entry, 10 x the measured spread of two reference solves on these tests' own
# inputs; the measurement, the constants and the seeded cases are in tests/swhdg_subgrid_ref.py (TOL_CONDENSED), and
# tests/test_swhdg_subgrids.py re-measures them on the CPU.
TOL_CONDENSED = R.TOL_CONDENSED
G = R.G
case = R.case


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def make_block(sm, roe=True, tr=None, layout=True):
    import mrhyde_amd
    blk = mrhyde_amd.Block(2, quadrature=2, physics="shallowwaterHybridized", variables=[(0, 1)] * 3)
    blk.set_mesh(sm["nodes"], sm["lids"], sm["offsets"], sm["ndof"])
    blk.set_graph()
    blk.set_physics_parameter("g", G)
    blk.set_physics_parameter("Roe-like stabilization", 1 if roe else 0)
    if tr is not None:
        blk.set_time_integration(True, 2, 2, 1, tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
    if layout:
        blk.set_swhdg_subgrids(sm["m"])
    return blk


def dev(a):
    return _torch().tensor(np.ascontiguousarray(a), device="cuda")


def run_blocks(blk, sm, u, lam, st, ff, tr):
    torch = _torch()
    Em, N = sm["nmacro"], sm["n_int"] + 24
    kw = {} if tr is None else dict(u_prev=dev(tr["u_prev"]), u_stage=dev(tr["u_stage"]))
    res = torch.full((Em, N), 7.0, dtype=torch.float64, device="cuda")
    blocks = torch.full((Em, N, N), 7.0, dtype=torch.float64, device="cuda")
    blk.swhdg_subgrid_blocks(dev(u), dev(lam), res, blocks, side_types=dev(st), farfield=ff, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy(), blocks.cpu().numpy()


def run_condensed(blk, sm, u, lam, st, ff, tr):
    torch = _torch()
    Em, ni = sm["nmacro"], sm["n_int"]
    kw = {} if tr is None else dict(u_prev=dev(tr["u_prev"]), u_stage=dev(tr["u_stage"]))
    S = torch.full((Em, 24, 24), 7.0, dtype=torch.float64, device="cuda")
    g = torch.full((Em, 24), 7.0, dtype=torch.float64, device="cuda")
    du = torch.full((Em, ni), 7.0, dtype=torch.float64, device="cuda")
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    blk.swhdg_condensed_subgrid(dev(u), dev(lam), schur=S, gvec=g, du=du, num_singular=ns, side_types=dev(st), farfield=ff, **kw)
    torch.cuda.synchronize()
    assert int(ns[0]) == 0
    return S.cpu().numpy(), g.cpu().numpy(), du.cpu().numpy()


def check_condensed(got, ref, m, what):
    """m <= 2: the array-relative criterion and bound of the one-element fused test; m = 3, 4: per entry, the measured bound."""
    for x, y, name in zip(got, ref, ("schur", "gvec", "du")):
        if m <= 2:
            d = float(np.abs(x - y).max() / np.abs(y).max())
            print("%s m=%d %s: array-relative difference %.3e (bound %.1e)" % (what, m, name, d, TOL_SMALL))
            assert d < TOL_SMALL, (what, name, d)
        else:
            d = R.entry_err(x, y)
            print("%s m=%d %s: per-entry difference %.3e (bound %.1e)" % (what, m, name, d, TOL_CONDENSED[m]))
            assert d < TOL_CONDENSED[m], (what, name, d)


@pytest.mark.parametrize("steady", [False, True])
def test_m1_equals_the_one_element_kernel(steady):
    """m = 1 through the new entry points equals mha_swhdg_condensed_element on the same inputs (the criterion of
    test_fused_element_step_equals_the_unfused_pipeline: array-relative difference below 1e-11)."""
    torch = _torch()
    sm, u, lam, st, ff, tr = case(1, not steady, ncell=(6, 5))
    blk = make_block(sm, tr=tr)
    blk.set_function("source Hux", ("sinprod", 0.3, [1.3, 0.7, 0.0]))
    new = run_condensed(blk, sm, u, lam, st, ff, tr)
    E = sm["nmacro"]
    kw = {} if tr is None else dict(u_prev=dev(tr["u_prev"]), u_stage=dev(tr["u_stage"]))
    S = torch.zeros((E, 24, 24), dtype=torch.float64, device="cuda")
    g = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    du = torch.zeros((E, 12), dtype=torch.float64, device="cuda")
    blk.swhdg_condensed_element(dev(u), dev(lam), schur=S, gvec=g, du=du, side_types=dev(st), farfield=ff, **kw)
    torch.cuda.synchronize()
    for a, b_, name in zip(new, (S, g, du), ("schur", "gvec", "du")):
        b_ = b_.cpu().numpy()
        d = float(np.abs(a - b_).max() / np.abs(b_).max())
        print("m=1 %s: %.3e" % (name, d))
        assert d < 1e-11, (name, d)
    # and the plain kernel's blocks, condensed by the existing batched condensation
    import mrhyde_amd
    res, blocks = run_blocks(blk, sm, u, lam, st, ff, tr)
    S2, g2, du2, nsing = mrhyde_amd.batched_condense(12, 24, dev(blocks), dev(res))
    assert nsing == 0
    for a, b_, name in zip(new, (S2, g2, du2), ("schur", "gvec", "du")):
        b_ = b_.cpu().numpy()
        assert float(np.abs(a - b_).max() / np.abs(b_).max()) < 1e-11, name


@pytest.mark.parametrize("roe", [True, False])
@pytest.mark.parametrize("transient", [False, True])
@pytest.mark.parametrize("m", [2, 3, 4])
def test_blocks_and_condensed_step_match_the_restatement(oracle, m, transient, roe):
    """Steady and transient, Roe-like and max-eigenvalue stabilisation, interface / far-field / slip macro sides, a warped
    macro mesh, 15 macro elements; no macro element is skipped."""
    sm, u, lam, st, ff, tr = case(m, transient)
    assert all((st == t).any() for t in range(3))
    r_ref, b_ref = R.assemble(oracle, sm, 2, u, lam, st, ff, g=G, roe=roe, transient=tr)
    blk = make_block(sm, roe=roe, tr=tr)
    res, blocks = run_blocks(blk, sm, u, lam, st, ff, tr)
    dr, db = np.abs(res - r_ref).max() / np.abs(r_ref).max(), np.abs(blocks - b_ref).max() / np.abs(b_ref).max()
    print("blocks m=%d: res %.3e blocks %.3e" % (m, dr, db))
    assert dr < RTOL and db < RTOL
    got = run_condensed(blk, sm, u, lam, st, ff, tr)
    check_condensed(got, R.condense(r_ref, b_ref, sm["n_int"]), m, "fused vs restatement")
    check_condensed(got, R.condense(res, blocks, sm["n_int"]), m, "fused vs plain blocks condensed")


def test_two_runs_are_bit_identical():
    sm, u, lam, st, ff, tr = case(4, True)
    blk = make_block(sm, tr=tr)
    a = run_condensed(blk, sm, u, lam, st, ff, tr)
    b = run_condensed(blk, sm, u, lam, st, ff, tr)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("m", [2, 3, 4])
def test_subgrid_solve_on_a_layout_matches_the_restatement(oracle, m):
    """The sub-iteration driver with a layout set: iteration counts, scaled norms, final u and the closing S, g per macro
    element against the restatement's loop (the assertions of test_subgrid_sub_iteration_matches_oracle)."""
    torch = _torch()
    ncell = (4, 3)
    sm = R.subgrid_mesh(ncell, m, warp=R.macro_warp)
    u, lam, st, ff, tr = R.seeded_case(sm, 21 + m, True, dt=0.05 / (max(ncell) * m))
    max_iter, tol = 8, 1e-9
    u_ref, it_ref, sc_ref = R.nonlinear_solver(oracle, sm, 2, u, lam, st, ff, max_iter, tol, g=G, transient=tr)
    assert it_ref.max() < max_iter and it_ref.min() >= 2 and sc_ref.max() <= tol      # converged inside the budget
    blk = make_block(sm, tr=tr)
    ud = dev(u)
    out = blk.swhdg_subgrid_solve(ud, dev(lam), max_iter, tol, side_types=dev(st), farfield=ff, u_prev=dev(tr["u_prev"]),
                                  u_stage=dev(tr["u_stage"]))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    u_gpu = ud.cpu().numpy()
    assert out["num_singular"][0] == 0 and out["iters"].shape == (sm["nmacro"],)
    assert np.array_equal(out["iters"], it_ref)
    assert np.abs(u_gpu - u_ref).max() < 1e-10 * np.abs(u_ref).max()
    assert np.all(out["resnorm"] <= tol) and np.abs(out["resnorm"] - sc_ref).max() < 1e-3 * tol + 1e-6 * sc_ref.max()
    res, b = R.assemble(oracle, sm, 2, u_ref, lam, st, ff, g=G, transient=tr)
    S_ref, g_ref, _ = R.condense(res, b, sm["n_int"])
    assert np.abs(out["schur"] - S_ref).max() < 1e-9 * np.abs(S_ref).max()
    assert np.abs(out["gvec"] - g_ref).max() < 1e-8 * max(np.abs(g_ref).max(), np.abs(res).max())
    # one pass only: one assembly and one update per macro element
    ud = dev(u)
    o1 = blk.swhdg_subgrid_solve(ud, dev(lam), 1, tol, side_types=dev(st), farfield=ff, u_prev=dev(tr["u_prev"]),
                                 u_stage=dev(tr["u_stage"]))
    torch.cuda.synchronize()
    u1_ref, it1, _ = R.nonlinear_solver(oracle, sm, 2, u, lam, st, ff, 1, tol, g=G, transient=tr)
    assert np.all(o1["iters"].cpu().numpy() == 1) and np.array_equal(it1, o1["iters"].cpu().numpy())
    assert np.abs(ud.cpu().numpy() - u1_ref).max() < 1e-11 * np.abs(u1_ref).max()


def test_macro_trace_system_end_to_end(oracle):
    """The condensed blocks of a small mesh scattered through mha_scatter_plan_apply with the macro trace LIDs against
    the numpy assembly of the restatement's condensed blocks."""
    torch = _torch()
    import mrhyde_amd
    import scipy.sparse as sp
    sm, u, lam, st, ff, tr = case(2, True, seed_shift=3, ncell=(4, 3))
    blk = make_block(sm, tr=tr)
    S, g, _ = run_condensed(blk, sm, u, lam, st, ff, tr)
    lids, nrows = sm["trace_lids"], sm["ntrace"]
    plan = mrhyde_amd.ScatterPlan(lids, nrows)
    rowptr, colind = plan.graph()
    vals = torch.zeros(plan.nnz, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(nrows, dtype=torch.float64, device="cuda")
    plan.apply(dev(S), dev(g), rhs, vals, overwrite=True)
    torch.cuda.synchronize()
    r_ref, b_ref = R.assemble(oracle, sm, 2, u, lam, st, ff, g=G, transient=tr)
    S_ref, g_ref, _ = R.condense(r_ref, b_ref, sm["n_int"])
    A_ref = sp.coo_matrix((S_ref.ravel(), (np.repeat(lids, 24, axis=1).ravel(), np.tile(lids, (1, 24)).ravel())), shape=(nrows, nrows)).tocsr()
    A = sp.csr_matrix((vals.cpu().numpy(), colind, rowptr), shape=(nrows, nrows))
    rhs_ref = np.zeros(nrows)
    np.add.at(rhs_ref, lids.ravel(), g_ref.ravel())
    assert abs(A - A_ref).max() < TOL_SMALL * abs(A_ref).max()
    assert np.abs(rhs.cpu().numpy() - rhs_ref).max() < TOL_SMALL * np.abs(rhs_ref).max()
    plan.close()


def test_size_256x256_macro_elements_m2(oracle):
    """256^2 macro elements x m = 2 (262 144 sub-elements): every macro element against the plain kernel's blocks condensed
    with numpy, a strided sample of 1 024 macro elements against the restatement."""
    sm = R.subgrid_mesh((256, 256), 2)
    u, lam, st, ff, tr = R.seeded_case(sm, 77, True, dt=0.05 / 512)
    blk = make_block(sm, tr=tr)
    got = run_condensed(blk, sm, u, lam, st, ff, tr)
    res, blocks = run_blocks(blk, sm, u, lam, st, ff, tr)
    check_condensed(got, R.condense(res, blocks, sm["n_int"]), 2, "size: fused vs plain blocks condensed")
    ks = np.arange(0, sm["nmacro"], 64)
    assert len(ks) >= 1000
    sub, rows = R.select_macros(sm, ks)
    trs = dict(tr, u_prev=tr["u_prev"][rows], u_stage=tr["u_stage"][rows])
    r_ref, b_ref = R.assemble(oracle, sub, 2, u[rows], lam[ks], st[ks], ff, g=G, transient=trs)
    assert np.abs(res[ks] - r_ref).max() < RTOL * np.abs(r_ref).max() and np.abs(blocks[ks] - b_ref).max() < RTOL * np.abs(b_ref).max()
    check_condensed([x[ks] for x in got], R.condense(r_ref, b_ref, sm["n_int"]), 2, "size: fused vs restatement (sample)")


def test_refusals(oracle):
    torch = _torch()
    import mrhyde_amd
    sm, u, lam, st, ff, tr = case(2, False, ncell=(3, 2))
    blk = make_block(sm, layout=False)
    # no layout on a block whose interior unknowns are shared between elements: today's error
    with pytest.raises(mrhyde_amd.MhaError, match="element-local"):
        blk.swhdg_subgrid_solve(dev(u), dev(lam), 2, 1e-9)
    with pytest.raises(mrhyde_amd.MhaError, match="no subgrid layout"):
        run_condensed(blk, sm, u, lam, st, ff, tr)
    with pytest.raises(mrhyde_amd.MhaError, match=r"outside 1\.\.4"):
        blk.set_swhdg_subgrids(5)
    with pytest.raises(mrhyde_amd.MhaError, match="not whole"):
        blk.set_swhdg_subgrids(4)
    blk.set_swhdg_subgrids(2)
    run_condensed(blk, sm, u, lam, st, ff, tr)
    blk.set_function("source H", "0.1*sin(x)")                 # a deck string
    with pytest.raises(mrhyde_amd.MhaError, match="deck-string"):
        run_condensed(blk, sm, u, lam, st, ff, tr)
    blk.set_function("source H", 0.1)
    run_condensed(blk, sm, u, lam, st, ff, tr)
    blk.set_swhdg_subgrids(0)                                  # cleared: the old check is back
    with pytest.raises(mrhyde_amd.MhaError, match="element-local"):
        blk.swhdg_subgrid_solve(dev(u), dev(lam), 2, 1e-9)
