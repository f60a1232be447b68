"""HDG subgrids of m x m sub-elements per macro element, host side: the numpy restatement (tests/swhdg_subgrid_ref.py) is
pinned against the oracle's one-element restatement, finite differences of its own residual and the divergence theorem;
the layout validator (mha_swhdg_set_subgrids) and the mesh helper (mha_mesh_swhdg_subgrids) are checked without a GPU."""
import numpy as np
import pytest

import swhdg_subgrid_ref as R

TOL = 1e-12  # relative: the tolerance of the existing oracle tests (tests/test_oracle_swhdg.py, tests/test_swhdg_gpu.py)


def test_m1_reproduces_the_one_element_oracle(oracle):
    """m = 1: the restatement's block is orc_swh_hdg_element + the oracle's volume block, the system the existing
    one-element tests condense (transient and steady, Roe-like and max-EV, mixed side types, warped)."""
    sm = R.subgrid_mesh((4, 3), 1, warp=R.macro_warp)
    om = R.oracle_mesh(oracle, sm)
    off = sm["offsets"]
    for transient in (False, True):
        for roe in (True, False):
            u, lam, st, ff, tr = R.seeded_case(sm, 5, transient)
            res, blk = R.assemble(oracle, sm, 2, u, lam, st, ff, g=7.3, roe=roe, transient=tr)
            r0, b0 = oracle.swh_hdg_element(om, 2, u, lam, st, ff, g=7.3, roe=roe, transient=tr)
            vol = oracle.assemble_block(om, oracle.PHYS_SHALLOWWATER_HYBRIDIZED, 2, u, params=[7.3], transient=tr, want_local=True)
            b0[:, :12, :12] += vol["local_J"][:, off][:, :, off]
            r0[:, :12] += vol["local_res"][:, off]
            assert np.abs(res - r0).max() < TOL * np.abs(r0).max(), (transient, roe)
            assert np.abs(blk - b0).max() < TOL * np.abs(b0).max(), (transient, roe)


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("roe", [True, False])
def test_blocks_are_the_derivative_of_the_residual(oracle, m, roe):
    """Central difference of the restatement's own residual along a random direction in (u, lambda): step 1e-6 and bound
    1e-6, the state kept away from the kinks of |eigenvalue|, as the full-size finite-difference test of
    tests/test_full_size_gpu.py does."""
    sm = R.subgrid_mesh((3, 2), m)
    rng = np.random.default_rng(6)
    Em, n = sm["nmacro"], sm["ndof"]
    isH = (np.arange(n) % 3) == 0
    u = 0.3 + 0.05 * rng.uniform(-1, 1, n)
    u[isH] = 1.0 + 0.2 * rng.uniform(0, 1, isH.sum())
    lam = 0.3 + 0.05 * rng.uniform(-1, 1, (Em, 3, 4, 2))
    lam[:, 0] = 1.0 + 0.2 * rng.uniform(0, 1, (Em, 4, 2))
    lam = lam.reshape(Em, 24)
    st = rng.integers(0, 3, (Em, 4)).astype(np.uint8)
    ff = np.array([1.1, 0.35, 0.25])
    du, dl = rng.uniform(-1, 1, n), rng.uniform(-1, 1, (Em, 24))
    res, blk = R.assemble(oracle, sm, 2, u, lam, st, ff, g=1.0, roe=roe)
    eps = 1e-6
    rp, _ = R.assemble(oracle, sm, 2, u + eps * du, lam + eps * dl, st, ff, g=1.0, roe=roe)
    rm, _ = R.assemble(oracle, sm, 2, u - eps * du, lam - eps * dl, st, ff, g=1.0, roe=roe)
    de = np.hstack([du[R.interior_rows(sm)], dl])
    Jd = np.einsum("erc,ec->er", blk, de)
    fd = -(rp - rm) / (2 * eps)                                # the residual arrays hold -res.val()
    assert np.abs(fd - Jd).max() / np.abs(Jd).max() < 1e-6


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_residual_vanishes_for_a_constant_state_with_matching_traces(oracle, m):
    """Divergence theorem on the macro element: the interior sub-sides carry no term because the interior is continuous,
    the boundary sub-sides close the surface; the trace rows hold F(S).n integrated against the trace basis, which sums
    to zero over the closed boundary per equation."""
    sm = R.subgrid_mesh((3, 2), m, warp=R.macro_warp)
    Em, n, ni = sm["nmacro"], sm["ndof"], sm["n_int"]
    const = np.array([1.7, 0.4, -0.3])
    u = np.tile(const, n // 3)
    lam = np.repeat(const, 8)[None].repeat(Em, 0)
    st = np.zeros((Em, 4), np.uint8)
    res, _ = R.assemble(oracle, sm, 2, u, lam, st, np.zeros(3))
    assert np.abs(res[:, :ni]).max() < 1e-12
    assert np.abs(res[:, ni:].reshape(Em, 3, 8).sum(axis=2)).max() < 1e-12
    assert np.abs(res[:, ni:]).max() > 1e-3                  # (the trace rows themselves are the boundary fluxes)


def test_two_reference_solves_agree(oracle):
    """numpy.linalg.solve against the plain Gauss-Jordan of the restatement on a seeded m = 4 case: the two agree far
    inside the GPU tests' bound (which is measured from this difference on their own inputs)."""
    sm = R.subgrid_mesh((3, 2), 4, warp=R.macro_warp)
    u, lam, st, ff, tr = R.seeded_case(sm, 11, True)
    res, blk = R.assemble(oracle, sm, 2, u, lam, st, ff, g=7.3, transient=tr)
    a = R.condense(res, blk, sm["n_int"])
    b = R.condense(res, blk, sm["n_int"], solve=R.gauss_jordan_solve)
    for x, y in zip(a, b):
        assert R.entry_err(x, y) < 1e-9


@pytest.mark.parametrize("m", [3, 4])
def test_the_condensed_bound_is_ten_times_the_measured_spread(oracle, m):
    """The bound of the GPU comparison at m = 3, 4 is 10 x the spread of the two reference solves on the GPU tests' own
    seeded cases: re-measured here, so that a drift of the seeded inputs away from the recorded figure is seen.  (The
    spread is rounding noise of two eliminations: it is held to the record within a factor, not to digits.)"""
    spread = R.reference_spread(oracle, m)
    print("m=%d: measured spread %.3e, recorded %.3e, bound %.3e" % (m, spread, R.SPREAD_MEASURED[m], R.TOL_CONDENSED[m]))
    assert R.TOL_CONDENSED[m] == 10.0 * R.SPREAD_MEASURED[m]
    assert 0.5 * R.SPREAD_MEASURED[m] < spread < 2.0 * R.SPREAD_MEASURED[m]


@pytest.mark.parametrize("ncell,m", [((5, 3), 1), ((4, 3), 2), ((2, 3), 3), ((3, 2), 4)])
def test_mesh_helper(ncell, m):
    import mrhyde_amd
    a = mrhyde_amd.mesh_swhdg_subgrids(ncell, m, lo=(0.5, -1.0), hi=(2.0, 0.25))
    b = R.subgrid_mesh(ncell, m, lo=(0.5, -1.0), hi=(2.0, 0.25))
    Em = ncell[0] * ncell[1]
    assert a["nelem"] == Em * m * m and a["nmacro"] == Em and a["ndof"] == Em * 3 * (m + 1) ** 2 and a["n_int"] == 3 * (m + 1) ** 2
    assert a["ntrace"] == 6 * ((ncell[0] + 1) * ncell[1] + ncell[0] * (ncell[1] + 1))
    for k in ("nodes", "lids", "offsets", "trace_lids"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert len(np.unique(a["lids"])) == a["ndof"] and a["lids"].min() == 0 and a["lids"].max() == a["ndof"] - 1
    assert len(np.unique(a["trace_lids"])) == a["ntrace"]
    # every macro element's rows are its own
    own = a["lids"].reshape(Em, -1)
    assert all(len(np.unique(own[k])) == a["n_int"] for k in range(Em)) and len(np.unique(own // a["n_int"] - np.arange(Em)[:, None])) == 1
    # interior trace rows are shared by exactly two macro elements, boundary ones by one
    cnt = np.bincount(a["trace_lids"].ravel(), minlength=a["ntrace"])
    assert set(np.unique(cnt)) <= {1, 2} and (cnt == 1).sum() == 6 * 2 * (ncell[0] + ncell[1])
    with pytest.raises(mrhyde_amd.MhaError, match="positive"):
        mrhyde_amd.mesh_swhdg_subgrids((0, 2), 2)


def test_layout_validator():
    """mha_test_swhdg_check_subgrids (csrc/test_hooks.h), the host check behind mha_swhdg_set_subgrids: accepts the helper's and a warped mesh,
    rejects a LID shared across macro elements, a broken Q1 connectivity, a non-bilinear sub-mesh and m outside 1..4."""
    import mrhyde_amd
    chk = lambda sm, m=None: mrhyde_amd.check_swhdg_subgrids(sm["m"] if m is None else m, sm["nodes"], sm["lids"], sm["offsets"], sm["ndof"])
    for m in (1, 2, 3, 4):
        chk(R.subgrid_mesh((3, 2), m))
        chk(R.subgrid_mesh((3, 2), m, warp=R.macro_warp))
    sm = R.subgrid_mesh((3, 2), 2)
    bad = dict(sm, lids=sm["lids"].copy())
    bad["lids"][4, 0:3] = sm["lids"][0, 0:3]                 # a vertex of macro element 1 takes rows of macro element 0
    with pytest.raises(mrhyde_amd.MhaError, match="shared by macro elements"):
        chk(bad)
    bad = dict(sm, lids=sm["lids"].copy())
    bad["lids"][1, 0:3] = sm["lids"][1, 3:6]                 # sub-element 1 no longer meets sub-element 0 along their side
    with pytest.raises(mrhyde_amd.MhaError, match="Q1"):
        chk(bad)
    bad = dict(sm, nodes=sm["nodes"].copy())
    mid = np.all(np.isclose(bad["nodes"], bad["nodes"][0, 2]), axis=-1)   # the centre node of macro element 0, in all four sub-elements
    bad["nodes"][mid] += 1e-9
    with pytest.raises(mrhyde_amd.MhaError, match="bilinear"):
        chk(bad)
    with pytest.raises(mrhyde_amd.MhaError, match=r"outside 1\.\.4"):
        chk(R.subgrid_mesh((1, 1), 5), 5)
    with pytest.raises(mrhyde_amd.MhaError, match="whole"):
        chk(R.subgrid_mesh((3, 1), 1), 2)
    bad = dict(sm, lids=sm["lids"].copy())
    bad["lids"][0, 0] = sm["ndof"]                           # a row outside the vector: an error, not a write out of bounds
    with pytest.raises(mrhyde_amd.MhaError, match="out of range"):
        chk(bad)
    bad["lids"][0, 0] = -1
    with pytest.raises(mrhyde_amd.MhaError, match="out of range"):
        chk(bad)
    bad = dict(sm, offsets=sm["offsets"].copy())
    bad["offsets"][3] = 12
    with pytest.raises(mrhyde_amd.MhaError, match="offset"):
        chk(bad)
    bad = dict(sm, lids=sm["lids"].copy())
    bad["lids"][3, 6:9] = sm["lids"][0, 0:3]                 # two distinct nodes of macro element 0 on the same rows
    with pytest.raises(mrhyde_amd.MhaError, match="two of its"):
        chk(bad)


def test_new_symbols_are_declared_and_exported():
    import mrhyde_amd
    lib = mrhyde_amd.load_library()
    for s in ("mha_swhdg_set_subgrids", "mha_swhdg_condensed_subgrid", "mha_swhdg_subgrid_blocks", "mha_mesh_swhdg_subgrids_sizes",
              "mha_mesh_swhdg_subgrids"):
        assert hasattr(lib, s) and s in mrhyde_amd.api.EXPORTS
    assert hasattr(lib, "mha_test_swhdg_check_subgrids") and "mha_test_swhdg_check_subgrids" not in mrhyde_amd.api.EXPORTS
    for name in ("set_swhdg_subgrids", "swhdg_condensed_subgrid", "swhdg_subgrid_blocks"):
        assert hasattr(mrhyde_amd.Block, name)
