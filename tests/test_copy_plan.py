"""Host logic of the database modes' line-aligned copy plan (no GPU): every entry of [0, nnz) is stored at most once and
every copied entry exactly once, by whole-line work items; nothing at or past nnz is stored; the result is the naive
run-by-run copy.  Also the geometry-database plans of the thermal block patterns, against every block assembled."""
import numpy as np
import pytest

import mrhyde_amd


def _naive(vals, runs):
    out = vals.copy()
    for s, d, n in runs:
        out[d:d + n] = vals[s:s + n]
    return out


def _check(nnz, runs, seed=0):
    rng = np.random.default_rng(seed)
    vals = rng.standard_normal(nnz + 40)          # entries past nnz: a larger tensor the caller's view sits in
    vals[nnz:] = np.nan
    want = _naive(vals, runs)
    got = vals.copy()
    stores, info = mrhyde_amd.copy_plan_host_apply(nnz, runs, got)
    copied = np.zeros(nnz, bool)
    for s, d, n in runs:
        copied[d:d + n] = True
    assert np.all(stores[nnz:] == 0), "nothing at or past nnz is stored"
    assert np.all(stores[:nnz] <= 1), "no entry stored twice"
    assert np.all(stores[:nnz][copied] == 1), "every copied entry stored once"
    span = info["span_entries"]
    assert span % 128 == 0
    for b in range(0, nnz, span):                 # a span is stored whole (up to nnz) or not at all
        seg = stores[b:min(b + span, nnz)]
        assert np.all(seg == seg[0])
    assert np.array_equal(got[:nnz], want[:nnz])
    assert np.array_equal(got[nnz:], vals[nnz:], equal_nan=True)
    return info


def _random_runs(rng, nnz, src_len, max_len, gap_max):
    """Runs copying out of [0, src_len) into the rest, with in-place gaps of 0..gap_max entries between them."""
    runs, d = [], src_len + int(rng.integers(0, 3))
    while d < nnz:
        n = int(min(rng.integers(1, max_len + 1), nnz - d))
        s = int(rng.integers(0, src_len - n + 1)) if n <= src_len else None
        if s is None:
            n = src_len
            s = 0
        runs.append((s, d, n))
        d += n + int(rng.integers(0, gap_max + 1))
    return runs


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("nnz,max_len,gap_max", [(5000, 7, 1), (12345, 40, 1), (40001, 300, 3), (3001, 3000, 0),
                                                 (70007, 2000, 50), (1003, 1, 1)])
def test_random_runs(seed, nnz, max_len, gap_max):
    rng = np.random.default_rng(1000 * seed + nnz)
    runs = _random_runs(rng, nnz, 600, max_len, gap_max)
    rng.shuffle(runs)                             # the plan sorts them
    _check(nnz, runs, seed)


def test_many_segments_per_item():
    """Runs of one entry, each with its own offset: a span meets far more segments than the kernel holds at once."""
    nnz, src = 4099, 256
    runs = [((7 * d) % src, d, 1) for d in range(src, nnz, 2)]   # gaps of one in-place entry between them
    info = _check(nnz, runs)
    assert info["max_item_segments"] > 2 * info["segment_registers"]


def test_in_place_only_spans_are_dropped():
    nnz = 10000
    runs = [(0, 5000, 100)]
    info = _check(nnz, runs)
    assert info["items"] <= -(-100 // info["span_entries"]) + 1


def test_no_runs_and_odd_sizes():
    for nnz in (1, 15, 16, 17, 255, 257):
        _check(nnz, [])
        if nnz > 2:
            _check(nnz, [(0, nnz - 1, 1)])


def test_invalid_runs_are_refused():
    vals = np.zeros(100)
    for runs in ([(0, 90, 20)], [(0, 10, 5), (0, 12, 5)], [(20, 10, 5), (0, 20, 5)]):
        with pytest.raises(Exception):
            mrhyde_amd.copy_plan_host_apply(100, runs, vals)


@pytest.mark.parametrize("dim,order,ncell", [(3, 2, (8, 8, 8)), (3, 2, (16, 8, 8)), (3, 1, (12, 8, 8)),
                                              (2, 2, (32, 32)), (3, 2, (9, 7, 6))])
def test_thermal_database_plan(oracle, dim, order, ncell):
    """The thermal runs (block_pattern_copy_runs) copied by the plan reproduce every block assembled, when all
    elements share one geometry record (one set of factors)."""
    m = mrhyde_amd.mesh_structured(dim, order, ncell)
    nrows = m["ndof"]
    rowptr, colind = oracle.build_graph(nrows, m["lids"])
    n = m["lids"].shape[1]
    nsym = dim * (dim + 1) // 2
    rng = np.random.default_rng(41)
    khat = rng.uniform(-1, 1, (nsym + 1, n * n))
    factors = np.tile(rng.uniform(0.5, 2.0, nsym + 1), (m["nelem"], 1))
    full, db, stores, info = mrhyde_amd.block_pattern_copy_plan(dim, m["nodes"], m["lids"], nrows, rowptr, colind,
                                                                khat, factors, m["boundary"], num_cus=32,
                                                                max_patterns=4096)
    nnz = len(colind)
    assert info["runs"] > 0 and info["items"] > 0
    assert not np.any(np.isnan(full))
    assert np.array_equal(db, full), "representatives + copies == every block"
    assert np.all(stores[nnz:] == 0) and np.all(stores[:nnz] <= 1)
