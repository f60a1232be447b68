"""The geometry-database step with kept representatives, on the host: the representatives store into a compact buffer
of their own, and a copy plan with that buffer as its separate source writes EVERY CRS entry, the representatives' own
positions included (csrc/block_pattern.hpp BpRepMap, csrc/copy_plan.hpp build_copy_plan_from)."""
import numpy as np
import pytest

import mrhyde_amd


@pytest.mark.parametrize("dim,order,ncell", [(3, 2, (8, 8, 8)), (3, 2, (16, 8, 8)), (3, 1, (12, 8, 8)),
                                              (2, 2, (32, 32)), (3, 2, (9, 7, 6))])
@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.85, 0.0), (0.37, 45.5)])
def test_step_plan_tiles_and_reproduces_every_block(oracle, dim, order, ncell, scales):
    m = mrhyde_amd.mesh_structured(dim, order, ncell)
    nrows = m["ndof"]
    rowptr, colind = oracle.build_graph(nrows, m["lids"])
    n = m["lids"].shape[1]
    nsym = dim * (dim + 1) // 2
    rng = np.random.default_rng(43)
    khat = rng.uniform(-1, 1, (nsym + 1, n * n))
    factors = np.tile(rng.uniform(0.5, 2.0, nsym + 1), (m["nelem"], 1))
    su, st = scales
    full, db, stores, rep_stores, segs, items, info = mrhyde_amd.block_pattern_step_plan(
        dim, m["nodes"], m["lids"], nrows, rowptr, colind, khat, factors, m["boundary"], scale_u=su, scale_t=st,
        num_cus=32, max_patterns=4096)
    nnz = len(colind)
    span = info["span_entries"]
    nrep = info["rep_entries"]
    assert 0 < nrep < nnz and info["rep_items"] > 0 and info["runs"] > 0

    # the representatives: every entry of the compact buffer stored exactly once
    assert rep_stores.shape == (nrep,) and np.all(rep_stores == 1)

    # the plan tiles [0, nnz): segments start at entry 0, strictly ascending, inside the array; one work item per span,
    # in order; every entry below nnz stored exactly once, nothing at or past nnz
    assert segs[0, 0] == 0 and np.all(np.diff(segs[:, 0]) > 0) and segs[-1, 0] < nnz
    assert info["items"] == -(-nnz // span)
    assert np.array_equal(items[:, 0].astype(np.int64) * 16, np.arange(info["items"], dtype=np.int64) * span)
    assert np.all(stores[:nnz] == 1) and np.all(stores[nnz:] == 0)

    # every entry's source lies inside the compact buffer
    e = np.arange(nnz, dtype=np.int64)
    src = e + segs[np.searchsorted(segs[:, 0], e, side="right") - 1, 1]
    assert src.min() >= 0 and src.max() < nrep
    assert len(np.unique(src)) == nrep, "every representative entry is somebody's source"
    # an item's segment range covers its span: its first segment starts at or before the span, the one after its last
    # at or after the span's end
    first, cnt = items[:, 1], items[:, 2]
    s0 = items[:, 0].astype(np.int64) * 16
    assert np.all(segs[first, 0] <= s0)
    nxt = first + cnt
    inside = nxt < len(segs)
    assert np.all(segs[nxt[inside], 0] >= np.minimum(s0 + span, nnz)[inside])

    # plan + host representatives == every block assembled (mha_test_block_patterns_host_apply)
    ref, _ = mrhyde_amd.block_patterns_host_apply(dim, m["nodes"], m["lids"], nrows, rowptr, colind, khat, factors,
                                                  m["boundary"], scale_u=su, scale_t=st, num_cus=32, max_patterns=4096)
    assert not np.any(np.isnan(ref))
    assert np.array_equal(full, ref)
    assert np.array_equal(db, ref)
