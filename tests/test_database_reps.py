"""Host logic of the geometry-database representatives' plan (no GPU): one item per column tile of every unit of every
role's first block, each stored exactly once; every W entry an item loads lies in its unit's class range; the items'
arithmetic reproduces the full plan's values on those blocks bit for bit."""
import numpy as np
import pytest

import mrhyde_amd


@pytest.mark.parametrize("dim,order,ncell", [(3, 2, (8, 8, 8)), (3, 2, (9, 7, 6)), (3, 1, (12, 8, 8)), (2, 2, (32, 32)),
                                              (2, 1, (24, 20))])
def test_rep_plan(oracle, dim, order, ncell):
    m = mrhyde_amd.mesh_structured(dim, order, ncell)
    nrows = m["ndof"]
    rowptr, colind = oracle.build_graph(nrows, m["lids"])
    n = m["lids"].shape[1]
    nsym = dim * (dim + 1) // 2
    rng = np.random.default_rng(7)
    khat = rng.uniform(-1, 1, (nsym + 1, n * n))
    factors = rng.uniform(0.5, 2.0, (m["nelem"], nsym + 1))   # per element: the items read the records, not one value
    full, rep, stores, expect, units, part_tiles, info = mrhyde_amd.block_pattern_rep_plan(
        dim, m["nodes"], m["lids"], nrows, rowptr, colind, khat, factors, m["boundary"], scale_u=0.75, scale_t=1.5,
        num_cus=32, max_patterns=4096)
    assert info["items"] > 0 and info["roles"] > 1

    # every (role, unit, column tile) exactly once
    want = sorted((int(r), p, q) for p, (r, nt) in enumerate(part_tiles) for q in range(nt))
    got = sorted(map(tuple, units.tolist()))
    assert got == want

    # the roles' first blocks are stored exactly once each, nothing else
    rep_entries = expect == 1
    assert rep_entries.any()
    assert np.all(stores[rep_entries] == 1), "every representative entry stored once"
    assert np.all(stores[~rep_entries] == 0), "nothing outside the representatives stored"
    assert np.all(np.isnan(rep[~rep_entries]))

    # the items' arithmetic is the full plan's (products in k-step order), fixed rows zero
    assert not np.any(np.isnan(full))
    assert np.array_equal(rep[rep_entries], full[rep_entries])
    fixed_rows = np.flatnonzero(m["boundary"])
    fixed_entries = np.zeros(len(colind), bool)
    for r in fixed_rows:
        fixed_entries[rowptr[r]:rowptr[r + 1]] = True
    assert np.all(rep[rep_entries & fixed_entries] == 0.0)
    assert np.any(rep[rep_entries & ~fixed_entries] != 0.0)
