"""Host-side plans of the affine row-owner path (csrc/row_owner_plan.hpp) and of the porousMixed direct form and its
database mode (csrc/porous_plan.hpp), through the test hooks (no GPU)."""
import numpy as np
import pytest

import mrhyde_amd

RTOL = 1e-12  # of the reference tables, as in test_thermal_gpu.py
HVOL, HDIV = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV
GEO_DET, GEO_J, GEO_XC = 6, 7, 16  # layout of a geometry record (kernels/device_types.hpp)


def _geo(nodes):
    """Geometry records [E][20] of the elements' corner maps: J from the edges at vertex 0 (exact for affine elements),
    detJ J^-1 J^-T (upper triangle), detJ, J row-major, centroid."""
    ne, _, dim = nodes.shape
    J = np.stack([(nodes[:, k] - nodes[:, 0]) / 2 for k in (1, 3, 4)[:dim]], axis=2)  # J[e][r][c] = d x_r / d xi_c
    det = np.linalg.det(J)
    Ji = np.linalg.inv(J)
    G = det[:, None, None] * Ji @ Ji.transpose(0, 2, 1)
    geo = np.zeros((ne, 20))
    k = 0
    for a in range(dim):
        for c in range(a, dim):
            geo[:, k] = G[:, a, c]
            k += 1
    geo[:, GEO_DET] = det
    geo[:, GEO_J:GEO_J + dim * dim] = J.reshape(ne, -1)
    geo[:, GEO_XC:GEO_XC + dim] = nodes.mean(axis=1)
    return geo


def _check_k1_plan(m, p):
    ne, n = m["lids"].shape
    G = (ne + 255) // 256
    we = p["wg_elems"]
    assert len(we) == G * 256 and np.array_equal(np.sort(we[:ne]), np.arange(ne)), "every element once"
    assert np.all(we[ne:] == we[ne - 1]), "padding repeats the last element"
    assert p["row_ptr"][0] == 0 and p["row_ptr"][-1] == len(p["rows"])
    for g in range(G):
        rows = p["rows"][p["row_ptr"][g]:p["row_ptr"][g + 1]]
        assert np.all(np.diff(rows) > 0), "rows of a group ascending and distinct"
        cnt = min(256, ne - g * 256)
        for ib in range(n):
            want = m["lids"][we[g * 256:g * 256 + cnt], m["offsets"][ib]]
            assert np.array_equal(rows[p["loc"][g, ib, :cnt]], want)
    assert p["max_rows"] % 2 == 0 and p["max_rows"] >= np.diff(p["row_ptr"]).max()
    assert p["max_rows"] <= np.diff(p["row_ptr"]).max() + 1


def test_k1_plan_groups_rows_and_positions():
    """7 x 7 x 6 Q2 elements = 294: two groups, the second partial."""
    m = mrhyde_amd.mesh_structured(3, 2, (7, 7, 6))
    geo = _geo(m["nodes"])
    plans = {o: mrhyde_amd.k1_plan(3, m["lids"], m["offsets"], geo, order=o) for o in ("auto", "natural", "morton")}
    for o, p in plans.items():
        _check_k1_plan(m, p)
        assert p["axis_aligned"] and p["morton"] == (o == "morton")
    assert np.array_equal(plans["auto"]["wg_elems"][:294], np.arange(294))
    assert not np.array_equal(plans["morton"]["wg_elems"][:294], np.arange(294))


def test_k1_plan_takes_the_morton_order_for_a_scattered_numbering():
    """Shuffled element numbering, and a row budget that any group exceeds: the Morton order is tried, and taken because
    its groups are compact."""
    m = mrhyde_amd.mesh_structured(3, 2, (7, 7, 6))
    perm = np.random.default_rng(5).permutation(m["nelem"])
    m["lids"] = np.ascontiguousarray(m["lids"][perm])
    m["nodes"] = np.ascontiguousarray(m["nodes"][perm])
    geo = _geo(m["nodes"])
    natural = mrhyde_amd.k1_plan(3, m["lids"], m["offsets"], geo, order="natural", row_budget=1)
    auto = mrhyde_amd.k1_plan(3, m["lids"], m["offsets"], geo, row_budget=1)
    for p in (natural, auto):
        _check_k1_plan(m, p)
    assert not natural["morton"] and auto["morton"] and auto["max_rows"] < natural["max_rows"]
    forced = mrhyde_amd.k1_plan(3, m["lids"], m["offsets"], geo, order="morton")
    assert all(np.array_equal(auto[k], forced[k]) for k in ("wg_elems", "row_ptr", "rows", "loc"))
    # within the kernel's own budget the numbering is kept
    assert not mrhyde_amd.k1_plan(3, m["lids"], m["offsets"], geo)["morton"]
    # an element that is not axis-aligned
    geo[17, GEO_J + 1] = 1e-3
    assert not mrhyde_amd.k1_plan(3, m["lids"], m["offsets"], geo)["axis_aligned"]


def test_distinct_shapes_match_bit_for_bit():
    m = mrhyde_amd.mesh_structured(3, 1, (4, 4, 4))
    shapes, index = mrhyde_amd.distinct_shapes(3, _geo(m["nodes"]))
    assert len(shapes) == 1 and np.all(index == 0)
    v = m["verts"].copy()
    v[np.flatnonzero(np.all((v > 0.3) & (v < 0.7), axis=1))[0]] += 1e-9
    geo = _geo(v[m["cell2vert"]])
    shapes, index = mrhyde_amd.distinct_shapes(3, geo)
    assert len(shapes) > 1 and index[0] == 0 and index.max() == len(shapes) - 1
    assert np.array_equal(shapes[index], geo[:, :16]), "nothing substituted"
    first = [np.flatnonzero(index == k)[0] for k in range(len(shapes))]
    assert first == sorted(first), "order of first appearance"


def test_distinct_shapes_ignore_the_unused_slots_of_a_2d_record():
    m = mrhyde_amd.mesh_structured(2, 2, (8, 4))
    geo = _geo(m["nodes"])
    rng = np.random.default_rng(2)
    unused = [k for k in range(16) if not (k < 3 or k == GEO_DET or GEO_J <= k < GEO_J + 4)]
    geo[:, unused] = rng.uniform(-1, 1, (len(geo), len(unused)))
    geo[:, GEO_XC:] = rng.uniform(-1, 1, (len(geo), 4))  # (the centroid is not part of the shape either)
    shapes, index = mrhyde_amd.distinct_shapes(2, geo)
    assert len(shapes) == 1 and np.all(index == 0) and np.all(shapes[0, unused] == 0.0)
    geo[5, GEO_J + 3] *= 1 + 2.0 ** -52
    assert len(mrhyde_amd.distinct_shapes(2, geo)[0]) == 2


@pytest.mark.parametrize("dim,order,ncell", [(2, 1, (6, 5)), (3, 1, (4, 4, 3)), (2, 2, (6, 6)), (3, 2, (4, 4, 4))])
def test_slot_pairs_use_every_slot_once(oracle, dim, order, ncell):
    """n = 4, 8 (even), 9, 27 (odd); the ownership masks of the row-owner partition of the mesh."""
    m = mrhyde_amd.mesh_structured(dim, order, ncell)
    rowptr, _ = oracle.build_graph(m["ndof"], m["lids"])
    part = mrhyde_amd.row_partition(dim, m["nodes"], m["lids"], m["ndof"], rowptr)
    n = m["lids"].shape[1]
    emask = []
    for b in range(part["num_blocks"]):
        owned = np.zeros(m["ndof"], bool)
        owned[part["rows"][part["row_ptr"][b]:part["row_ptr"][b + 1]]] = True
        for e in part["elems"][part["elem_ptr"][b]:part["elem_ptr"][b + 1]]:
            emask.append(int(np.sum(owned[m["lids"][e]].astype(np.int64) << np.arange(n))))
    pairs = mrhyde_amd.pair_lid_slots(np.array(emask, np.int64).astype(np.int32), n)
    assert len(pairs) == 2 * ((n + 1) // 2)
    assert sorted(pairs[pairs >= 0].tolist()) == list(range(n))
    assert np.all(pairs[:2 * (n // 2)] >= 0) and (n % 2 == 0 or (pairs[-2] >= 0 and pairs[-1] == -1))


@pytest.mark.parametrize("order", [1, 2])
def test_collocation_derivative_differentiates_the_basis(order):
    dcol, phi, dphi = mrhyde_amd.collocation_derivative(order)
    for i in range(order + 1):
        assert np.abs(dcol @ phi[i] - dphi[i]).max() <= RTOL * np.abs(dphi).max()


# ---- porousMixed

def _porous(ncell):
    m = mrhyde_amd.mesh_multi(len(ncell), ncell, [HVOL, HDIV], [0, 1])
    return m


def test_porous_direct_plan_sides_and_diagonals(oracle):
    m = _porous((4, 4, 4))
    lids, offs, nrows = m["lids"], m["offsets"], m["ndof"]
    rowptr, colind = oracle.build_graph(nrows, lids)
    side, diag = mrhyde_amd.porous_direct_plan(lids, offs, nrows, rowptr, colind)
    assert set(np.unique(side).tolist()) == {0, 1}
    first = np.full(nrows, -1)  # incidence order: elements ascending
    for e in range(m["nelem"]):
        for d in range(lids.shape[1]):
            r = lids[e, offs[d]]
            assert side[e, d] == (0 if first[r] < 0 else 1)
            first[r] = e if first[r] < 0 else first[r]
    for r in range(nrows):
        if m["dof_var"][r] == 1:
            assert colind[diag[r]] == r and rowptr[r] <= diag[r] < rowptr[r + 1]
        else:
            assert diag[r] == -1


def test_porous_direct_plan_refuses_two_shared_dofs(oracle):
    m = _porous((4, 4, 4))
    lids = m["lids"].copy()
    count = np.bincount(lids.ravel(), minlength=m["ndof"])
    is_face = m["dof_var"] == 1
    g = next(r for r in lids[0] if is_face[r] and count[r] == 1)          # a boundary face of element 0 ...
    j = next(j for j, r in enumerate(lids[1]) if is_face[r] and count[r] == 1)
    lids[1, j] = g                                                        # ... becomes a second face shared with element 1
    rowptr, colind = oracle.build_graph(m["ndof"], lids)
    with pytest.raises(mrhyde_amd.MhaError, match="two elements share more than one dof"):
        mrhyde_amd.porous_direct_plan(lids, m["offsets"], m["ndof"], rowptr, colind)


def _slot_map(lids, rowptr, colind):
    E, n = lids.shape
    slot = np.zeros((E, n, n), np.uint8)
    for e in range(E):
        for i in range(n):
            r = lids[e, i]
            slot[e, i] = np.searchsorted(colind[rowptr[r]:rowptr[r + 1]], lids[e])
    return slot


def test_porous_database_plan_replicates_the_scattered_matrix(oracle):
    """(64, 2, 4): long x-lines, so that classes have runs of 2 K rows (K = ceil(128 / row length) + 2)."""
    m = _porous((64, 2, 4))
    lids, nrows = m["lids"], m["ndof"]
    E, n = lids.shape
    rowptr, colind = oracle.build_graph(nrows, lids)
    nnz = len(colind)
    slot = _slot_map(lids, rowptr, colind)
    rng = np.random.default_rng(11)
    fixed = (rng.uniform(size=nrows) < 0.02).astype(np.uint8)
    p = mrhyde_amd.porous_database_plan(m["nodes"], lids, m["offsets"], nrows, rowptr, colind, slot, orient=m["orient"],
                                        fixed=fixed)
    assert p["axis_aligned"] and p["num_classes"] >= 2 and len(p["runs"]) > 0
    # one element matrix of small integers, scattered: sums are exact in any order
    A = rng.integers(-8, 9, (n, n)).astype(np.float64)
    full = np.zeros(nnz)
    np.add.at(full, (rowptr[lids][:, :, None] + slot).ravel(), np.tile(A.ravel(), E))
    covered = np.zeros(nnz, np.int32)
    for s, d, l in p["runs"]:
        covered[d:d + l] += 1
    assert covered.max() == 1 and all(covered[s:s + l].max() == 0 for s, d, l in p["runs"]), "runs read computed entries"
    rowcov = np.add.reduceat(covered, rowptr[:-1])
    replicated = rowcov > 0
    assert np.array_equal(rowcov[replicated], np.diff(rowptr)[replicated]), "whole rows"
    assert np.count_nonzero(~replicated) == p["computed_rows"] and not np.any(replicated & (fixed != 0))
    db = np.where(covered == 1, np.nan, full)
    mrhyde_amd.copy_plan_host_apply(nnz, p["runs"], db)
    assert np.array_equal(db, full)
    want = np.any(~replicated[lids], axis=1)
    assert np.array_equal(p["jacflag"] != 0, want) and np.array_equal(p["elist"], np.flatnonzero(want))
    face = (m["dof_var"] == 1) & ~replicated
    assert np.all(p["diag"][~face] == -1) and np.array_equal(colind[p["diag"][face]], np.flatnonzero(face))


def test_porous_database_plan_refuses_a_perturbed_mesh(oracle):
    m = _porous((64, 2, 4))
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    slot = _slot_map(m["lids"], rowptr, colind)
    v = m["verts"].copy()
    v[len(v) // 2, 0] += 1e-9
    with pytest.raises(mrhyde_amd.MhaError, match="elements of different shapes"):
        mrhyde_amd.porous_database_plan(v[m["cell2vert"]], m["lids"], m["offsets"], m["ndof"], rowptr, colind, slot,
                                        orient=m["orient"])
