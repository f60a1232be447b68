"""The HVOL/HDIV yardstick (tests/highprec_hdiv_ref.py) against its own invariants and against mpmath alone, and the CPU
oracle's porousMixed against the yardstick entry by entry on every case that tests/test_highprec_hdiv_gpu.py runs on the
device.  The second part measures K_oracle per input family (a key of its own for the boundary term), prints it beside the
exact-geometry figure, and holds it to the constant recorded in highprec_hdiv_ref.K_ORACLE from both sides."""
import numpy as np
import pytest

import highprec_hdiv_ref as HD
import highprec_ref as H

LD = np.longdouble


def kl_roots(N, L, sigma, eta):
    import mrhyde_amd
    return mrhyde_amd.kl_expansion(N, L, sigma, eta)[0]


def volume_cases(oracle, family):
    for shape in HD.shapes(family):
        for qdeg in HD.qdegs(family):
            for transient in (False, True):
                c = HD.build_case(oracle, family, shape, qdeg, transient, kl_roots)
                yield c, "%s q%d %s" % (shape[0], qdeg, "stage 1" if transient else "steady")


# ---- the yardstick's own checks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", HD.GEOMETRY + HD.DATABASE)
def test_fluxes_and_constant_fields(oracle, family):
    """(a), (b) on every geometry (the flips applied), (c) on the affine ones."""
    for shape in HD.shapes(family):
        for qdeg in HD.qdegs(family):
            blk = HD.build_case(oracle, family, shape, qdeg, False, kl_roots)["blk"]
            blk.check_fluxes()
            if family in HD.AFFINE:
                ev, ed = blk.check_constant_field()
                print("%-18s %-10s q%d  constant vector: value error %.2e, divergence error %.2e" % (family, shape[0], qdeg, ev, ed))
                # J = sum_v x(v) dN_v is a difference of coordinates of size |x| that differ by the edge: its columns carry
                # the rounding of their terms over the edge.  The vertices are doubles, those of a parallelepiped to
                # 2^-53 |x| only; on the dyadic database meshes they are exact and the rounding left is that of the
                # longdouble tables, 2^-64 |x|.  (1e-15: the longdouble arithmetic of everything else.)
                nodes = blk.nodes
                edge = min(np.abs(nodes[:, a] - nodes[:, b]).max(axis=1).min() for a in range(nodes.shape[1])
                           for b in range(a) if bin(H._vertex_perm(blk.dim)[a] ^ H._vertex_perm(blk.dim)[b]).count("1") == 1)
                tol = 1e-15 + 8 * (2.0 ** -64 if family in HD.DATABASE else H.EPS64) * np.abs(nodes).max() / edge
                assert ev <= tol and ed <= tol, (ev, ed, tol)


def test_flux_check_sees_an_inconsistent_sign(oracle):
    c = HD.build_case(oracle, "unit", HD.SHAPES[0], 2, False)
    m = dict(c["m"], orient=c["m"]["orient"].copy())
    rows = m["lids"][:, m["offsets"][m["varptr"][1]:]]
    e, f = np.argwhere(rows == np.flatnonzero(np.bincount(rows.ravel()) == 2)[0])[0]
    m["orient"][e, m["varptr"][1] + f] *= -1                               # one of the two elements of an interior face
    with pytest.raises(AssertionError, match="interior face"):
        HD.HdivBlock(m, 2).check_fluxes()


def test_side_points_are_where_the_mesh_puts_them(oracle):
    """The order of a side's points is part of the interface (per-point boundary data): the yardstick's side points sit
    where the structured mesh's sides are, in the order of oracle_lib.physical_side_basis, and its normals point outward."""
    for shape in HD.SHAPES:
        c = HD.build_boundary_case(oracle, "stretched warped", shape)
        blk, m = c["blk"], c["m"]
        centre = m["verts"].mean(axis=0)
        for side, be, bs, _ in c["groups"]:
            pt, n, ws, _ = blk.side_tables(be, int(bs[0]))
            got = oracle.physical_side_basis(c["dim"], 1, 2, m["nodes"], be, bs)
            size = np.abs(m["verts"]).max()
            assert np.abs(pt.x - got["ip"]).max() < 1e-13 * size, side
            assert np.abs(ws - got["wts"]).max() < 1e-13 * float(ws.max()), side
            assert np.all((n * (pt.x - centre)).sum(axis=2) > 0), side


def test_one_warped_element_against_mpmath():
    """(d) A, B and the residual of one warped hex and one warped quad at 50 digits, plain loops, to 1e-17 of the scale."""
    for dim in (3, 2):
        v = np.array([[a, b, c] for c in (0, 1) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))], dtype=np.float64)[:2 ** dim, :dim]
        nodes = H.map_vertices(v, "unit") * np.array([1.0, 0.25, 2.0])[:dim]
        n = 1 + 2 * dim
        s = np.array([1, -1, -1, 1, 1, -1][:2 * dim])
        m = dict(nodes=nodes[None], lids=np.arange(n)[None], offsets=np.arange(n), varptr=np.array([0, 1, n]), ndof=n,
                 orient=np.concatenate([[1], s])[None].astype(np.int8))
        rng = np.random.default_rng(7)
        u = rng.uniform(-1, 1, n)
        P = dict(Kinv=[1.3, 0.7, 2.1], mobility=1.9, source=("sinprod", 2.0, [1.3, 0.7, 2.1][:dim]))
        for qdeg in (2, 4):
            blk = HD.HdivBlock(m, qdeg)
            el = HD.element_arrays(blk, P, u)
            A, B, Ru, Rp = HD.element_arrays_mp(nodes, s.tolist(), qdeg, P["Kinv"], P["mobility"], P["source"], u[1:], u[0])
            J, S = el["local_J"][0], el["S_J"][0]
            assert np.all(np.abs(J[1:, 1:] - A) <= 1e-17 * S[1:, 1:]) and S[1:, 1:].min() > 0
            assert np.all(np.abs(J[1:, 0] - B) <= 1e-17 * S[1:, 0]) and np.array_equal(J[0, 1:], J[1:, 0])
            assert J[0, 0] == 0 and S[0, 0] == 0
            assert np.all(np.abs(-el["local_res"][0, 1:] - Ru) <= 1e-17 * el["S_res"][0, 1:])
            assert abs(-el["local_res"][0, 0] - Rp) <= 1e-17 * el["S_res"][0, 0]


# ---- the oracle against the yardstick -------------------------------------------------------------------------------------------
def oracle_funcs(oracle, c):
    """The case's coefficients as the oracle takes them: numbers, sinprod, a deck string, or point arrays (element data
    and the KL field through the existing numpy restatement)."""
    P, dim, fam = c["P"], c["dim"], c["family"]
    f = {"source": P["source"], "total_mobility": P["mobility"]}
    f.update({"Kinv_" + "xyz"[d] * 2: P["Kinv"][d] for d in range(3)})
    if fam == "unit deck source":
        f["source"] = H.sinprod_text(P["source"], dim)
    nq = c["blk"].nq
    if fam == "unit element data":
        kinv = np.repeat(1.0 / P["edata"][:, None], nq, axis=1)
        f.update({"Kinv_" + "xyz"[d] * 2: ("array", kinv) for d in range(dim)})
    if fam == "unit KL":
        from test_porous_heterogeneous_gpu import _kl_field
        x = oracle.physical_basis_var(dim, oracle.HVOL, 0, c["qdeg"], c["m"]["nodes"])["ip"]
        klf = _kl_field(dim, x, P["kl"], P["uq"], P["stoch"], 1)
        f.update({"Kinv_" + "xyz"[d] * 2: ("array", np.ascontiguousarray(P["Kinv"][d] / np.exp(klf[..., d]))) for d in range(dim)})
    return f


def oracle_arrays(oracle, c):
    g = c["g"]
    return oracle.assemble_block(c["m"], oracle.PHYS_POROUS_MIXED, c["qdeg"], c["u"], funcs=oracle_funcs(oracle, c), fixed=c["fixed"],
                                 transient=c["tr"], want_local=True, rowptr=g["rowptr"], colind=g["colind"])


def distances(c, got):
    el, g = c["el"], c["g"]
    return dict(crs_vals=H.distance(got["crs_vals"], g["crs_vals"], g["S_vals"]), res=H.distance(got["res"], g["res"], g["S_res"]),
                local_J=H.distance(got["local_J"], el["local_J"], el["S_J"]),
                local_res=H.distance(got["local_res"], el["local_res"], el["S_res"]))


def exact_geometry_figure(c, got):
    """For the record: the oracle's local_J judged by the scale of the EXACT geometry (|V| in place of Vabs), as the HGRAD
    criterion would: the largest d over the entries with S > 0, and how many entries with S == 0 are not 0.0."""
    ex = HD.element_arrays(c["blk"], c["P"], c["u"], c["tr"], exact_scale=True)
    S, ref, J = ex["S_J"], c["el"]["local_J"], got["local_J"]
    pos = S > 0
    d = float((np.abs(J[pos].astype(LD) - ref[pos]) / (LD(H.EPS64) * S[pos])).max())
    return d, int(np.count_nonzero(J[~pos]))


@pytest.mark.parametrize("family", HD.GEOMETRY + HD.EXTRA + HD.DATABASE)
def test_oracle_against_the_yardstick(oracle, family):
    K = 0.0
    for c, tag in volume_cases(oracle, family):
        assert np.array_equal(c["g"]["colind"], oracle.build_graph(c["m"]["ndof"], c["m"]["lids"])[1])
        got = oracle_arrays(oracle, c)
        d = distances(c, got)
        dx, nz = exact_geometry_figure(c, got)
        print("%-18s %-22s " % (family, tag) + "  ".join("%s %.3g" % kv for kv in d.items()) +
              "   [exact-geometry scale: local_J d %.3g, %d non-zero entries where S == 0]" % (dx, nz))
        pp = c["blk"].pp
        assert np.all(got["local_J"][:, pp, pp] == 0.0)                   # the p-p entry: a structural zero
        assert all(v == v for v in d.values()), d
        K = max(K, max(d.values()))
    _two_sided(HD.MODULE, family, K)


@pytest.mark.parametrize("family", HD.BOUNDARY_FAMILIES)
def test_oracle_boundary_against_the_yardstick(oracle, family):
    K = 0.0
    for shape in HD.SHAPES:
        c = HD.build_boundary_case(oracle, family, shape)
        res, vals = np.zeros(c["m"]["ndof"]), np.zeros(len(c["colind"]))
        for side, be, bs, data in c["groups"]:
            oracle.assemble_block_boundary(c["m"], oracle.PHYS_POROUS_MIXED, 2, c["u"], be, bs, 1, data, rowptr=c["rowptr"],
                                           colind=c["colind"], crs_vals=vals, res=res)
        d = H.distance(res, c["res"], c["S_res"])
        print("%-18s %-10s boundary res %.3g" % (family, shape[0], d))
        assert np.abs(res).max() > 0 and np.all(vals == 0.0)
        K = max(K, d)
    _two_sided(HD.BOUNDARY, family, K)


def _two_sided(module, family, K):
    rec = H.K_ORACLE.get((module, family))
    print("K_oracle[%s, %s] = %.5g (recorded %s, device bound %s)" %
          (module, family, K, rec, H.device_bound(module, family) if rec is not None else None))
    assert rec is not None, "no recorded K_oracle"
    assert K <= rec, "the oracle is farther from the yardstick than recorded"
    assert rec <= 1.5 * K + 1.0, "the recorded K_oracle is stale (more than half above the measurement)"
