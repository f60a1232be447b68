"""porousWeakGalerkin on the device (through the C ABI) against the yardstick of tests/porous_wg_ref.py in 80-bit, entry
by entry: d = |device - yardstick| / (2^-53 S), exact zeros where S == 0, bound max(8 K, 8) per input family with K the
float64 yardstick's own d (porous_wg_ref.K_YARDSTICK, re-measured by tests/test_porous_wg.py; never taken from the
device).  The fused kernel is compared with the yardstick, with the plain kernel + batched_condense (the sum of the two
bounds) and with porousMixedHybridized's fused kernel at Kinv = 1 / perm.  Every comparison prints its largest d beside
its bound."""
import functools
import os

import numpy as np
import pytest

import porous_hybrid_ref as R
import porous_wg_ref as W
from test_porous_wg import DECKS, GOLD, gold_values, printed

pytestmark = pytest.mark.gpu
# every geometry against the three coefficient families, and element data beside a deck-string source (one kernel
# variant carries both) on the two warped meshes
CASES = [(g, k) for g in R.GEOMETRIES for k in R.COEFFICIENTS] + [(g, W.MIXED) for g in W.MIXED_GEOMETRIES]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def dev(a, dtype=None):
    torch = _torch()
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def make_block(mesh, kind="constant", edata=None, orient=None, source=None, perm=None, workset_size=100):
    """A porousWeakGalerkin block of the mesh with the coefficients of a family (or the given source / constant perm)."""
    import mrhyde_amd
    HVOL, HDIV = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV
    blk = mrhyde_amd.Block(mesh["dim"], quadrature=2, physics="porousWeakGalerkin", workset_size=workset_size,
                           variables=[(HVOL, 0), (HDIV, 1), (HDIV, 1)])
    blk.set_mesh(mesh["nodes"], mesh["lids"], mesh["offsets"], mesh["ndof"])
    blk.set_orientation(mesh["orient"] if orient is None else orient)
    if kind == "constant":
        blk.set_function("perm", W.PERM_CONSTANT if perm is None else perm)
        blk.set_function("source", W.SOURCE_CONSTANT if source is None else source)
    elif kind in ("element data", W.MIXED):
        blk.set_element_data(np.asarray(edata, np.float64).reshape(-1, 1))
        blk.set_physics_parameter("use permeability data", 1)
        blk.set_function("source", W.SOURCE_DECK if kind == W.MIXED else W.SOURCE_CONSTANT if source is None else source)
    else:
        blk.set_function("perm", W.PERM_DECK)
        blk.set_function("source", W.SOURCE_DECK)
    return blk


@functools.lru_cache(maxsize=None)
def case(geometry, kind):
    """Mesh, inputs and the yardstick's 80-bit arrays of one case, computed once and shared (read-only)."""
    import mrhyde_amd
    mesh = R.make_mesh(geometry, mrhyde_amd.mesh_porous_weak_galerkin)
    perm, source, edata = W.coefficients(kind, mesh)
    state, lam = W.random_state(mesh, 3)
    NI = 1 + 4 * mesh["dim"]
    lam_el = np.ascontiguousarray(lam[mesh["trace_lids"]])
    arr = W.element_blocks(mesh["nodes"], mesh["orient"][:, 1:], state, lam_el, perm, source, T=W.LD)
    cond = W.condense(arr, NI)
    assert arr["cond_M"].max() <= W.COND_GUARD and arr["perm_ratio"].max() <= W.PERM_RATIO_GUARD
    return dict(mesh=mesh, edata=edata, state=state, lam_el=lam_el, arr=arr, cond=cond, NI=NI, NU=2 * mesh["dim"],
                fam=R.family(geometry, kind), perm=perm, source=source)


def run_plain(blk, c):
    torch = _torch()
    E, n = c["mesh"]["nelem"], c["NI"] + c["NU"]
    res = torch.full((E, n), 7.0, dtype=torch.float64, device="cuda")
    blocks = torch.full((E, n, n), 7.0, dtype=torch.float64, device="cuda")
    blk.pwg_element_blocks(dev(c["state"].ravel()), dev(c["lam_el"]), res, blocks)
    torch.cuda.synchronize()
    return res, blocks


def run_fused(blk, state, lam_el, NI, want=("schur", "gvec", "du"), fill=7.0):
    torch = _torch()
    E, NU = lam_el.shape
    shapes = dict(schur=(E, NU, NU), gvec=(E, NU), du=(E, NI))
    out = {k: torch.full(shapes[k], fill, dtype=torch.float64, device="cuda") for k in shapes}
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    blk.pwg_condensed_element(dev(np.asarray(state).ravel()), dev(lam_el), num_singular=ns, **{k: out[k] for k in want})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, int(ns[0])


def check(tag, got, ref, S, limit):
    d, k = W.distance(got, ref, S)
    print("%-52s largest d = %-9.3g bound %g" % (tag, d, limit))
    assert d <= limit, (tag, d, limit, k)
    return d


@pytest.mark.parametrize("geometry,kind", CASES)
def test_blocks_against_the_yardstick(geometry, kind):
    """pwg_element_blocks entry by entry at a random state; the structurally empty sub-blocks are exactly +0.0."""
    c = case(geometry, kind)
    blk = make_block(c["mesh"], kind, c["edata"])
    res, blocks = run_plain(blk, c)
    res, blocks = res.cpu().numpy(), blocks.cpu().numpy()
    limit = W.bound(c["fam"], "blocks")
    check(geometry + " " + kind + " res", res, c["arr"]["res"], c["arr"]["S_res"], limit)
    check(geometry + " " + kind + " blocks", blocks, c["arr"]["blocks"], c["arr"]["S_blocks"], limit)
    NI, NU = c["NI"], c["NU"]
    o, iu, it, il = slice(0, 1), slice(1, 1 + NU), slice(1 + NU, NI), slice(NI, None)
    for rows, cols in ((o, o), (o, iu), (o, il), (iu, it), (it, o), (it, il), (il, o), (il, iu), (il, il)):
        part = blocks[:, rows, cols]
        assert part.size and np.all(part == 0.0) and not np.any(np.signbit(part)), (rows, cols)
    blk.close()


@pytest.mark.parametrize("geometry,kind", CASES)
def test_fused_against_generic_and_yardstick(geometry, kind):
    """pwg_condensed_element against the yardstick's condensed values and against batched_condense of the plain kernel's
    output (the sum of the two bounds), on the componentwise scale; no singular element."""
    import mrhyde_amd
    c = case(geometry, kind)
    NI, NU = c["NI"], c["NU"]
    blk = make_block(c["mesh"], kind, c["edata"])
    fused, ns = run_fused(blk, c["state"], c["lam_el"], NI)
    assert ns == 0
    res, blocks = run_plain(blk, c)
    schur, gvec, du, nsg = mrhyde_amd.batched_condense(NI, NU, blocks, res)
    assert nsg == 0
    generic = dict(schur=schur.cpu().numpy(), gvec=gvec.cpu().numpy(), du=du.cpu().numpy())
    limit = W.bound(c["fam"], "condensed")
    for k in ("schur", "gvec", "du"):
        ref, S = c["cond"][k], c["cond"]["S_" + k]
        check("%s %s fused %s" % (geometry, kind, k), fused[k], ref, S, limit)
        check("%s %s generic %s" % (geometry, kind, k), generic[k], ref, S, limit)
        check("%s %s fused - generic %s" % (geometry, kind, k), fused[k], generic[k], S, 2 * limit)
    blk.close()


@pytest.mark.parametrize("geometry,kind", [(g, k) for g in R.GEOMETRIES for k in ("constant", "element data")])
def test_schur_is_the_hybridized_mixed_kernels(geometry, kind):
    """perm constant within an element: the fused schur is pmh_condensed_element's at Kinv = 1 / perm, within the sum of
    this module's condensed bound and porousMixedHybridized's own, on the larger of the two yardsticks' scales."""
    import mrhyde_amd
    torch = _torch()
    c = case(geometry, kind)
    NU = c["NU"]
    blk = make_block(c["mesh"], kind, c["edata"])
    fused, _ = run_fused(blk, c["state"], c["lam_el"], c["NI"], want=("schur",))
    blk.close()
    h = R.make_mesh(geometry, mrhyde_amd.mesh_porous_hybrid)
    assert np.array_equal(h["nodes"], c["mesh"]["nodes"])
    hyb = mrhyde_amd.Block(h["dim"], quadrature=2, physics="porousMixedHybridized",
                           variables=[(mrhyde_amd.BASIS_HVOL, 0), (mrhyde_amd.BASIS_HDIV, 1)])
    hyb.set_mesh(h["nodes"], h["lids"], h["offsets"], h["ndof"])
    hyb.set_orientation(h["orient"])
    if kind == "constant":
        kinv = R.const_kinv((1 / W.PERM_CONSTANT,) * 3)
        for d in "xyz":
            hyb.set_function("Kinv_" + d * 2, 1 / W.PERM_CONSTANT)
    else:
        kinv = R.element_kinv(c["edata"])
        hyb.set_element_data(np.asarray(c["edata"], np.float64).reshape(-1, 1))
        hyb.set_physics_parameter("use permeability data", 1)
    schur = torch.full((h["nelem"], NU, NU), 7.0, dtype=torch.float64, device="cuda")
    hyb.pmh_condensed_element(torch.zeros(h["ndof"], dtype=torch.float64, device="cuda"), dev(c["lam_el"]), schur=schur)
    torch.cuda.synchronize()
    hyb.close()
    zero = lambda x: np.zeros(x.shape[:2], x.dtype)
    hc = R.condense(R.element_blocks(h["nodes"], h["orient"][:, 1:], np.zeros((h["nelem"], 1 + NU)), c["lam_el"], kinv, zero, T=R.LD), 1 + NU)
    S = np.maximum(hc["S_schur"], c["cond"]["S_schur"])
    limit = W.bound(c["fam"], "condensed") + R.bound(c["fam"], "condensed")
    check("%s %s schur - pmh schur" % (geometry, kind), fused["schur"], schur.cpu().numpy(), S, limit)


def test_null_outputs_and_determinism():
    """Every combination of NULL outputs: the outputs that are asked for are bit for bit those of the full call; two
    full calls are bit-identical; all three NULL is refused."""
    import mrhyde_amd
    for geometry in ("2d 3x5 warped", "3d 67x1x1"):
        c = case(geometry, "deck strings")
        blk = make_block(c["mesh"], "deck strings")
        full, _ = run_fused(blk, c["state"], c["lam_el"], c["NI"])
        again, _ = run_fused(blk, c["state"], c["lam_el"], c["NI"])
        for k in full:
            assert np.array_equal(full[k], again[k]) and not np.any(full[k] == 7.0), k
        for mask in range(1, 7):
            want = tuple(k for i, k in enumerate(("schur", "gvec", "du")) if mask >> i & 1)
            part, _ = run_fused(blk, c["state"], c["lam_el"], c["NI"], want=want)
            for k in full:
                assert np.array_equal(part[k], full[k]) if k in want else np.all(part[k] == 7.0), (want, k)
        with pytest.raises(mrhyde_amd.MhaError, match="no output requested"):
            run_fused(blk, c["state"], c["lam_el"], c["NI"], want=())
        blk.close()


@pytest.mark.parametrize("geometry", ["2d 3x5 warped", "3d 3x2x2 warped"])
def test_face_signs_do_not_reach_the_condensed_blocks(geometry):
    """Flipping every sign in `orient` changes schur and gvec by nothing beyond the tolerance and flips the u and t parts
    of du."""
    c = case(geometry, "constant")
    NI = c["NI"]
    state = c["state"].copy()
    flipped = state.copy()
    flipped[:, 1:] *= -1  # the same fields in the flipped basis
    a_blk = make_block(c["mesh"], "constant")
    o = c["mesh"]["orient"].copy()
    o[:, 1:] *= -1
    b_blk = make_block(c["mesh"], "constant", orient=o)
    a, _ = run_fused(a_blk, state, c["lam_el"], NI)
    b, _ = run_fused(b_blk, flipped, c["lam_el"], NI)
    limit = W.bound(c["fam"], "condensed")
    flip = np.array([1.0] + [-1.0] * (NI - 1))
    for k, gb in (("schur", b["schur"]), ("gvec", b["gvec"]), ("du", b["du"] * flip)):
        check("%s flipped signs %s" % (geometry, k), gb, c["cond"][k], c["cond"]["S_" + k], limit)
        check("%s flipped - plain signs %s" % (geometry, k), gb, a[k], c["cond"]["S_" + k], 2 * limit)
    a_blk.close()
    b_blk.close()


def test_singular_element_is_counted():
    """One element with perm = -1 (element data) among 70: counted once, every output finite, the other 69 elements'
    outputs bit-identical to a run without it."""
    import mrhyde_amd
    mesh = mrhyde_amd.mesh_porous_weak_galerkin((10, 7))
    state, lam = W.random_state(mesh, 8)
    lam_el = np.ascontiguousarray(lam[mesh["trace_lids"]])
    edata = np.random.default_rng(2).uniform(0.5, 2.0, 70)
    bad = edata.copy()
    bad[37] = -1.0
    good_blk, bad_blk = make_block(mesh, "element data", edata), make_block(mesh, "element data", bad)
    g, ng = run_fused(good_blk, state, lam_el, 9)
    b, nb = run_fused(bad_blk, state, lam_el, 9)
    assert ng == 0 and nb == 1
    keep = np.arange(70) != 37
    for k in g:
        assert np.all(np.isfinite(b[k])), k
        assert np.array_equal(b[k][keep], g[k][keep]), k
    good_blk.close()
    bad_blk.close()


def two_call_solve(mesh, blk, lam0):
    """The linear solve on one block: step at (0, lam0), ScatterPlan.apply with the boundary rows fixed, trace solve on the
    host, step again, u += du.  -> (state [E][NI], lam [ntrace], |second gvec| summed per free trace row, max)."""
    import mrhyde_amd
    torch = _torch()
    E, dim = mesh["nelem"], mesh["dim"]
    NI, NU, nt = 1 + 4 * dim, 2 * dim, mesh["ntrace"]
    tl, fixed = mesh["trace_lids"], (mesh["trace_side"] != 0)
    u = torch.zeros(mesh["ndof"], dtype=torch.float64, device="cuda")
    lam = np.array(lam0, np.float64)
    schur = torch.zeros((E, NU, NU), dtype=torch.float64, device="cuda")
    gvec = torch.zeros((E, NU), dtype=torch.float64, device="cuda")
    du = torch.zeros((E, NI), dtype=torch.float64, device="cuda")
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan = mrhyde_amd.ScatterPlan(tl, nt, fixed=fixed.astype(np.uint8))
    rowptr, colind = plan.graph()
    vals = torch.zeros(plan.nnz, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(nt, dtype=torch.float64, device="cuda")
    blk.pwg_condensed_element(u, dev(lam[tl]), schur=schur, gvec=gvec, num_singular=ns)
    plan.apply(schur, gvec, rhs, vals, overwrite=True)
    torch.cuda.synchronize()
    M = np.zeros((nt, nt))
    M[np.repeat(np.arange(nt), np.diff(rowptr)), colind] = vals.cpu().numpy()
    b = rhs.cpu().numpy()
    assert np.all(M[fixed] == 0.0) and np.all(b[fixed] == 0.0)
    M[fixed, fixed] = 1.0
    lam = lam + np.linalg.solve(M, b)
    blk.pwg_condensed_element(u, dev(lam[tl]), gvec=gvec, du=du, num_singular=ns)
    plan.apply(None, gvec, rhs, None, overwrite=True)
    u += du.reshape(-1)
    torch.cuda.synchronize()
    assert int(ns[0]) == 0
    plan.close()
    return u.cpu().numpy().reshape(E, NI), lam, float(np.abs(rhs.cpu().numpy()[~fixed]).max())


@pytest.mark.parametrize("deck,ncell,want", DECKS)
def test_the_recorded_decks_through_the_device(deck, ncell, want):
    """The three decks, end to end (100 and 1000 elements: several workgroups, a partial last wavefront): the four error
    norms, computed by the yardstick's loops from the device's state and lambda, match the printed digits."""
    import mrhyde_amd
    mesh = mrhyde_amd.mesh_porous_weak_galerkin(ncell)
    src = "8*(pi*pi)*sin(2*pi*x)*sin(2*pi*y)" if len(ncell) == 2 else "12*(pi*pi)*sin(2*pi*x)*sin(2*pi*y)*sin(2*pi*z)"
    blk = make_block(mesh, "constant", source=src, perm=1.0)
    if "PermData" in deck:
        pts = np.loadtxt(os.path.join(GOLD, deck + ".perm_xy.dat"))
        vals = np.loadtxt(os.path.join(GOLD, deck + ".perm.dat"))
        blk.import_mesh_data(pts, vals.reshape(-1, 1))
        blk.set_physics_parameter("use permeability data", 1)
    state, lam, g2 = two_call_solve(mesh, blk, np.zeros(mesh["ntrace"]))
    got = [printed(v) for v in W.four_errors(mesh, state, lam)]
    print(deck, got, gold_values(deck), "second gvec on free rows", g2)
    assert got == gold_values(deck) == want
    assert g2 < 1e-12
    blk.close()


def test_nonzero_dirichlet_data_lifts_itself():
    """pbndry = x + 2y on the boundary faces, source 0, perm 1: pint = x + 2y (its mean), u = (1, 2) and t = (-1, -2) lie
    in the spaces, so pbndry is the value at the face centroid on every face.  Tolerance as the porousMixedHybridized
    test's: the trace system of the 8 x 8 mesh has a condition number below 1e3 and the solution is of size 3."""
    import mrhyde_amd
    mesh = mrhyde_amd.mesh_porous_weak_galerkin((8, 8))
    cen = R.face_centroids(mesh)
    exact = np.zeros(mesh["ntrace"])
    exact[mesh["trace_lids"]] = cen[:, :, 0] + 2 * cen[:, :, 1]
    lam0 = np.where(mesh["trace_side"] != 0, exact, 0.0)
    blk = make_block(mesh, "constant", source=0.0, perm=1.0)
    state, lam, g2 = two_call_solve(mesh, blk, lam0)
    assert np.abs(lam - exact).max() < 1e-11 and g2 < 1e-11
    grad = lambda s: (lambda x: (x[:, :, 0] + 2 * x[:, :, 1], np.stack([s * np.ones(x.shape[:2]), 2 * s * np.ones(x.shape[:2])], axis=2)))
    ep, ef, eu, et = W.four_errors(mesh, state, lam, true_u=grad(1.0), true_t=grad(-1.0))
    assert eu < 1e-11 and et < 1e-11
    assert np.abs(state[:, 0] - (mesh["nodes"][:, :, 0] + 2 * mesh["nodes"][:, :, 1]).mean(axis=1)).max() < 1e-11
    blk.close()


@pytest.mark.parametrize("geometry", ["2d 3x5 warped", "3d 3x2x2 warped"])
@pytest.mark.parametrize("kind", R.COEFFICIENTS + (W.MIXED,))
def test_volume_terms_against_the_yardstick(geometry, kind):
    """volumeResidual on the point function: assemble_jacres (AUTO and the point engine; res and CRS values),
    apply_jacobian forward and transposed, the multi-vector product, jacobian_diagonal, get_mass and the workset views
    against the yardstick's volume block assembled on the host.  Tolerances: those of the porousMixedHybridized test,
    1e-13 (1e-12 for the products) of the largest entry."""
    import mrhyde_amd
    import scipy.sparse as sp
    torch = _torch()
    c = case(geometry, kind)
    mesh, NI, NU = c["mesh"], c["NI"], c["NU"]
    E, nd = mesh["nelem"], mesh["ndof"]
    Ab, data = W.volume_block(mesh["nodes"], mesh["orient"][:, 1:], c["perm"], c["source"])
    rows = np.repeat(mesh["lids"][:, :, None], NI, axis=2)
    cols = np.repeat(mesh["lids"][:, None, :], NI, axis=1)
    A = sp.csr_matrix((Ab.ravel(), (rows.ravel(), cols.ravel())), shape=(nd, nd))
    u_h = np.random.default_rng(1).uniform(-1, 1, nd)
    val = A @ u_h
    np.add.at(val, mesh["lids"].ravel(), data.ravel())
    res_ref = -val  # the global residual receives -res.val(), the Jacobian +d res / d u (include/mrhyde_amd.h)
    scale, rscale = np.abs(Ab).max(), max(1.0, np.abs(res_ref).max())
    blk = make_block(mesh, kind, c["edata"], workset_size=E)
    blk.set_graph()
    rowptr, colind = blk.get_graph()
    u = dev(u_h)
    for path in (mrhyde_amd.PATH_AUTO, mrhyde_amd.PATH_POINT_ENGINE):
        res = torch.zeros(nd, dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
        blk.assemble_jacres(u, res, vals, path=path)
        torch.cuda.synchronize()
        G = sp.csr_matrix((vals.cpu().numpy(), colind, rowptr), shape=(nd, nd))
        assert np.abs(res.cpu().numpy() - res_ref).max() < 1e-13 * rscale, path
        assert abs(G - A).max() < 1e-13 * scale, path
    x_h = np.random.default_rng(2).uniform(-1, 1, (2, nd))
    x, y, yt, dg = dev(x_h[0]), torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
    blk.apply_jacobian(u, x, y, overwrite=True)
    blk.apply_jacobian(u, x, yt, transpose=True, overwrite=True)
    blk.jacobian_diagonal(u, dg, overwrite=True)
    X, Y = dev(x_h), torch.zeros((2, nd), dtype=torch.float64, device="cuda")
    blk.apply_jacobian_multi(u, X, Y, overwrite=True)
    mass = torch.zeros((E, NI, NI), dtype=torch.float64, device="cuda")
    blk.get_mass(mass)
    torch.cuda.synchronize()
    assert np.abs(y.cpu().numpy() - A @ x_h[0]).max() < 1e-12 * scale
    assert np.abs(yt.cpu().numpy() - A.T @ x_h[0]).max() < 1e-12 * scale
    assert np.abs(Y.cpu().numpy() - (A @ x_h.T).T).max() < 1e-12 * scale
    assert np.abs(dg.cpu().numpy() - A.diagonal()).max() < 1e-13 * scale
    # the mass matrix: (q, q), (v_f, v_g) for u and for t, nothing between the variables
    mref = np.zeros((E, NI, NI))
    mref[:, 1:1 + NU, 1:1 + NU] = Ab[:, 1:1 + NU, 1:1 + NU]
    mref[:, 1 + NU:, 1 + NU:] = Ab[:, 1 + NU:, 1 + NU:]
    det = R.det_cof(R.geometry(np.asarray(mesh["nodes"], np.float64), R.tensor_rule(mesh["dim"], 2, np.float64)[0])[1])[0]
    mref[:, 0, 0] = (det * R.tensor_rule(mesh["dim"], 2, np.float64)[1][None, :]).sum(1)
    assert np.abs(mass.cpu().numpy() - mref).max() < 1e-13 * np.abs(mref).max()
    # the workset views against the CPU oracle's physical HDIV basis at the block's own points, value by value: pint is
    # the element's state; u[x].., div(u), t[x].., div(t) are the dofs of that variable times its basis
    import oracle_lib
    blk.workset_update(0)
    blk.workset_compute_solution(u)
    st = u_h[mesh["lids"]]
    pint = blk.workset_view_numpy("pint")
    assert pint.shape[0] == E and np.abs(pint - st[:, :1]).max() < 1e-14
    for name, sl in (("u", slice(1, 1 + NU)), ("t", slice(1 + NU, NI))):
        pb = oracle_lib.physical_basis_var(mesh["dim"], oracle_lib.HDIV, 1, 2, mesh["nodes"], np.ascontiguousarray(mesh["orient"][:, sl]))
        want = np.einsum("ef,efq->eq", st[:, sl], pb["div"])
        got = blk.workset_view_numpy("div(%s)" % name)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-12 * np.abs(want).max(), name
        for d, comp in enumerate(("[x]", "[y]", "[z]")[:mesh["dim"]]):
            want = np.einsum("ef,efq->eq", st[:, sl], pb["basis"][:, :, :, d])
            got = blk.workset_view_numpy(name + comp)
            assert got.shape == want.shape and np.abs(got - want).max() < 1e-12 * np.abs(want).max(), name + comp
    blk.close()


def test_refusals_through_the_abi():
    """A conforming LID map, a boundary group of the module, compute_flux, the deterministic flag, the row-owner path, a
    field-reading deck string, a transient context and a misaligned output are refused with MHA_ERR_INVALID, each naming
    its cause; outputs stay untouched."""
    import mrhyde_amd
    torch = _torch()
    HVOL, HDIV = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV
    INVALID = mrhyde_amd.api.ERR_INVALID
    conf = mrhyde_amd.mesh_multi(2, (3, 2), [HVOL, HDIV, HDIV], [0, 1, 1])
    blk = mrhyde_amd.Block(2, quadrature=2, physics="porousWeakGalerkin", variables=[(HVOL, 0), (HDIV, 1), (HDIV, 1)])
    blk.set_mesh(conf["nodes"], conf["lids"], conf["offsets"], conf["ndof"])
    blk.set_orientation(conf["orient"])
    E = conf["nelem"]
    u = torch.zeros(conf["ndof"], dtype=torch.float64, device="cuda")
    lam = torch.zeros((E, 4), dtype=torch.float64, device="cuda")
    S = torch.full((E, 4, 4), 7.0, dtype=torch.float64, device="cuda")
    B = torch.full((E, 13, 13), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="porousWeakGalerkin: row .* must be DG") as ei:
        blk.pwg_condensed_element(u, lam, schur=S)
    assert ei.value.code == INVALID
    with pytest.raises(mrhyde_amd.MhaError, match="must be DG"):
        blk.pwg_element_blocks(u, lam, blocks=B)
    torch.cuda.synchronize()
    assert bool((S == 7.0).all()) and bool((B == 7.0).all())
    blk.close()
    # a variable list that is not the module's is refused by the module; an order above lowest already by the block
    # ("HDIV is available at order 1"), before the module is asked
    for bad, words in (([(HVOL, 0), (HDIV, 1)], "porousWeakGalerkin needs"), ([(HVOL, 0), (HDIV, 2), (HDIV, 1)], "order 1")):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            mrhyde_amd.Block(2, quadrature=2, physics="porousWeakGalerkin", variables=bad)
        assert ei.value.code == INVALID and words in str(ei.value), str(ei.value)

    mesh = mrhyde_amd.mesh_porous_weak_galerkin((3, 2))
    blk = make_block(mesh, "constant")
    with pytest.raises(mrhyde_amd.MhaError, match="HDIV_AC") as ei:
        blk.set_physics_parameter("useAC", 1)
    assert ei.value.code == INVALID
    with pytest.raises(mrhyde_amd.MhaError, match="no KL expansion"):
        blk.set_physics_parameter("use KL expansion", 1)
    be, bs = np.array([0, 1, 2], np.int32), np.zeros(3, np.int32)
    for bc in (mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE, mrhyde_amd.BC_NEUMANN):
        with pytest.raises(mrhyde_amd.MhaError, match="boundary groups of the module") as ei:
            blk.add_boundary_group("bottom", bc, be, bs)
        assert ei.value.code == INVALID
    assert blk.num_boundary_groups() == 0
    gid = blk.add_flux_group("bottom", "t", be, bs)
    u = torch.zeros(mesh["ndof"], dtype=torch.float64, device="cuda")
    flux = torch.full((3, 2), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="computeFlux") as ei:
        blk.compute_flux(gid, u, flux)
    assert ei.value.code == INVALID
    blk.set_graph()
    _, colind = blk.get_graph()
    res = torch.full((mesh["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((len(colind),), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="MHA_ASSEMBLE_DETERMINISTIC") as ei:
        blk.assemble_jacres(u, res, vals, deterministic=True)
    assert ei.value.code == INVALID
    with pytest.raises(mrhyde_amd.MhaError, match="not available for this physics module") as ei:
        blk.assemble_jacres(u, res, vals, path=mrhyde_amd.PATH_ROW_OWNER)
    assert ei.value.code == INVALID
    lam = torch.zeros((mesh["nelem"], 4), dtype=torch.float64, device="cuda")
    S = torch.full((mesh["nelem"], 4, 4), 7.0, dtype=torch.float64, device="cuda")
    # an output that is not 16-byte aligned
    pool = torch.full((mesh["nelem"] * 4 + 1,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="16-byte aligned") as ei:
        blk.pwg_condensed_element(u, lam, gvec=pool[1:])
    assert ei.value.code == INVALID
    blk.set_function("perm", "1+pint*pint")
    with pytest.raises(mrhyde_amd.MhaError, match="reads solution fields"):
        blk.pwg_condensed_element(u, lam, schur=S)
    with pytest.raises(mrhyde_amd.MhaError, match="reads solution fields"):
        blk.assemble_jacres(u, res, vals)
    blk.set_function("perm", 1.0)
    blk.set_time_integration(True, 1, 1, 0, 0.1, [1.0], [1.0], [1.0, -1.0])
    with pytest.raises(mrhyde_amd.MhaError, match="steady residual"):
        blk.pwg_condensed_element(u, lam, schur=S)
    torch.cuda.synchronize()
    for t in (flux, res, vals, S, pool):
        assert bool((t == 7.0).all())
    blk.close()
    # a block of another module has no such step
    h = mrhyde_amd.mesh_porous_hybrid((3, 2))
    other = mrhyde_amd.Block(2, quadrature=2, physics="porousMixedHybridized", variables=[(HVOL, 0), (HDIV, 1)])
    other.set_mesh(h["nodes"], h["lids"], h["offsets"], h["ndof"])
    with pytest.raises(mrhyde_amd.MhaError, match="not porousWeakGalerkin"):
        other.pwg_condensed_element(u, lam, schur=S)
    other.close()
