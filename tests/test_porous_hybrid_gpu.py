"""porousMixedHybridized on the device (through the C ABI) against the yardstick of tests/porous_hybrid_ref.py in 80-bit,
entry by entry: d = |device - yardstick| / (2^-53 S), exact zeros where S == 0, bound max(8 K, 8) per input family with
K the float64 yardstick's own d (porous_hybrid_ref.K_YARDSTICK, re-measured by tests/test_porous_hybrid.py; never taken
from the device).  The fused kernel is compared with the yardstick and with the plain kernel + batched_condense (the
sum of the two bounds).  Every comparison prints its largest d beside its bound."""
import functools

import numpy as np
import pytest

import porous_hybrid_ref as R
from test_porous_hybrid import gold_values, printed

pytestmark = pytest.mark.gpu
CASES = [(g, k) for g in R.GEOMETRIES for k in R.COEFFICIENTS]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def dev(a, dtype=None):
    torch = _torch()
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def make_block(mesh, kind="constant", edata=None, orient=None, source=None, kinv=None):
    """A porousMixedHybridized block of the mesh with the coefficients of a family (or the given source / constant Kinv)."""
    import mrhyde_amd
    dim = mesh["dim"]
    blk = mrhyde_amd.Block(dim, quadrature=2, physics="porousMixedHybridized",
                           variables=[(mrhyde_amd.BASIS_HVOL, 0), (mrhyde_amd.BASIS_HDIV, 1)])
    blk.set_mesh(mesh["nodes"], mesh["lids"], mesh["offsets"], mesh["ndof"])
    blk.set_orientation(mesh["orient"] if orient is None else orient)
    if kind == "constant":
        for d, v in zip("xyz", R.KINV_CONSTANT if kinv is None else kinv):
            blk.set_function("Kinv_" + d * 2, v)
        blk.set_function("source", R.SOURCE_CONSTANT if source is None else source)
    elif kind == "element data":
        blk.set_element_data(np.asarray(edata, np.float64).reshape(-1, 1))
        blk.set_physics_parameter("use permeability data", 1)
        blk.set_function("source", R.SOURCE_CONSTANT)
    else:
        blk.set_function("Kinv_xx", "1.0+x*x+y")
        blk.set_function("source", "sin(2*pi*x)*y")
    return blk


@functools.lru_cache(maxsize=None)
def case(geometry, kind):
    """Mesh, inputs and the yardstick's 80-bit arrays of one case, computed once and shared (read-only)."""
    import mrhyde_amd
    mesh = R.make_mesh(geometry, mrhyde_amd.mesh_porous_hybrid)
    kinv, source, edata = R.coefficients(kind, mesh)
    state, lam = R.random_state(mesh, 3)
    NI = 1 + 2 * mesh["dim"]
    lam_el = np.ascontiguousarray(lam[mesh["trace_lids"]])
    arr = R.element_blocks(mesh["nodes"], mesh["orient"][:, 1:], state, lam_el, kinv, source, T=R.LD)
    cond = R.condense(arr, NI)
    assert cond["cond"].max() <= R.COND_GUARD
    return dict(mesh=mesh, edata=edata, state=state, lam_el=lam_el, arr=arr, cond=cond, NI=NI, fam=R.family(geometry, kind))


def run_plain(blk, c):
    torch = _torch()
    E, NI = c["mesh"]["nelem"], c["NI"]
    n = 2 * NI - 1
    res = torch.full((E, n), 7.0, dtype=torch.float64, device="cuda")
    blocks = torch.full((E, n, n), 7.0, dtype=torch.float64, device="cuda")
    blk.pmh_element_blocks(dev(c["state"].ravel()), dev(c["lam_el"]), res, blocks)
    torch.cuda.synchronize()
    return res, blocks


def run_fused(blk, state, lam_el, NI, want=("schur", "gvec", "du"), fill=7.0):
    torch = _torch()
    E, NU = lam_el.shape[0], NI - 1
    shapes = dict(schur=(E, NU, NU), gvec=(E, NU), du=(E, NI))
    out = {k: torch.full(shapes[k], fill, dtype=torch.float64, device="cuda") for k in shapes}
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    blk.pmh_condensed_element(dev(np.asarray(state).ravel()), dev(lam_el), num_singular=ns, **{k: out[k] for k in want})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, int(ns[0])


def check(tag, got, ref, S, limit):
    d, k = R.distance(got, ref, S)
    print("%-44s largest d = %-9.3g bound %g" % (tag, d, limit))
    assert d <= limit, (tag, d, limit, k)
    return d


@pytest.mark.parametrize("geometry,kind", CASES)
def test_blocks_against_the_yardstick(geometry, kind):
    """pmh_element_blocks entry by entry at a random state; the p-lambda, lambda-lambda and p-p entries are exactly 0.0."""
    c = case(geometry, kind)
    blk = make_block(c["mesh"], kind, c["edata"])
    res, blocks = run_plain(blk, c)
    res, blocks = res.cpu().numpy(), blocks.cpu().numpy()
    limit = R.bound(c["fam"], "blocks")
    check(geometry + " " + kind + " res", res, c["arr"]["res"], c["arr"]["S_res"], limit)
    check(geometry + " " + kind + " blocks", blocks, c["arr"]["blocks"], c["arr"]["S_blocks"], limit)
    NI = c["NI"]
    for part in (blocks[:, 0, 0], blocks[:, 0, NI:], blocks[:, NI:, 0], blocks[:, NI:, NI:]):
        assert np.all(part == 0.0) and not np.any(np.signbit(part))
    blk.close()


@pytest.mark.parametrize("geometry,kind", CASES)
def test_fused_against_generic_and_yardstick(geometry, kind):
    """pmh_condensed_element against the yardstick's condensed values and against batched_condense of the plain kernel's
    output (the sum of the two bounds), on the componentwise scale; no singular element."""
    import mrhyde_amd
    c = case(geometry, kind)
    NI, NU = c["NI"], c["NI"] - 1
    blk = make_block(c["mesh"], kind, c["edata"])
    fused, ns = run_fused(blk, c["state"], c["lam_el"], NI)
    assert ns == 0
    res, blocks = run_plain(blk, c)
    schur, gvec, du, nsg = mrhyde_amd.batched_condense(NI, NU, blocks, res)
    assert nsg == 0
    generic = dict(schur=schur.cpu().numpy(), gvec=gvec.cpu().numpy(), du=du.cpu().numpy())
    limit = R.bound(c["fam"], "condensed")
    for k in ("schur", "gvec", "du"):
        ref, S = c["cond"][k], c["cond"]["S_" + k]
        check("%s %s fused %s" % (geometry, kind, k), fused[k], ref, S, limit)
        check("%s %s generic %s" % (geometry, kind, k), generic[k], ref, S, limit)
        check("%s %s fused - generic %s" % (geometry, kind, k), fused[k], generic[k], S, 2 * limit)
    blk.close()


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
    """Flipping every sign in `orient` changes schur and gvec by nothing beyond the tolerance and flips the flux part of du."""
    c = case(geometry, "constant")
    NI = c["NI"]
    state = c["state"].copy()
    flipped = state.copy()
    flipped[:, 1:] *= -1  # the same flux field in the flipped basis
    a_blk = make_block(c["mesh"], "constant")
    o = c["mesh"]["orient"].copy()
    o[:, 1:] *= -1
    b_blk = make_block(c["mesh"], "constant", orient=o)
    a, _ = run_fused(a_blk, state, c["lam_el"], NI)
    b, _ = run_fused(b_blk, flipped, c["lam_el"], NI)
    limit = R.bound(c["fam"], "condensed")
    flip = np.array([1.0] + [-1.0] * (NI - 1))
    for k, gb in (("schur", b["schur"]), ("gvec", b["gvec"]), ("du", b["du"] * flip)):
        check("%s flipped signs %s" % (geometry, k), gb, c["cond"][k], c["cond"]["S_" + k], limit)
        check("%s flipped - plain signs %s" % (geometry, k), gb, a[k], c["cond"]["S_" + k], 2 * limit)
    a_blk.close()
    b_blk.close()


def test_singular_element_is_counted():
    """One element with Kinv = -1 (element data) among 70: counted once, every output finite, the other 69 elements'
    outputs bit-identical to a run without it."""
    import mrhyde_amd
    mesh = mrhyde_amd.mesh_porous_hybrid((10, 7))
    state, lam = R.random_state(mesh, 8)
    lam_el = np.ascontiguousarray(lam[mesh["trace_lids"]])
    edata = np.random.default_rng(2).uniform(0.5, 2.0, 70)
    bad = edata.copy()
    bad[37] = -1.0
    good_blk, bad_blk = make_block(mesh, "element data", edata), make_block(mesh, "element data", bad)
    g, ng = run_fused(good_blk, state, lam_el, 5)
    b, nb = run_fused(bad_blk, state, lam_el, 5)
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
    NI, NU, nt = 1 + 2 * dim, 2 * dim, mesh["ntrace"]
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
    blk.pmh_condensed_element(u, dev(lam[tl]), schur=schur, gvec=gvec, num_singular=ns)
    plan.apply(schur, gvec, rhs, vals, overwrite=True)
    torch.cuda.synchronize()
    M = np.zeros((nt, nt))
    M[np.repeat(np.arange(nt), np.diff(rowptr)), colind] = vals.cpu().numpy()
    b = rhs.cpu().numpy()
    assert np.all(M[fixed] == 0.0) and np.all(b[fixed] == 0.0)
    M[fixed, fixed] = 1.0
    lam = lam + np.linalg.solve(M, b)
    blk.pmh_condensed_element(u, dev(lam[tl]), gvec=gvec, du=du, num_singular=ns)
    plan.apply(None, gvec, rhs, None, overwrite=True)
    u += du.reshape(-1)
    torch.cuda.synchronize()
    assert int(ns[0]) == 0
    plan.close()
    return u.cpu().numpy().reshape(E, NI), lam, float(np.abs(rhs.cpu().numpy()[~fixed]).max())


@pytest.mark.parametrize("deck,ncell", [("porous_Mixed_hybrid", (8, 8)), ("porous_Mixed_3D_hybrid", (8, 8, 8))])
def test_the_recorded_decks_through_the_device(deck, ncell):
    """Both decks, end to end: the three error norms, computed by the yardstick's loops from the device's u and lambda,
    match the printed digits."""
    import mrhyde_amd
    mesh = mrhyde_amd.mesh_porous_hybrid(ncell)
    src = "8*(pi*pi)*sin(2*pi*x)*sin(2*pi*y)" if len(ncell) == 2 else "12*(pi*pi)*sin(2*pi*x)*sin(2*pi*y)*sin(2*pi*z)"
    blk = make_block(mesh, "constant", source=src, kinv=(1.0, 1.0, 1.0))
    state, lam, g2 = two_call_solve(mesh, blk, np.zeros(mesh["ntrace"]))
    got = [printed(v) for v in R.errors(mesh, state, lam)]
    print(deck, got, gold_values(deck), "second gvec on free rows", g2)
    assert got == gold_values(deck)
    # the right-hand side of the first step is of size |source| h^dim ~ 1: round-off of the second one
    assert g2 < 1e-12
    blk.close()


def test_nonzero_dirichlet_data_lifts_itself():
    """lambda = x + 2y on the boundary faces, source 0, Kinv 1: p = x + 2y solves the problem and u = (-1, -2) lies in
    RT0, so lambda is the L2-face projection of x + 2y on every face (its value at the face centroid) and u = (-1, -2)
    at every point.  Tolerance: the trace system of the 8 x 8 mesh has a condition number below 1e3 and the solution is of
    size 3, so round-off is below 1e3 x 3 x 2^-53 = 4e-13; 1e-11 leaves a factor of 25."""
    import mrhyde_amd
    mesh = mrhyde_amd.mesh_porous_hybrid((8, 8))
    cen = R.face_centroids(mesh)
    exact = np.zeros(mesh["ntrace"])
    exact[mesh["trace_lids"]] = cen[:, :, 0] + 2 * cen[:, :, 1]
    lam0 = np.where(mesh["trace_side"] != 0, exact, 0.0)
    blk = make_block(mesh, "constant", source=0.0, kinv=(1.0, 1.0, 1.0))
    state, lam, g2 = two_call_solve(mesh, blk, lam0)
    assert np.abs(lam - exact).max() < 1e-11 and g2 < 1e-11
    true = lambda x: (x[:, :, 0] + 2 * x[:, :, 1], np.stack([-np.ones(x.shape[:2]), -2 * np.ones(x.shape[:2])], axis=2))
    _, eu, _ = R.errors(mesh, state, lam, true=true)
    assert eu < 1e-11
    assert np.abs(state[:, 0] - (mesh["nodes"][:, :, 0] + 2 * mesh["nodes"][:, :, 1]).mean(axis=1)).max() < 1e-11
    blk.close()


def test_volume_terms_run_on_the_porous_point_function():
    """volumeResidual is porousMixed's with total_mobility == 1: assemble_jacres (AUTO and the point engine), the
    matrix-free product, the diagonal and get_mass on the block agree with a porousMixed block of the same DG mesh."""
    import mrhyde_amd
    torch = _torch()
    mesh = R.make_mesh("3d 3x2x2 warped", mrhyde_amd.mesh_porous_hybrid)
    hyb = make_block(mesh, "constant")
    ref = mrhyde_amd.Block(3, quadrature=2, physics="porousMixed", variables=[(mrhyde_amd.BASIS_HVOL, 0), (mrhyde_amd.BASIS_HDIV, 1)])
    ref.set_mesh(mesh["nodes"], mesh["lids"], mesh["offsets"], mesh["ndof"])
    ref.set_orientation(mesh["orient"])
    for d, v in zip("xyz", R.KINV_CONSTANT):
        ref.set_function("Kinv_" + d * 2, v)
    ref.set_function("source", R.SOURCE_CONSTANT)
    u = dev(np.random.default_rng(1).uniform(-1, 1, mesh["ndof"]))
    out = {}
    for name, blk in (("hyb", hyb), ("ref", ref)):
        blk.set_graph()
        rowptr, colind = blk.get_graph()
        res = torch.zeros(mesh["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
        blk.assemble_jacres(u, res, vals, path=mrhyde_amd.PATH_POINT_ENGINE)
        mass = torch.zeros((mesh["nelem"], 7, 7), dtype=torch.float64, device="cuda")
        blk.get_mass(mass)
        torch.cuda.synchronize()
        out[name] = (res.cpu().numpy(), vals.cpu().numpy(), mass.cpu().numpy())
    for a, b in zip(out["hyb"], out["ref"]):
        assert np.array_equal(a, b) and np.abs(a).max() > 0
    res, vals = torch.zeros_like(u), torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    hyb.assemble_jacres(u, res, vals)  # AUTO: dense element matrices + row gather
    y, dg = torch.zeros_like(u), torch.zeros_like(u)
    hyb.apply_jacobian(u, u, y, overwrite=True)
    hyb.jacobian_diagonal(u, dg, overwrite=True)
    torch.cuda.synchronize()
    scale = np.abs(out["ref"][1]).max()
    assert np.abs(res.cpu().numpy() - out["ref"][0]).max() < 1e-13 * max(1.0, np.abs(out["ref"][0]).max())
    assert np.abs(vals.cpu().numpy() - out["ref"][1]).max() < 1e-13 * scale
    import scipy.sparse as sp
    A = sp.csr_matrix((out["ref"][1], colind, rowptr), shape=(mesh["ndof"],) * 2)
    assert np.abs(y.cpu().numpy() - A @ u.cpu().numpy()).max() < 1e-12 * scale
    assert np.abs(dg.cpu().numpy() - A.diagonal()).max() < 1e-13 * scale
    hyb.close()
    ref.close()


def test_refusals_through_the_abi():
    """A conforming LID map, a boundary group of the module, compute_flux, the deterministic flag and a transient context
    are refused with MHA_ERR_INVALID, each naming its cause; outputs stay untouched."""
    import mrhyde_amd
    torch = _torch()
    HVOL, HDIV = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV
    conf = mrhyde_amd.mesh_multi(2, (3, 2), [HVOL, HDIV], [0, 1])
    blk = mrhyde_amd.Block(2, quadrature=2, physics="porousMixedHybridized", variables=[(HVOL, 0), (HDIV, 1)])
    blk.set_mesh(conf["nodes"], conf["lids"], conf["offsets"], conf["ndof"])
    blk.set_orientation(conf["orient"])
    E = conf["nelem"]
    u = torch.zeros(conf["ndof"], dtype=torch.float64, device="cuda")
    lam = torch.zeros((E, 4), dtype=torch.float64, device="cuda")
    S = torch.full((E, 4, 4), 7.0, dtype=torch.float64, device="cuda")
    B = torch.full((E, 9, 9), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="must be DG") as ei:
        blk.pmh_condensed_element(u, lam, schur=S)
    assert ei.value.code == mrhyde_amd.api.ERR_INVALID
    with pytest.raises(mrhyde_amd.MhaError, match="must be DG"):
        blk.pmh_element_blocks(u, lam, blocks=B)
    torch.cuda.synchronize()
    assert bool((S == 7.0).all()) and bool((B == 7.0).all())
    blk.close()

    mesh = mrhyde_amd.mesh_porous_hybrid((3, 2))
    blk = make_block(mesh, "constant")
    be, bs = np.array([0, 1, 2], np.int32), np.zeros(3, np.int32)
    for bc in (mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE, mrhyde_amd.BC_NEUMANN):
        with pytest.raises(mrhyde_amd.MhaError, match="boundary groups of the module") as ei:
            blk.add_boundary_group("bottom", bc, be, bs)
        assert ei.value.code == mrhyde_amd.api.ERR_INVALID
    assert blk.num_boundary_groups() == 0
    gid = blk.add_flux_group("bottom", "u", be, bs)
    u = torch.zeros(mesh["ndof"], dtype=torch.float64, device="cuda")
    flux = torch.full((3, 2), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="computeFlux") as ei:
        blk.compute_flux(gid, u, flux)
    assert ei.value.code == mrhyde_amd.api.ERR_INVALID
    blk.set_graph()
    _, colind = blk.get_graph()
    res = torch.full((mesh["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((len(colind),), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="MHA_ASSEMBLE_DETERMINISTIC") as ei:
        blk.assemble_jacres(u, res, vals, deterministic=True)
    assert ei.value.code == mrhyde_amd.api.ERR_INVALID
    blk.set_function("Kinv_yy", "1+p*p")
    lam = torch.zeros((mesh["nelem"], 4), dtype=torch.float64, device="cuda")
    S = torch.full((mesh["nelem"], 4, 4), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError, match="reads solution fields"):
        blk.pmh_condensed_element(u, lam, schur=S)
    blk.set_function("Kinv_yy", 1.0)
    blk.set_time_integration(True, 1, 1, 0, 0.1, [1.0], [1.0], [1.0, -1.0])
    with pytest.raises(mrhyde_amd.MhaError, match="steady residual"):
        blk.pmh_condensed_element(u, lam, schur=S)
    torch.cuda.synchronize()
    for t in (flux, res, vals, S):
        assert bool((t == 7.0).all())
    blk.close()
    # a block of another module has no such step
    other = mrhyde_amd.Block(2, quadrature=2, physics="porousMixed", variables=[(HVOL, 0), (HDIV, 1)])
    other.set_mesh(mesh["nodes"], mesh["lids"], mesh["offsets"], mesh["ndof"])
    with pytest.raises(mrhyde_amd.MhaError, match="not porousMixedHybridized"):
        other.pmh_condensed_element(u, lam, schur=S)
    other.close()
