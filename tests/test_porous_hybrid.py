"""porousMixedHybridized without a device: the yardstick of tests/porous_hybrid_ref.py against the reference's two recorded
decks, the yardstick in float64 against itself in 80-bit (the constants the GPU tests use), the mesh helper, and the
module's rules through the host-only hooks of csrc/test_hooks.h."""
import os
import re

import numpy as np
import pytest

import mrhyde_amd
import porous_hybrid_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
HVOL, HDIV, HGRAD = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV, mrhyde_amd.BASIS_HGRAD
PID = mrhyde_amd.PHYSICS_POROUS_MIXED_HYBRIDIZED


def gold_values(name):
    txt = open(os.path.join(GOLD, name + ".gold")).read()
    return [m.group(1) for m in re.finditer(r"norm of the error for \w+ = (\S+)", txt)]


def printed(v):
    return "%.6g" % v  # the reference prints with the stream's default precision of 6 digits


@pytest.mark.parametrize("deck,ncell", [("porous_Mixed_hybrid", (8, 8)), ("porous_Mixed_3D_hybrid", (8, 8, 8))])
def test_yardstick_reproduces_the_recorded_decks(deck, ncell):
    """`Dirichlet conditions: lambda` = 0 on every side, the deck's source, quadrature 2: the three printed norms."""
    yaml = open(os.path.join(GOLD, deck + ".input.yaml")).read()
    assert "porous mixed hybridized" in yaml and "assemble face terms: true" in yaml and "quadrature: 2" in yaml
    want = gold_values(deck)
    assert want == (["0.158697", "1.02259", "1.30353"] if len(ncell) == 2 else ["0.135175", "1.22176", "4.40245"])
    mesh = mrhyde_amd.mesh_porous_hybrid(ncell)
    state, lam, g2 = R.solve_mesh(mesh, R.const_kinv((1.0, 1.0, 1.0)), R.gold_source, np.zeros(mesh["ntrace"]))
    free = mesh["trace_side"] == 0
    gsum = np.zeros(mesh["ntrace"])
    np.add.at(gsum, mesh["trace_lids"].ravel(), g2.ravel())
    assert np.abs(gsum[free]).max() < 1e-12  # the second step's gvec vanishes on the free rows
    got = [printed(v) for v in R.errors(mesh, state, lam)]
    print(deck, got, want)
    assert got == want


def measure(geometry, kind):
    """d of the float64 yardstick against the 80-bit one on one case: (blocks, condensed, cond of A_uu)."""
    mesh = R.make_mesh(geometry, mrhyde_amd.mesh_porous_hybrid)
    kinv, source, _ = R.coefficients(kind, mesh)
    state, lam = R.random_state(mesh, 3)
    NI = 1 + 2 * mesh["dim"]
    args = (mesh["nodes"], mesh["orient"][:, 1:], state, lam[mesh["trace_lids"]], kinv, source)
    a64, a80 = R.element_blocks(*args, T=np.float64), R.element_blocks(*args, T=R.LD)
    c64, c80 = R.condense(a64, NI), R.condense(a80, NI)
    db = max(R.distance(a64[k], a80[k], a80["S_" + k])[0] for k in ("res", "blocks"))
    dc = max(R.distance(c64[k], c80[k], c80["S_" + k])[0] for k in ("schur", "gvec", "du"))
    # the structural zeros have no scale
    n = a80["blocks"].shape[1]
    Sb = a80["S_blocks"]
    assert np.all(Sb[:, 0, 0] == 0) and np.all(Sb[:, 0, NI:] == 0) and np.all(Sb[:, NI:, 0] == 0) and np.all(Sb[:, NI:, NI:] == 0)
    assert n == NI + 2 * mesh["dim"]
    return db, dc, float(c80["cond"].max())


@pytest.mark.parametrize("kind", R.COEFFICIENTS)
def test_yardstick_float64_against_80_bit(kind):
    """The recorded constants hold, and are not stale: every measurement is at most its constant and the family's largest
    is at least a quarter of a constant above 1.  The conditioning guard holds."""
    worst = {}
    for geometry in R.GEOMETRIES:
        fam = R.family(geometry, kind)
        db, dc, cond = measure(geometry, kind)
        print("%-18s %-13s blocks d = %.3g  condensed d = %.3g  cond(A_uu) = %.3g" % (geometry, kind, db, dc, cond))
        K = R.K_YARDSTICK[fam]
        assert db <= K["blocks"] and dc <= K["condensed"], (geometry, kind, db, dc, K)
        assert cond <= R.COND_GUARD, (geometry, kind, cond)
        w = worst.setdefault(fam, [0.0, 0.0])
        w[0], w[1] = max(w[0], db), max(w[1], dc)
    for fam, (db, dc) in worst.items():
        K = R.K_YARDSTICK[fam]
        assert (K["blocks"] == 1 or db >= K["blocks"] / 4) and (K["condensed"] == 1 or dc >= K["condensed"] / 4), (fam, db, dc, K)


def test_yardstick_does_not_depend_on_the_face_signs():
    """Flipping every sign of `orient` leaves S and g where they are and flips the flux part of du."""
    mesh = R.make_mesh("2d 3x5 warped", mrhyde_amd.mesh_porous_hybrid)
    kinv, source, _ = R.coefficients("deck strings", mesh)
    _, lam = R.random_state(mesh, 4)
    state = np.zeros((mesh["nelem"], 5))
    o = mesh["orient"][:, 1:]
    a = R.condense(R.element_blocks(mesh["nodes"], o, state, lam[mesh["trace_lids"]], kinv, source), 5)
    b = R.condense(R.element_blocks(mesh["nodes"], -o, state, lam[mesh["trace_lids"]], kinv, source), 5)
    for k in ("schur", "gvec"):
        assert R.distance(b[k], a[k], a["S_" + k])[0] < 8
    flip = np.array([1, -1, -1, -1, -1.0])
    assert R.distance(b["du"] * flip, a["du"], a["S_du"])[0] < 8


# ---- the mesh helper --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncell", [(3, 5), (1, 1), (3, 2, 2), (67, 1, 1)])
def test_mesh_helper(ncell):
    m = mrhyde_amd.mesh_porous_hybrid(ncell)
    dim, E = len(ncell), int(np.prod(ncell))
    NU, NI = 2 * dim, 1 + 2 * dim
    assert m["nelem"] == E and m["ndof"] == E * NI and m["nodes"].shape == (E, 2 ** dim, dim)
    assert m["ntrace"] == sum(int(np.prod([n + (d == c) for d, n in enumerate(ncell)])) for c in range(dim))
    # DG LIDs: a permutation of range(ndof); the library's own check takes it
    assert sorted(m["lids"].ravel().tolist()) == list(range(m["ndof"])) and m["offsets"].tolist() == list(range(NI))
    mrhyde_amd.check_dg_lids(m["lids"], m["ndof"])
    # face order = HFACE order: the centroid of face k lies where the header says
    cen, mid = R.face_centroids(m), m["nodes"].mean(axis=1)
    for k in range(NU):
        c, s = R.face_dir(k)
        h = 1.0 / ncell[c]
        want = mid.copy()
        want[:, c] += (0.5 if s else -0.5) * h
        assert np.abs(cen[:, k] - want).max() < 1e-14, k
    assert [R.face_dir(k) for k in range(NU)] == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 1)][:NU]
    # every interior face is shared by exactly two elements with the same trace row, and they see the same centroid;
    # boundary faces belong to one element and carry their side
    tl, ts = m["trace_lids"], m["trace_side"]
    assert tl.min() == 0 and tl.max() == m["ntrace"] - 1
    count = np.bincount(tl.ravel(), minlength=m["ntrace"])
    assert np.all(count[ts == 0] == 2) and np.all(count[ts != 0] == 1)
    where = {}
    for e in range(E):
        for k in range(NU):
            where.setdefault(int(tl[e, k]), []).append(cen[e, k])
    for row, cs in where.items():
        assert np.abs(np.array(cs) - cs[0]).max() < 1e-14, row
        side = int(ts[row])
        on = [2 * d + s for d in range(dim) for s in (0, 1) if abs(cs[0][d] - s) < 1e-14]
        assert (side == 0 and not on) or (side - 1 in on and len(on) == 1), (row, side, on)
    assert mrhyde_amd.PMH_SIDES[:NU] == ("left", "right", "bottom", "top", "front", "back")[:NU]
    # the face signs are those of the conforming HDIV mesh
    c = mrhyde_amd.mesh_multi(dim, ncell, [HVOL, HDIV], [0, 1])
    assert np.array_equal(m["orient"], c["orient"]) and np.array_equal(m["nodes"], c["nodes"])


def test_mesh_helper_refuses_bad_sizes():
    with pytest.raises(mrhyde_amd.MhaError, match="positive"):
        mrhyde_amd.mesh_porous_hybrid((3, 0))
    with pytest.raises(ValueError):
        mrhyde_amd.mesh_porous_hybrid((3,))


# ---- the module's rules -------------------------------------------------------------------------------------------------
def ask(dim, types, orders, bc=0):
    lib = mrhyde_amd.load_library()
    f = lib.mha_test_module_rules
    import ctypes as C
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int, C.c_char_p] + [C.c_int] * 4
    t, o = np.asarray(types, np.int32), np.asarray(orders, np.int32)
    c = np.asarray([1 if b == HVOL else 2 * dim if b == HDIV else 2 ** dim for b in types], np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    code = f(PID, dim, len(types), vp(t), vp(o), vp(c), bc, b"left", int(c.sum()), 1, 2 ** (dim - 1), 0)
    return code, lib.mha_last_error().decode()


def test_module_id_and_name():
    src = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "mrhyde_amd.h")).read()
    m = re.search(r"#define\s+MHA_PHYSICS_POROUS_MIXED_HYBRIDIZED\s+\(MHA_PHYSICS_LINEARELASTICITY_THERMAL \+ (\d+)\)", src)
    assert m and 7 + int(m.group(1)) == PID == mrhyde_amd.MODULE_IDS["porousMixedHybridized"]
    assert PID not in mrhyde_amd.ALL_PHYSICS_IDS.values()
    assert all(mrhyde_amd.MODULE_IDS[k] == v for k, v in mrhyde_amd.ALL_PHYSICS_IDS.items())


@pytest.mark.parametrize("dim", [2, 3])
def test_variable_rule(dim):
    assert ask(dim, [HVOL, HDIV], [0, 1]) == (0, "")
    for types, orders in (([HDIV, HVOL], [1, 0]), ([HVOL], [0]), ([HVOL, HDIV, HGRAD], [0, 1, 1]), ([HVOL, HGRAD], [0, 1])):
        code, msg = ask(dim, types, orders)
        assert code == 1 and "p (HVOL, order 0) and u (HDIV-DG, order 1)" in msg and "lambda" in msg, msg
    code, msg = ask(dim, [HVOL, HDIV], [0, 2])
    assert code == 1 and "above lowest order" in msg


def test_one_dimension_is_refused():
    code, msg = ask(1, [HVOL, HDIV], [0, 1])
    assert code == 1 and "1-D is not built" in msg


@pytest.mark.parametrize("bc", [mrhyde_amd.BC_NEUMANN, mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE])
def test_boundary_groups_are_refused(bc):
    code, msg = ask(2, [HVOL, HDIV], [0, 1], bc=bc)
    assert code == 1 and "boundary groups of the module" in msg and "Dirichlet p" in msg and "interface" in msg


def test_kl_options_are_refused_and_permeability_data_is_taken():
    mrhyde_amd.module_parameter("porousMixedHybridized", 2, "use permeability data", 1)
    for name in ("use KL expansion", "KL N x", "KL sigma y", "fix_KL_3d"):
        with pytest.raises(mrhyde_amd.MhaError, match="no KL expansion") as ei:
            mrhyde_amd.module_parameter("porousMixedHybridized", 3, name, 1)
        assert ei.value.code == 1 and name in str(ei.value)
    for name in ("KLUQcoeffs", "KLStochcoeffs"):
        with pytest.raises(mrhyde_amd.MhaError, match="no KL expansion"):
            mrhyde_amd.module_parameter("porousMixedHybridized", 3, name, 1, as_vector=True)
    with pytest.raises(mrhyde_amd.MhaError, match="has no parameter 'form_param'"):
        mrhyde_amd.module_parameter("porousMixedHybridized", 2, "form_param", 1)
    mrhyde_amd.module_parameter("porousMixed", 3, "use KL expansion", 1)  # porousMixed keeps its options


def test_a_conforming_lid_map_is_refused():
    c = mrhyde_amd.mesh_multi(2, (3, 2), [HVOL, HDIV], [0, 1])
    with pytest.raises(mrhyde_amd.MhaError, match="must be DG") as ei:
        mrhyde_amd.check_dg_lids(c["lids"], c["ndof"])
    assert ei.value.code == 1 and "conforming HDIV" in str(ei.value) and "belongs to elements 0 and 1" in str(ei.value)
    with pytest.raises(mrhyde_amd.MhaError, match="out of range"):
        mrhyde_amd.check_dg_lids(np.array([[0, 1, 2, 3, 9]]), 5)
