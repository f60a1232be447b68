"""porousWeakGalerkin without a device: the yardstick of tests/porous_wg_ref.py against the reference's three recorded
decks, its closed-form elimination against condense() of the full block, the yardstick in float64 against itself in
80-bit (the constants the GPU tests use), the mesh helper, the module's rules through the host-only hooks of
csrc/test_hooks.h, and the dispatch table of the new module by a host-only program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mrhyde_amd
import porous_hybrid_ref as R
import porous_wg_ref as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "reference")
HVOL, HDIV, HGRAD = mrhyde_amd.BASIS_HVOL, mrhyde_amd.BASIS_HDIV, mrhyde_amd.BASIS_HGRAD
PID = mrhyde_amd.PHYSICS_POROUS_WEAK_GALERKIN
DECKS = [("porous_WeakGalerkin_2D", (10, 10), ["0.127469", "1.2962", "0.814028", "0.814028"]),
         ("porous_WeakGalerkin_3D", (10, 10, 10), ["0.109212", "4.93896", "0.98109", "0.98109"]),
         ("porous_WeakGalerkin_PermData", (10, 10), ["0.332462", "4.62447", "2.94996", "1.52868"])]


def gold_values(name):
    txt = open(os.path.join(GOLD, name + ".gold")).read()
    return [m.group(1) for m in re.finditer(r"norm of the error for \w+ = (\S+)", txt)]


def printed(v):
    return "%.6g" % v  # the reference prints with the stream's default precision of 6 digits


def deck_perm_data(deck, mesh):
    """Element data of a deck: None, or the `data file` values at the `data points file` point nearest to each element."""
    # WeakGalerkin_3D and WeakGalerkin_PermData are recorded byte for byte, and the reference's files are not well-formed
    # YAML (`Functions:` is indented by three spaces, which the reference's reader takes): they carry the suffix
    # .input.verbatim.yaml, which keeps them out of the decks tests/test_expression.py parses
    name = os.path.join(GOLD, deck + ".input.yaml")
    yaml = open(name if os.path.exists(name) else name.replace(".input.yaml", ".input.verbatim.yaml")).read()
    assert "porous weak Galerkin" in yaml and "assemble face terms: true" in yaml and "quadrature: 2" in yaml
    if "use permeability data: true" not in yaml:
        return None
    assert "data file: perm" in yaml and "data points file: perm_xy" in yaml
    return W.nearest_data(mesh, np.loadtxt(os.path.join(GOLD, deck + ".perm_xy.dat")), np.loadtxt(os.path.join(GOLD, deck + ".perm.dat")))


@pytest.mark.parametrize("deck,ncell,want", DECKS)
def test_yardstick_reproduces_the_recorded_decks(deck, ncell, want):
    """`Dirichlet conditions: pbndry` = 0 on every side, the deck's source, quadrature 2: the four printed norms, by the
    trace solve and the interior step."""
    assert gold_values(deck) == want
    mesh = mrhyde_amd.mesh_porous_weak_galerkin(ncell)
    edata = deck_perm_data(deck, mesh)
    perm = W.const_perm(1.0) if edata is None else W.element_perm(edata)
    state, lam, g2 = W.solve_mesh(mesh, perm, W.gold_source, np.zeros(mesh["ntrace"]))
    gsum = np.zeros(mesh["ntrace"])
    np.add.at(gsum, mesh["trace_lids"].ravel(), g2.ravel())
    assert np.abs(gsum[mesh["trace_side"] == 0]).max() < 1e-12  # the second step's gvec vanishes on the free rows
    got = [printed(v) for v in W.four_errors(mesh, state, lam)]
    print(deck, got, want)
    assert got == want


def inputs(geometry, kind):
    mesh = R.make_mesh(geometry, mrhyde_amd.mesh_porous_weak_galerkin)
    perm, source, edata = W.coefficients(kind, mesh)
    state, lam = W.random_state(mesh, 3)
    return mesh, edata, (mesh["nodes"], mesh["orient"][:, 1:], state, lam[mesh["trace_lids"]], perm, source)


@pytest.mark.parametrize("kind", R.COEFFICIENTS + (W.MIXED,))
def test_yardstick_float64_against_80_bit_and_the_closed_form(kind):
    """The recorded constants hold, and are not stale: every measurement is at most its constant and the family's largest
    is at least a quarter of a constant above 1.  The two guards hold on the yardstick alone.  The closed-form S, g, du
    in 80-bit arithmetic are condense() of the full block in 80-bit arithmetic: below half a rounding of float64 on the
    componentwise scale, that is, the same function at the precision the device is judged at."""
    worst = {}
    for geometry in (W.MIXED_GEOMETRIES if kind == W.MIXED else R.GEOMETRIES):
        fam = R.family(geometry, kind)
        mesh, _, args = inputs(geometry, kind)
        NI = 1 + 4 * mesh["dim"]
        a64, a80 = W.element_blocks(*args, T=np.float64), W.element_blocks(*args, T=W.LD)
        c64, c80 = W.condense(a64, NI), W.condense(a80, NI)
        f80 = W.closed_form(*args, T=W.LD)
        db = max(W.distance(a64[k], a80[k], a80["S_" + k])[0] for k in ("res", "blocks"))
        dc = max(W.distance(c64[k], c80[k], c80["S_" + k])[0] for k in ("schur", "gvec", "du"))
        df = max(W.distance(f80[k].astype(np.float64), c80[k], c80["S_" + k])[0] for k in ("schur", "gvec", "du"))
        # compared in 80-bit, not after rounding to float64
        df80 = max(float(np.max(np.abs(f80[k] - c80[k]) / (W.LD(W.U) * c80["S_" + k]))) for k in ("schur", "gvec", "du"))
        print("%-18s %-13s blocks d = %.3g  condensed d = %.3g  closed form d = %.3g (%.3g unrounded)  cond(M) = %.3g  perm ratio = %.3g"
              % (geometry, kind, db, dc, df, df80, a80["cond_M"].max(), a80["perm_ratio"].max()))
        assert not f80["singular"].any()
        assert df80 < 0.5, (geometry, kind, df80)
        K = W.K_YARDSTICK[fam]
        assert db <= K["blocks"] and dc <= K["condensed"], (geometry, kind, db, dc, K)
        assert a80["cond_M"].max() <= W.COND_GUARD and a80["perm_ratio"].max() <= W.PERM_RATIO_GUARD
        # the structural zeros have no scale
        Sb, NU = a80["S_blocks"], 2 * mesh["dim"]
        iu, it, il = slice(1, 1 + NU), slice(1 + NU, NI), slice(NI, None)
        for rows, cols in ((0, 0), (0, iu), (0, il), (iu, it), (it, 0), (it, il), (il, 0), (il, iu), (il, il)):
            assert np.all(Sb[:, rows, cols] == 0)
        w = worst.setdefault(fam, [0.0, 0.0])
        w[0], w[1] = max(w[0], db), max(w[1], dc)
    for fam, (db, dc) in worst.items():
        K = W.K_YARDSTICK[fam]
        assert (K["blocks"] == 1 or db >= K["blocks"] / 4) and (K["condensed"] == 1 or dc >= K["condensed"] / 4), (fam, db, dc, K)


@pytest.mark.parametrize("geometry", ["2d 3x5 warped", "3d 3x2x2 warped"])
@pytest.mark.parametrize("kind", ["constant", "element data"])
def test_schur_is_the_hybridized_mixed_one_for_element_constant_perm(geometry, kind):
    """perm constant within an element: W = perm M^-1, and S is porousMixedHybridized's schur at Kinv = 1 / perm.  Both in
    80-bit: below half a rounding of float64 on the pmh yardstick's scale."""
    mesh, edata, args = inputs(geometry, kind)
    dim = mesh["dim"]
    f80 = W.closed_form(*args, T=W.LD)
    kinv = R.const_kinv((1 / W.PERM_CONSTANT,) * 3) if edata is None else R.element_kinv(edata)
    h = mrhyde_amd.mesh_porous_hybrid(tuple(int(v) for v in geometry.split()[1].split("x")))
    h = dict(h, nodes=mesh["nodes"])
    assert np.array_equal(h["trace_lids"], mesh["trace_lids"])
    hs, _ = R.random_state(h, 3)
    arr = R.element_blocks(h["nodes"], h["orient"][:, 1:], hs, args[3], kinv, lambda x: np.zeros(x.shape[:2], x.dtype), T=R.LD)
    c = R.condense(arr, 1 + 2 * dim)
    d = float(np.max(np.abs(f80["schur"] - c["schur"]) / (W.LD(W.U) * c["S_schur"])))
    print(geometry, kind, "S against the pmh yardstick: d =", d)
    assert d < 0.5


def test_yardstick_does_not_depend_on_the_face_signs():
    """Flipping every sign of `orient` leaves S and g where they are and flips the u and t parts of du."""
    mesh, _, args = inputs("2d 3x5 warped", "deck strings")
    nodes, o, state, lam, perm, source = args
    flipped = state.copy()
    flipped[:, 1:] *= -1
    a = W.condense(W.element_blocks(nodes, o, state, lam, perm, source), 9)
    b = W.condense(W.element_blocks(nodes, -o, flipped, lam, perm, source), 9)
    for k in ("schur", "gvec"):
        assert W.distance(b[k], a[k], a["S_" + k])[0] < 8
    flip = np.array([1.0] + [-1.0] * 8)
    assert W.distance(b["du"] * flip, a["du"], a["S_du"])[0] < 8


# ---- the mesh helper --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncell", [(3, 5), (1, 1), (3, 2, 2), (67, 1, 1)])
def test_mesh_helper(ncell):
    m, h = mrhyde_amd.mesh_porous_weak_galerkin(ncell), mrhyde_amd.mesh_porous_hybrid(ncell)
    dim, E = len(ncell), int(np.prod(ncell))
    NU, NI = 2 * dim, 1 + 4 * dim
    assert m["nelem"] == E and m["ndof"] == E * NI and m["lids"].shape == (E, NI) and m["orient"].shape == (E, NI)
    for k in ("nodes", "trace_lids", "trace_side"):
        assert np.array_equal(m[k], h[k]), k
    assert m["ntrace"] == h["ntrace"]
    # DG LIDs: a permutation of range(ndof), u's and t's disjoint; the library's own check takes it
    assert sorted(m["lids"].ravel().tolist()) == list(range(m["ndof"])) and m["offsets"].tolist() == list(range(NI))
    assert not set(m["lids"][:, 1:1 + NU].ravel()) & set(m["lids"][:, 1 + NU:].ravel())
    mrhyde_amd.check_dg_lids(m["lids"], m["ndof"])
    # u and t carry the face signs of the hybridized mesh
    assert np.array_equal(m["orient"][:, :1 + NU], h["orient"]) and np.array_equal(m["orient"][:, 1 + NU:], h["orient"][:, 1:])
    assert set(np.unique(m["orient"])) <= {-1, 1}


def test_mesh_helper_refuses_bad_sizes():
    with pytest.raises(mrhyde_amd.MhaError, match="positive"):
        mrhyde_amd.mesh_porous_weak_galerkin((3, 0))
    with pytest.raises(ValueError):
        mrhyde_amd.mesh_porous_weak_galerkin((3,))


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
    src = open(os.path.join(HERE, "..", "include", "mrhyde_amd.h")).read()
    m = re.search(r"#define\s+MHA_PHYSICS_POROUS_WEAK_GALERKIN\s+\(MHA_PHYSICS_LINEARELASTICITY_THERMAL \+ (\d+)\)", src)
    assert m and 7 + int(m.group(1)) == PID == 13 == mrhyde_amd.MODULE_IDS["porousWeakGalerkin"]
    assert PID not in mrhyde_amd.ALL_PHYSICS_IDS.values() and "porousWeakGalerkin" not in mrhyde_amd.ALL_PHYSICS_IDS
    assert all(mrhyde_amd.MODULE_IDS[k] == v for k, v in mrhyde_amd.ALL_PHYSICS_IDS.items())
    assert 11 not in mrhyde_amd.MODULE_IDS.values()


@pytest.mark.parametrize("dim", [2, 3])
def test_variable_rule(dim):
    assert ask(dim, [HVOL, HDIV, HDIV], [0, 1, 1]) == (0, "")
    for types, orders in (([HVOL, HDIV], [0, 1]), ([HDIV, HVOL, HDIV], [1, 0, 1]), ([HVOL], [0]),
                          ([HVOL, HDIV, HDIV, HGRAD], [0, 1, 1, 1]), ([HVOL, HDIV, HGRAD], [0, 1, 1])):
        code, msg = ask(dim, types, orders)
        assert code == 1 and "pint (HVOL, order 0), u and t (HDIV-DG, order 1)" in msg and "pbndry" in msg, msg
    for orders in ([0, 2, 1], [0, 1, 2], [1, 1, 1]):
        code, msg = ask(dim, [HVOL, HDIV, HDIV], orders)
        assert code == 1 and "above lowest order" in msg


def test_one_dimension_is_refused():
    code, msg = ask(1, [HVOL, HDIV, HDIV], [0, 1, 1])
    assert code == 1 and "1-D is not built" in msg and "porousWeakGalerkin" in msg


@pytest.mark.parametrize("bc", [mrhyde_amd.BC_NEUMANN, mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE])
def test_boundary_groups_are_refused(bc):
    code, msg = ask(2, [HVOL, HDIV, HDIV], [0, 1, 1], bc=bc)
    assert code == 1 and "boundary groups of the module" in msg and "Dirichlet pbndry" in msg and "interface" in msg


def test_parameters():
    mrhyde_amd.module_parameter("porousWeakGalerkin", 2, "use permeability data", 1)
    mrhyde_amd.module_parameter("porousWeakGalerkin", 2, "useAC", 0)
    with pytest.raises(mrhyde_amd.MhaError, match="HDIV_AC") as ei:
        mrhyde_amd.module_parameter("porousWeakGalerkin", 3, "useAC", 1)
    assert ei.value.code == 1 and "useAC" in str(ei.value)
    for name in ("use KL expansion", "KL N x", "KL sigma y", "fix_KL_3d"):
        with pytest.raises(mrhyde_amd.MhaError, match="no KL expansion") as ei:
            mrhyde_amd.module_parameter("porousWeakGalerkin", 3, name, 1)
        assert ei.value.code == 1 and name in str(ei.value)
    for name in ("KLUQcoeffs", "KLStochcoeffs", "anything"):
        with pytest.raises(mrhyde_amd.MhaError, match="no parameter vector"):
            mrhyde_amd.module_parameter("porousWeakGalerkin", 3, name, 1, as_vector=True)
    with pytest.raises(mrhyde_amd.MhaError, match="has no parameter 'form_param'"):
        mrhyde_amd.module_parameter("porousWeakGalerkin", 2, "form_param", 1)


def test_a_conforming_lid_map_is_refused_by_the_shared_check():
    """The DG check is porousMixedHybridized's; its default message still names that module."""
    c = mrhyde_amd.mesh_multi(2, (3, 2), [HVOL, HDIV, HDIV], [0, 1, 1])
    with pytest.raises(mrhyde_amd.MhaError, match="must be DG") as ei:
        mrhyde_amd.check_dg_lids(c["lids"], c["ndof"])
    assert ei.value.code == 1 and "belongs to elements 0 and 1" in str(ei.value)


# ---- the dispatch table of the new module -----------------------------------------------------------------------------
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_dispatch_table_of_the_new_module(tmp_path):
    exe = tmp_path / "porous_wg_dispatch_check"
    build = subprocess.run([HIPCC, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Wno-unused-parameter", "-x", "hip",
                            "--cuda-host-only", os.path.join(HERE, "porous_wg_dispatch_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
