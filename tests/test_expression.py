"""Deck function strings (MHA_FUNC_EXPRESSION): the oracle's recursive-descent evaluator against Python on the strings of
the mirrored reference decks, grammar corner cases, and the product's host compiler accepting / rejecting the same
vocabulary (no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest
import yaml

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")


def deck_strings():
    """Every function-like string of the mirrored input decks (Functions:, Neumann / Dirichlet data, true solutions)."""
    out = set()

    def walk(node):
        if isinstance(node, dict):
            for v in node.values():
                walk(v)
        elif isinstance(node, str) and re.search(r"[xyzt]|pi|\d", node) and re.fullmatch(r"[-+*/^().\w\s<>=]+", node):
            out.add(node)

    for f in sorted(os.listdir(GOLD)):
        if f.endswith(".input.yaml"):
            d = yaml.safe_load(open(os.path.join(GOLD, f)))["ANONYMOUS"]
            walk(d.get("Functions", {}))
            walk(d.get("Physics", {}))
            walk(d.get("Postprocess", {}).get("True solutions", {}))
    return sorted(s for s in out if not re.fullmatch(r"[A-Za-z ]+", s))


def py_eval(s, x, y, z, t, nx=0.0, ny=0.0):
    env = {k: getattr(math, k) for k in ("sin", "cos", "tan", "exp", "log", "sqrt", "sinh", "cosh")}
    env.update(abs=abs, pi=math.pi, x=x, y=y, z=z, t=t, nx=nx, ny=ny, nz=0.0, h=0.0)
    return float(eval(s.replace("^", "**"), {"__builtins__": {}}, env))


def test_deck_strings_evaluate(oracle):
    import mrhyde_amd
    strings = [s for s in deck_strings() if not re.search(r"\b(thermal|navier|porous|Stokes|true|false|quad|hex)\b", s)]
    assert any("sin(2*pi*x)" in s for s in strings) and any("cos(2*pi*y)" in s for s in strings)
    rng = np.random.default_rng(1)
    for s in strings:
        try:
            py_eval(s, 0.3, 0.4, 0.5, 0.1)
        except Exception:
            continue  # not a function string (module names, solver options)
        mrhyde_amd.api.check_expression(s)  # the product's compiler accepts every deck function
        for _ in range(5):
            x, y, z, t = rng.uniform(0, 1, 4)
            ref = py_eval(s, x, y, z, t, 0.6, -0.8)
            got = oracle.eval_expression(s, [x, y, z], t, nrm=[0.6, -0.8])
            assert abs(got - ref) <= 1e-13 * max(1.0, abs(ref)), s


@pytest.mark.parametrize("s,val", [("-2^2", -4.0), ("2^-1", 0.5), ("2^3^2", 512.0), ("-(1+2)*3", -9.0), ("1-2-3", -4.0),
                                   ("8/4/2", 1.0), ("(x<0.5)*3+(x>=0.5)*7", 7.0), ("1.5e1+.5", 15.5), ("abs(-x)+sqrt(4)", 2.75),
                                   ("exp(log(3))", 3.0), ("sinh(0)+cosh(0)", 1.0), ("2*pi", 2 * math.pi), ("+x", 0.75)])
def test_grammar_corner_cases(oracle, s, val):
    import mrhyde_amd
    assert abs(oracle.eval_expression(s, [0.75, 0.0, 0.0]) - val) < 1e-13
    mrhyde_amd.api.check_expression(s)


@pytest.mark.parametrize("s", ["2*e", "max(x)", "sin x", "(1+2", "1+", "3 4", "x**2", "emean(x)", ""])
def test_unsupported_strings_are_rejected(oracle, s):
    import mrhyde_amd
    with pytest.raises(mrhyde_amd.MhaError) as e:
        mrhyde_amd.api.check_expression(s)
    assert e.value.code == 1
    if s not in ("x**2",):
        with pytest.raises(ValueError):
            oracle.eval_expression(s, [0.1, 0.2, 0.3])


def test_field_dependent_deck_strings_restatement(oracle):
    """The numpy restatement of FunctionManager<AD>::evaluate (oracle_lib.deck_eval_ad / assemble_thermal_fields) pinned on
    the CPU: with constant strings it reproduces the C oracle's thermal assembly (itself pinned by the reference's golds);
    with 'thermal diffusion' = "1+e*e" the Jacobian is the central difference of the residual, and a named function
    referenced from another string ("kappa0 + e*e") gives the same result as the inlined string."""
    dim, order, qdeg = 2, 2, 4
    m = oracle.mesh_structured(dim, order, (3, 2))
    rng = np.random.default_rng(12)
    nodes = m["nodes"] + 0.03 * rng.uniform(-1, 1, m["nodes"].shape)
    u = rng.uniform(-1, 1, m["ndof"])
    ref = oracle.assemble_thermal(dim, order, qdeg, nodes, m["lids"], m["offsets"], u, diff=1.3, source=("const", 0.7))
    got = oracle.assemble_thermal_fields(dim, order, qdeg, nodes, m["lids"], m["offsets"], u,
                                         {"thermal source": "0.7", "thermal diffusion": "1.3"}, rowptr=ref["rowptr"], colind=ref["colind"])
    assert np.abs(got["crs_vals"] - ref["crs_vals"]).max() < 1e-13 * np.abs(ref["crs_vals"]).max()
    assert np.abs(got["res"] - ref["res"]).max() < 1e-13 * np.abs(ref["res"]).max()
    funcs = {"thermal source": "2*sin(pi*x)*y + 0.1*e", "thermal diffusion": "1+e*e + 0.2*grad(e)[x]^2"}
    out = oracle.assemble_thermal_fields(dim, order, qdeg, nodes, m["lids"], m["offsets"], u, funcs, rowptr=ref["rowptr"], colind=ref["colind"])
    v = rng.uniform(-1, 1, m["ndof"])
    eps = 1e-6
    rp = oracle.assemble_thermal_fields(dim, order, qdeg, nodes, m["lids"], m["offsets"], u + eps * v, funcs, rowptr=ref["rowptr"], colind=ref["colind"])["res"]
    rm = oracle.assemble_thermal_fields(dim, order, qdeg, nodes, m["lids"], m["offsets"], u - eps * v, funcs, rowptr=ref["rowptr"], colind=ref["colind"])["res"]
    import scipy.sparse as sp
    J = sp.csr_matrix((out["crs_vals"], out["colind"], out["rowptr"]), shape=(m["ndof"],) * 2)
    fd = -(rp - rm) / (2 * eps)  # the vector holds -res.val()
    assert np.abs(J @ v - fd).max() < 1e-7 * np.abs(fd).max()
    named = oracle.assemble_thermal_fields(dim, order, qdeg, nodes, m["lids"], m["offsets"], u,
                                           {"thermal source": funcs["thermal source"], "thermal diffusion": "kappa0 + 0.2*grad(e)[x]^2"},
                                           rowptr=ref["rowptr"], colind=ref["colind"], functions={"kappa0": "1+e*e"})
    assert np.abs(named["crs_vals"] - out["crs_vals"]).max() < 1e-14 * np.abs(out["crs_vals"]).max()


# ---- the case table of tests/expression_cases.py: the yardsticks against mpmath, and every entry sensitive to its item ----

import expression_cases as X  # noqa: E402

YTOL = 1e-14  # test_deck_strings_evaluate's bound with one digit of room for the two-function compositions
NPTS = 20
COORD_STRINGS = [e[0] for e in X.COORD] + [X.COORD_ALL, X.STACK12]
FIELD_NAMES = ["c", "c_t", "grad(c)[x]", "grad(c)[y]", "grad(c)[z]"]
COUPLED_NAMES = [p % v for v in ("ux", "pr", "uy") for p in ("%s", "%s_t", "grad(%s)[x]", "grad(%s)[y]")]
FIELD_STRINGS = ([(e[0], FIELD_NAMES) for e in X.FIELD] + [(e[0], FIELD_NAMES + COUPLED_NAMES) for e in X.COUPLED]
                 + [(X.field_all("c", True), FIELD_NAMES), (X.STACK12_FIELD, FIELD_NAMES), (X.INLINE["source"], FIELD_NAMES)])


def _points(rng, names):
    """Random points where every function of the table is tame: coordinates in (0.05, 1.1), the normal and h anything,
    fields with a magnitude in [0.2, 1.3] (gradients up to 3, time derivatives up to 5) and a random sign -- off zero,
    because _AD_FUNCS["abs"] differentiates with np.sign, which is 0 at 0 where the device and Sacado take +1, and off the
    0.1 of the comparison entries."""
    pts = []
    for _ in range(NPTS):
        p = dict(zip("xyz", rng.uniform(0.05, 1.1, 3)), t=X.TIME, h=rng.uniform(0.1, 0.5))
        p.update(zip(("nx", "ny", "nz"), rng.uniform(-1, 1, 3)))
        for nm in names:
            hi = 5.0 if nm.endswith("_t") else 3.0 if nm.startswith("grad") else 1.3
            p[nm] = rng.choice([-1.0, 1.0]) * rng.uniform(0.2, hi)
        pts.append(p)
    return pts


@pytest.mark.parametrize("s", COORD_STRINGS)
def test_coordinate_strings_against_mpmath(oracle, s):
    """oracle.eval_expression (the C evaluator) and deck_eval_ad (the numpy one) on a coordinate string of the table
    against the string evaluated by mpmath at 50 digits; the normal and h are given values here, so that a leaf that
    reads the wrong one shows."""
    pts = _points(np.random.default_rng(31), [])
    fields = {k: oracle.ADView(np.array([[p[k] for p in pts]]), W=1) for k in pts[0]}
    ad = oracle.ADView._lift(oracle.deck_eval_ad(s, fields), fields["t"])
    assert not ad.dx.any()
    for i, p in enumerate(pts):
        ref, _ = X.mp_eval(s, p)
        got = oracle.eval_expression(s, [p["x"], p["y"], p["z"]], p["t"], nrm=[p["nx"], p["ny"], p["nz"]], h=p["h"])
        assert abs(got - ref) <= YTOL * max(1.0, abs(ref)), (s, p, got, ref)
        assert abs(ad.val[0, i] - ref) <= YTOL * max(1.0, abs(ref)), (s, p, ad.val[0, i], ref)
    if s.startswith("(x<x)"):  # the four comparisons at equality
        assert np.all(ad.val == 10.0)


@pytest.mark.parametrize("s,names", FIELD_STRINGS, ids=[s for s, _ in FIELD_STRINGS])
def test_field_strings_against_mpmath(oracle, s, names):
    """deck_eval_ad on a field string of the table: the value, and the derivative along a random direction in the fields
    against mpmath.diff of the same string -- the first check of the yardstick's own rules for tan log sqrt sinh cosh
    abs / and the variable-exponent power."""
    rng = np.random.default_rng(32)
    pts = _points(rng, names)
    dirs = [{nm: rng.uniform(-1, 1) for nm in names} for _ in pts]
    fields = {k: oracle.ADView(np.array([[p[k] for p in pts]]),
                               np.array([[[d.get(k, 0.0)] for d in dirs]])) for k in pts[0]}
    functions = {k: v for k, v in X.INLINE.items() if k != "source"}
    ad = oracle.deck_eval_ad(s, fields, functions)
    for i, (p, d) in enumerate(zip(pts, dirs)):
        flat = s
        for _ in range(3):  # mpmath sees the named functions inlined
            for k, v in functions.items():
                flat = re.sub(r"\b%s\b" % k, "(" + v + ")", flat)
        ref, dref = X.mp_eval(flat, p, d)
        assert abs(ad.val[0, i] - ref) <= YTOL * max(1.0, abs(ref)), (s, p, ad.val[0, i], ref)
        assert abs(ad.dx[0, i, 0] - dref) <= YTOL * max(1.0, abs(dref)), (s, p, d, ad.dx[0, i, 0], dref)
    assert np.abs(ad.dx).max() > 0


def _differs(a, b):
    return np.abs(a - b).max() / np.abs(a).max()


COORD_SENS = X.entries(X.COORD) + [(X.COORD_ALL, "all rules", X.COORD_ALL_MUTANT), (X.STACK12, "stack", X.STACK12.replace("(x)", "(y)"))]


@pytest.mark.parametrize("s,item,mutant", COORD_SENS, ids=[e[0] for e in COORD_SENS])
def test_coordinate_entries_are_sensitive_to_their_item(oracle, s, item, mutant):
    """The sweep's reference with the item swapped for its neighbour differs by more than 1e-3 in the residual: a device
    that confuses the two cannot pass at RTOL.  The normal's and h's entries are sensitive through their mutants (a leaf
    that wrongly reads a coordinate)."""
    shape = "3d-q1" if "z" in item.lower() else "2d-q1"
    ref, mut = X.sweep_reference(oracle, shape, s), X.sweep_reference(oracle, shape, mutant)
    assert _differs(ref["res"], mut["res"]) > 1e-3, (s, item, _differs(ref["res"], mut["res"]))


FIELD_SENS = (X.entries(X.FIELD) + [(X.field_all("c", True), "all rules", X.field_all_mutant("c", True)),
                                    (X.STACK12_FIELD, "stack", X.STACK12_FIELD.replace("11.5+(c)", "11.5-(c)"))])


@pytest.mark.parametrize("s,item,mutant", FIELD_SENS, ids=[e[0] for e in FIELD_SENS])
def test_field_entries_are_sensitive_to_their_item_and_their_derivative(oracle, s, item, mutant):
    """As above, in the residual and in the CRS values; and the CRS values move by more than 1e-3 when the string's
    derivative is dropped (the same values handed over as per-point data), so a missing chain rule shows."""
    when = [e[3] for e in X.FIELD if e[0] == s and len(e) > 3]
    shape, transient = ("3d-q1" if when == ["3d"] else "2d-q1"), when == ["transient"] or "_t" in s
    ref = X.sweep_reference(oracle, shape, s, transient=transient)
    mut = X.sweep_reference(oracle, shape, mutant, transient=transient)
    flat = X.sweep_reference(oracle, shape, s, transient=transient, drop_derivative=True)
    assert _differs(ref["res"], mut["res"]) > 1e-3, (s, item, _differs(ref["res"], mut["res"]))
    assert _differs(ref["crs_vals"], mut["crs_vals"]) > 1e-3, (s, item, _differs(ref["crs_vals"], mut["crs_vals"]))
    assert _differs(ref["res"], flat["res"]) < 1e-13
    assert _differs(ref["crs_vals"], flat["crs_vals"]) > 1e-3, (s, item, _differs(ref["crs_vals"], flat["crs_vals"]))


@pytest.mark.parametrize("s,item,mutant", X.COUPLED, ids=[e[0] for e in X.COUPLED])
def test_coupled_entries_are_sensitive_to_their_item(oracle, s, item, mutant):
    import cdr_ref as R
    rng = np.random.default_rng(X.SEED)
    m = R.coupled_mesh(oracle, 2, (3, 2), (1, 1, 1))
    u = rng.uniform(-1, 1, m["ndof"])
    out = [R.assemble(oracle, m, 2, u, funcs=X.sweep_funcs(2, f, "source"), time=X.TIME) for f in (s, mutant)]
    assert _differs(out[0]["res"], out[1]["res"]) > 1e-3 and _differs(out[0]["crs_vals"], out[1]["crs_vals"]) > 1e-3


def test_stack_limit_in_the_host_compiler():
    """kExprStack = 12: the string that needs exactly twelve entries is accepted, one more level is refused."""
    import mrhyde_amd
    mrhyde_amd.api.check_expression(X.STACK12)
    with pytest.raises(mrhyde_amd.MhaError) as e:
        mrhyde_amd.api.check_expression(X.STACK13)
    assert e.value.code == 1 and "stack" in str(e.value)
