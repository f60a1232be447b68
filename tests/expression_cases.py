"""The case table of the device deck-string interpreters (kernels/device_math.hpp: eval_expression on doubles,
eval_expression_dual on value + one directional derivative), shared by tests/test_expression.py (CPU: the yardsticks
against mpmath, the sensitivity of every entry) and tests/test_expression_device_gpu.py (the device against the
yardsticks).  Plain data plus small helpers; TEST INFRASTRUCTURE, not a conftest.

Which entry pins which value of ExprOp (kernels/device_types.hpp) -- a new opcode gets a line here, an entry in COORD (and
in FIELD when the Dual interpreter can execute it) and a term in the all-rules strings:

  EXPR_CONST            COORD "1.25*x+2.5*y+0.75" (three constant indices); INLINE (indices shifted by inlining)
  EXPR_X, EXPR_Y        COORD "1+x-y*y"                      EXPR_Z    COORD "1+x+z" (0 on a 2-D block), FIELD "c*(1+z)"
  EXPR_T                COORD "1+t*x", FIELD "t*c"           EXPR_PI   COORD "x*pi", FIELD "pi*c"
  EXPR_NX EXPR_NY EXPR_NZ   COORD "2+3*nx" ... (0 in volume functions), FIELD "c*(1+nx+ny+nz+h)"; SIDE_3D / SIDE_2D (normals)
  EXPR_H                COORD "1+nx+ny+nz+h", FIELD "c*(1+nx+ny+nz+h)" (0: no caller supplies it)
  EXPR_ADD EXPR_SUB EXPR_MUL EXPR_DIV   COORD "1.5+x+2*y" "1.5+x-2*y" "(1+x)*(2-y)" "(1+x)/(2+y)";
                        FIELD "c+x*c" "c-0.5*c*c" "c/(3+c)" "(1+x)/(3+c)" "1/(3+c)"
  EXPR_POW              COORD "(1+x)^3" "(1+x)^-1.5" "(2+x)^(1+y)"; FIELD "(3+c)^1.5" (no-log branch), "2^c" and
                        "(3+c)^(0.5*c)" (log branch)
  EXPR_LT EXPR_GT EXPR_LE EXPR_GE   COORD "1+(x<0.5)" ... and "(x<x)+2*(x<=x)+4*(x>x)+8*(x>=x)" (= 10: at equality);
                        FIELD "(c>0.1)*c" ... (zero derivative)
  EXPR_NEG              COORD "-x+1.5" "2^-x*3" "2*-x^2" "1--x" (the compiler's special cases); FIELD "-c"
  EXPR_SIN ... EXPR_COSH   COORD and FIELD, one entry per function; EXPR_ABS on FIELD with both signs of the argument
  EXPR_FIELD            FIELD "grad(c)[y]*grad(c)[x]", "grad(c)[z]" (3-D); COUPLED "ux*pr" "grad(ux)[y]" "uy/(3+c)"
  EXPR_FIELD_T          FIELD "c_t*c" (transient)
  the stack (kExprStack = 12)   STACK12 / STACK12_FIELD run, STACK13 is refused by the host compiler

Every entry: (string, the item it pins, a mutant = the string with that item swapped for its nearest neighbour[, when]).
when: "any" (default) | "3d" (needs a 3-D block) | "transient" (sensitive only with a time derivative).  Arguments stay where
the functions are tame and the relative condition number is of order one: |c| stays below 1.3 on the steady shapes of the
GPU tests and below 2 on the transient state of the Q2 shape, where tan(0.7*c) has a condition number of 7, and 3+c > 0."""
import functools
import re

import numpy as np

COORD = [
    ("1.25*x+2.5*y+0.75", "EXPR_CONST", "2.5*x+1.25*y+0.75"),
    ("1+x-y*y", "EXPR_X EXPR_Y", "1+y-x*x"),
    ("1+x+z", "EXPR_Z", "1+x+y"),
    ("1+t*x", "EXPR_T", "1+x*x"),
    ("x*pi", "EXPR_PI", "x*3"),
    ("1+nx+ny+nz+h", "EXPR_H", "1+nx+ny+nz+x"),
    ("2+3*nx", "EXPR_NX", "2+3*x"),
    ("2+3*ny", "EXPR_NY", "2+3*y"),
    ("2+3*nz", "EXPR_NZ", "2+3*y"),
    ("1.5+x+2*y", "EXPR_ADD", "1.5+x-2*y"),
    ("1.5+x-2*y", "EXPR_SUB", "1.5+x+2*y"),
    ("(1+x)*(2-y)", "EXPR_MUL", "(1+x)/(2-y)"),
    ("(1+x)/(2+y)", "EXPR_DIV", "(1+x)*(2+y)"),
    ("(1+x)^3", "EXPR_POW literal exponent", "(1+x)*3"),
    ("(1+x)^-1.5", "EXPR_POW negative exponent", "(1+x)^1.5"),
    ("(2+x)^(1+y)", "EXPR_POW non-literal exponent", "(2+x)*(1+y)"),
    ("-x+1.5", "EXPR_NEG", "x+1.5"),
    ("2^-x*3", "EXPR_NEG under ^", "2^(-x*3)"),
    ("2*-x^2", "EXPR_NEG before ^", "2*(-x)^2"),
    ("1--x", "EXPR_NEG after -", "1-x"),
    ("1+(x<0.5)", "EXPR_LT", "1+(x>0.5)"),
    ("1+(y>0.4)", "EXPR_GT", "1+(y<0.4)"),
    ("1+(x<=0.5)", "EXPR_LE", "1+(x>=0.5)"),
    ("1+(y>=0.4)", "EXPR_GE", "1+(y<=0.4)"),
    ("(x<x)+2*(x<=x)+4*(x>x)+8*(x>=x)", "EXPR_LT EXPR_LE EXPR_GT EXPR_GE at equality", "(x<=x)+2*(x<x)+4*(x>=x)+8*(x>x)"),
    ("1.5+sin(2*x+y)", "EXPR_SIN", "1.5+cos(2*x+y)"),
    ("1.5+cos(2*x+y)", "EXPR_COS", "1.5+sin(2*x+y)"),
    ("tan(0.7*x+0.3*y)", "EXPR_TAN", "sin(0.7*x+0.3*y)"),
    ("exp(x-0.5*y)", "EXPR_EXP", "cosh(x-0.5*y)"),
    ("log(1.5+x+y)", "EXPR_LOG", "sqrt(1.5+x+y)"),
    ("abs(x-2*y)", "EXPR_ABS", "x-2*y"),
    ("sqrt(1+x+2*y)", "EXPR_SQRT", "log(1+x+2*y)"),
    ("sinh(x+y)", "EXPR_SINH", "cosh(x+y)"),
    ("cosh(x-y)", "EXPR_COSH", "sinh(x-y)"),
]

# every rule of the double interpreter in one string (the literal 10 is the comparison entry above)
COORD_ALL = ("1.5 + sin(2*x+y)*cos(x-y) + tan(0.7*x) - exp(-y)/(2+x) + log(1.5+x*y) + abs(x-2*y) + sqrt(1+x+2*y)"
             " + sinh(x)*cosh(y) + (2+x)^(1+y) + (1+x)^-1.5 + 2^-x*3 + (x<0.5) + 2*(y>0.4) + 4*(x<=y) + 8*(y>=0.3)"
             " + t*x + pi*z + nx + ny + nz + h")
COORD_ALL_MUTANT = COORD_ALL.replace("sinh(x)*cosh(y)", "cosh(x)*sinh(y)")

FIELD = [
    ("c+x*c", "EXPR_ADD", "c-x*c"),
    ("c-0.5*c*c", "EXPR_SUB EXPR_MUL", "c+0.5*c*c"),
    ("c/(3+c)", "EXPR_DIV Dual / Dual", "c*(3+c)"),
    ("(1+x)/(3+c)", "EXPR_DIV constant numerator", "(1+x)*(3+c)"),
    ("1/(3+c)", "EXPR_DIV literal numerator", "1*(3+c)"),
    ("(3+c)^1.5", "EXPR_POW constant exponent", "(3+c)*1.5"),
    ("2^c", "EXPR_POW constant base", "2*c"),
    ("(3+c)^(0.5*c)", "EXPR_POW both Duals", "(3+c)*(0.5*c)"),
    ("sin(c)", "EXPR_SIN", "cos(c)"),
    ("cos(c)", "EXPR_COS", "sin(c)"),
    ("tan(0.7*c)", "EXPR_TAN", "sin(0.7*c)"),
    ("sinh(0.8*c)", "EXPR_SINH", "cosh(0.8*c)"),
    ("cosh(0.8*c)", "EXPR_COSH", "sinh(0.8*c)"),
    ("exp(0.5*c)", "EXPR_EXP", "cosh(0.5*c)"),
    ("log(3+c)", "EXPR_LOG", "sqrt(3+c)"),
    ("sqrt(2+c*c)", "EXPR_SQRT", "log(2+c*c)"),
    ("abs(c)", "EXPR_ABS", "c"),
    ("abs(grad(c)[x])", "EXPR_ABS of a gradient slot", "grad(c)[x]"),
    ("(c>0.1)*c", "EXPR_GT", "(c<0.1)*c"),
    ("(c<0.1)*c", "EXPR_LT", "(c>0.1)*c"),
    ("(c>=0.1)*c", "EXPR_GE", "(c<=0.1)*c"),
    ("(c<=0.1)*c", "EXPR_LE", "(c>=0.1)*c"),
    ("-c", "EXPR_NEG", "c"),
    ("c_t*c", "EXPR_FIELD_T", "c*c", "transient"),
    ("t*c", "EXPR_T", "x*c"),
    ("pi*c", "EXPR_PI", "3*c"),
    ("c*(1+z)", "EXPR_Z", "c*(1+y)"),
    ("c*(1+nx+ny+nz+h)", "EXPR_NX EXPR_NY EXPR_NZ EXPR_H", "c*(1+nx+ny+nz+x)"),
    ("grad(c)[y]*grad(c)[x]", "EXPR_FIELD gradient slots", "grad(c)[x]*grad(c)[x]"),
    ("grad(c)[z]", "EXPR_FIELD z slot", "grad(c)[y]", "3d"),
]
# expressions that must stay away from zero at every point for an entry to be differentiable there (the reference
# asserts |value| > 1e-9); abs entries must also see both signs
KINKS = {"abs(c)": "c", "abs(grad(c)[x])": "grad(c)[x]", "(c>0.1)*c": "c-0.1", "(c<0.1)*c": "c-0.1", "(c>=0.1)*c": "c-0.1",
         "(c<=0.1)*c": "c-0.1"}

COUPLED = [
    ("ux*pr", "EXPR_FIELD slots of two other variables", "ux*ux"),
    ("grad(ux)[y]", "EXPR_FIELD gradient slot of another variable", "grad(ux)[x]"),
    ("uy/(3+c)", "EXPR_DIV across variables", "uy*(3+c)"),
]


def field_all(u="c", with_t=False):
    """Every rule of the Dual interpreter in one string, on the field named u; with_t adds the time-derivative operand."""
    s = ("{u}/(3+{u}) + (1+x)/(3+{u}) + (3+{u})^1.5 + 2^{u} + (3+{u})^(0.5*{u}) + sin({u})*cos({u}) + tan(0.7*{u})"
         " + sinh(0.8*{u}) - cosh(0.8*{u}) + exp(0.5*{u}) + log(3+{u}) + sqrt(2+{u}*{u}) + abs({u}) + abs(grad({u})[x])"
         " + ({u}>0.1)*{u} + ({u}<=0.1)*x + ({u}<0.1)*y + ({u}>=0.1)*2 + -{u}*y + t*{u} + pi*grad({u})[y]*grad({u})[x] + z"
         " + nx + ny + nz + h").format(u=u)
    return s + (" + 0.01*%s_t*%s" % (u, u) if with_t else "")


def field_all_mutant(u="c", with_t=False):
    return field_all(u, with_t).replace("sinh(0.8*%s) - cosh(0.8*%s)" % (u, u), "cosh(0.8*%s) - sinh(0.8*%s)" % (u, u))


# kExprStack = 12 entries exactly; one more level; the field twin
STACK12 = "1.5+(2.5*(3.5+(4.5*(5.5+(6.5*(7.5+(8.5*(9.5+(10.5*(11.5+(x)))))))))))"
STACK13 = "0.5*(" + STACK12 + ")"
STACK12_FIELD = STACK12.replace("(x)", "(c)")

# three levels of named functions with constants at every level, named twice: constant indices shifted more than once
INLINE = {"f1": "1.25 + f2*2.5", "f2": "0.75*f3 - 3.5", "f3": "0.125*c + x", "source": "f1*f1 + f2"}

# side data with the normals (thermal_boundary.hip); h is 0 there too
SIDE_3D = "1.5 + x*nx - 2*y*ny + z*nz + 0.5*sin(3*x+y-z) + h"
SIDE_2D = "1.5 + x*nx - 2*y*ny + 0.5*sin(3*x+y) + h"

TIME = 0.37  # the value of t in the sweeps


def entries(table, dim=3, transient=True):
    """(string, item, mutant) of the entries that apply on a block of this dimension / time mode."""
    out = []
    for e in table:
        when = e[3] if len(e) > 3 else "any"
        if (when == "3d" and dim != 3) or (when == "transient" and not transient):
            continue
        out.append(e[:3])
    return out


# ---- the plain high-precision reference: the string evaluated by mpmath at 50 digits --------------------------------

def tagged(text, names):
    """text with ^ -> ** and every name of `names` it uses replaced by an identifier -> (expression, {identifier: name});
    longest names first, so 'grad(c)[x]' goes before 'c' (the substitution of oracle_lib.deck_eval_ad)."""
    expr, tags = text.replace("^", "**"), {}
    for k, nm in enumerate(sorted(names, key=len, reverse=True)):
        pat = re.escape(nm) if not nm.isidentifier() else r"(?<![A-Za-z0-9_])" + re.escape(nm) + r"(?![A-Za-z0-9_(\[])"
        if re.search(pat, expr):
            tags["_v%d_" % k] = nm
            expr = re.sub(pat, "_v%d_" % k, expr)
    return expr, tags


def mp_eval(text, values, direction=None):
    """text at the point `values` (name -> float) -> (value, derivative along `direction` (name -> float) or None), both
    computed by mpmath at 50 digits and rounded to double once.  The literals of the string are the doubles the host
    compiler reads with strtod."""
    import mpmath
    with mpmath.workdps(50):
        env = {k: getattr(mpmath, k) for k in ("sin", "cos", "tan", "exp", "log", "sqrt", "sinh", "cosh")}
        env.update(abs=mpmath.fabs, pi=+mpmath.pi)
        expr, tags = tagged(text, values)
        code = compile(expr, "<deck string>", "eval")

        def at(s):
            loc = dict(env)
            for tag, nm in tags.items():
                loc[tag] = mpmath.mpf(values[nm]) + (s * mpmath.mpf(direction[nm]) if direction and nm in direction else 0)
            return mpmath.mpf(eval(code, {"__builtins__": {}}, loc))
        val = float(at(mpmath.mpf(0)))
        der = float(mpmath.diff(at, mpmath.mpf(0))) if direction is not None else None
    return val, der


# ---- the sweep's cases and references (cdr_ref.assemble), computed once and shared ------------------------------------

SHAPES = {"2d-q1": (2, (3, 2), 1, 2), "3d-q1": (3, (2, 3, 2), 1, 2), "2d-q2": (2, (3, 2), 2, 4)}
# The seed of the sweep's meshes' states.  No integration point may sit on a kink (the reference asserts it).  crs_err has
# a noise floor of its own on the transient state: an entry below a thousandth of its row's largest is a sum of about
# thirty terms of that size, so device and yardstick differ by up to ~30 eps / 1e-3, a few 1e-13, whatever the kernel
# does.  The seeds 161..168 all pass at RTOL on the device, with largest figures between 2.5e-13 and 9.4e-13; 167 leaves
# the most room.
SEED = 167


@functools.lru_cache(maxsize=None)
def _sweep_case(shape, transient):
    import oracle_lib as oracle
    import cdr_ref as R
    dim, ncell, order, qdeg = SHAPES[shape]
    rng = np.random.default_rng(SEED)
    m = R.cdr_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    fixed = ((m["side_mask"] & 0b0011) != 0).astype(np.uint8)
    return m, u, tr, fixed


def sweep_case(oracle, shape, transient):
    """(mesh, u, transient state or None, fixed rows) of a shape of SHAPES: warped, random u."""
    return _sweep_case(shape, bool(transient))


def sweep_funcs(dim, text, slot, extra=None):
    """The string under test in `slot` ("source" | "diffusion"); no reaction, no advection, a small diffusion, so that the
    value slot of the residual is the function itself (plus c_t) and nothing dilutes an error."""
    f = {"reaction": 0.0, "xvel": 0.0, "yvel": 0.0, "diffusion": 0.05}
    if dim == 3:
        f["zvel"] = 0.0
    f[slot] = text
    f.update(extra or {})
    return f


@functools.lru_cache(maxsize=None)
def _sweep_reference(shape, text, slot, transient, drop_derivative, extra):
    import oracle_lib as oracle
    import cdr_ref as R
    dim, ncell, order, qdeg = SHAPES[shape]
    m, u, tr, fixed = _sweep_case(shape, transient)
    funcs = sweep_funcs(dim, text, slot, dict(extra))
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr, time=TIME)
    fields = R.field_dict(oracle, ref["fields"], ["c"], TIME)
    if text in KINKS:
        k = oracle.deck_eval_ad(KINKS[text], fields).val
        assert np.abs(k).min() > 1e-9, (text, shape, "an integration point sits on the kink: pick another SEED")
        if text.startswith("abs"):
            assert k.min() < 0.0 < k.max(), (text, shape, "abs needs both signs of its argument")
    if drop_derivative:  # the same values with the string's derivative dropped: per-point data
        strings = {k: (v if isinstance(v, str) else repr(float(v))) for k, v in funcs.items()}
        vals = oracle.ADView._lift(oracle.deck_eval_ad(text, fields, strings), fields["t"]).val
        ref = R.assemble(oracle, m, qdeg, u, funcs=dict(funcs, **{slot: ("array", vals)}), fixed=fixed, transient=tr, time=TIME)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def sweep_reference(oracle, shape, text, slot="source", transient=False, drop_derivative=False, extra=None):
    """cdr_ref.assemble for one string of the sweep; cached, read-only arrays."""
    return _sweep_reference(shape, text, slot, bool(transient), bool(drop_derivative), tuple(sorted((extra or {}).items())))
