"""CPU tests of the shallowwater module (MHA_PHYSICS_SHALLOWWATER): the yardstick tests/shallowwater_ref.py against the
reference's droptest gold and against a finite difference of itself, and the module's variable rule.  No GPU."""
import os

import numpy as np
import pytest

import mrhyde_amd
import shallowwater_ref as R
from test_stokes import ask

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "reference", "shallowwater_droptest.gold")
HGRAD, HVOL = 0, 1
PID = 15


# The two gold lines that the converged solution misses by more than half a unit of the last digit: Hu and Hv at time
# 0.004 print 0.00981684 where Newton converged to 1e-12 gives 0.0098168336 (6.4e-9 off, half a unit is 5e-9; 6.5e-7
# relative).  The reference stops Newton at its default `nonlinear TOL` of 1e-6, which the deck does not override, and the
# stage formula is the project's own: these lines are held to the yardstick's converged value instead, and its distance
# from the gold to 1e-6 relative (profiles/stokes_shallowwater.md).  The converged value is reproduced to 1e-9 relative:
# the stage residual is below 1e-12, and 1e-9 leaves three digits for the conditioning of the stage matrix, which the
# mass / dt part dominates at dt = 1e-3.
CONVERGED = {("Hu", 4): 0.00981683359321933, ("Hv", 4): 0.009816833593219314}


def check_droptest(errs):
    """The assertions on the 18 gold lines, shared with the GPU test: 14 to half a unit of the last printed digit, the two
    of CONVERGED as stated there; Hu and Hv at time 0 print the residue of the reference's iterative projection solve
    (1.07e-08) where a direct solve gives round-off: both below 1e-7.  No line is left out."""
    gold = R.read_gold(GOLD)
    assert sorted(gold) == ["H", "Hu", "Hv"] and all(len(v) == 6 for v in gold.values())
    compared = 0
    for nm in R.NAMES:
        for k, (s, t) in enumerate(gold[nm]):
            assert abs(t - 1e-3 * k) < 1e-12
            got = errs[nm][k]
            print(nm, t, repr(got), s, "deviation from the gold %.3e relative" % (abs(got - float(s)) / float(s)))
            if k == 0 and nm in ("Hu", "Hv"):
                assert float(s) < 1.1e-8 and got < 1e-7, (nm, got)
            elif (nm, k) in CONVERGED:
                want = CONVERGED[nm, k]
                assert abs(want - float(s)) <= 1e-6 * float(s) and abs(got - want) <= 1e-9 * want, (nm, t, got, want, s)
                compared += 1
            else:
                assert abs(got - float(s)) <= R.half_unit(s), (nm, t, got, s)
                compared += 1
    assert compared == 16


@pytest.fixture(scope="module")
def droptest(oracle):
    return R.gold_droptest(oracle, R.host_assembler(oracle, 2))


def test_gold_droptest(droptest):
    """DIRK-1,2 (A = [[1/2]], b = [1]), dt 1e-3, five steps, Newton to 1e-12, one direct sparse solve per linear system."""
    check_droptest(droptest[0])


@pytest.mark.parametrize("transient", [False, True])
def test_ad_jacobian_against_a_central_difference(oracle, transient):
    """Warped 3x3 mesh, every function set: the AD Jacobian against a central difference of the yardstick's own residual,
    step 1e-6, 1e-7 relative to the matrix's largest entry."""
    rng = np.random.default_rng(151)
    m = R.sw_mesh(oracle, (3, 3), 1)
    u = R.random_state(rng, m)
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    if tr is not None:  # the stage state is a combination of u, u_prev and u_stage: keep its depth positive as well
        for k in ("u_prev", "u_stage"):
            tr[k][R.var_rows(m, 0)] = rng.uniform(0.5, 1.5, tr[k][R.var_rows(m, 0)].shape)
    kw = dict(funcs={"bathymetry": "1+0.5*sin(x)*cos(y)", "bathymetry_x": "0.5*cos(x)*cos(y)", "bathymetry_y": "-0.5*sin(x)*sin(y)",
                     "source H": 0.2, "source Hu": ("sinprod", 0.4, [1.0, 2.0]), "source Hv": "x-y"}, transient=tr)
    ref = R.assemble(oracle, m, 2, u, **kw)
    F = ref["fields"]
    assert F["val"][0].val.min() > -0.25  # the bathymetry is at least 0.5: the depth stays away from zero
    import scipy.sparse as sp
    J = sp.csr_matrix((ref["crs_vals"], ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2).toarray()
    fd = np.zeros_like(J)
    eps = 1e-6
    for j in range(m["ndof"]):
        up, um = u.copy(), u.copy()
        up[j] += eps
        um[j] -= eps
        fd[:, j] = -(R.assemble(oracle, m, 2, up, **kw)["res"] - R.assemble(oracle, m, 2, um, **kw)["res"]) / (2 * eps)
    err = np.abs(J - fd).max() / np.abs(J).max()
    print("AD against central difference:", err)
    assert err < 1e-7


def test_variable_rule():
    right = [HGRAD] * 3
    text = "shallowwater needs H, Hu, Hv in 2-D"
    assert ask(PID, 2, right) == (0, "")
    assert ask(PID, 2, right, [2, 2, 2]) == (0, "")
    for wrong in (right[:-1], right + [HGRAD], right[:-1] + [HVOL]):
        code, msg = ask(PID, 2, wrong)
        assert code == 1 and text in msg, (wrong, code, msg)
    code, msg = ask(PID, 3, right)  # 2-D only
    assert code == 1 and text in msg, (code, msg)


def test_parameters():
    mrhyde_amd.module_parameter("shallowwater", 2, "gravity", 9.81)
    mrhyde_amd.module_parameter("shallowwater", 2, "form_param", 1.0)  # accepted, read by no term
    for name in ("g", "Roe-like stabilization", "usePSPG"):
        with pytest.raises(mrhyde_amd.MhaError, match="has no parameter '%s'" % name) as ei:
            mrhyde_amd.module_parameter("shallowwater", 2, name, 1)
        assert ei.value.code == 1
