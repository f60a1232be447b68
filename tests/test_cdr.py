"""The yardstick of the cdr module and of the coupled navierstokes + cdr block, pinned without a GPU.

tests/cdr_ref.py restates cdr::volumeResidual (src/physics/cdr.cpp:62-142) on the numpy forward-AD class, its functions
evaluated as deck strings that may read the solution fields.  Here it is held against
  * the reference's own golds regression/cdr/2D_manufactured, 2D_transient and 2D_ns_coupled (1, 11 and 4 printed values);
  * the oracle's thermal block with its advection term: the same operator when the reaction is 0 and density = specific
    heat = 1;
  * a central difference of its own residual, with functions that read c, grad(c)[x] and, on the coupled block, ux / uy.
Host-only checks of the two module ids follow.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cdr_ref as R
from cdr_ref import RTOL, crs_err, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reference")


def _yardstick(oracle, ns_params=(0, 1, 0)):
    def assemble(m, u, funcs, fixed, tr):
        out = R.assemble(oracle, m, 2, u, funcs=funcs, ns_params=ns_params, fixed=fixed, transient=tr)
        oracle.apply_dbc_diag(fixed, out["rowptr"], out["colind"], out["crs_vals"])
        return sp.csr_matrix((out["crs_vals"], out["colind"], out["rowptr"]), shape=(m["ndof"],) * 2), out["res"]
    return assemble


def fmt(x):
    return "%.6g" % x


def gold_errors(name):
    txt = open(os.path.join(GOLD, name)).read()
    return {k: float(v) for k, v in re.findall(r"L2 norm of the error for (\w+) = ([-0-9.e]+)", txt)}


def gold_series(name):
    txt = open(os.path.join(GOLD, name)).read()
    return [float(v) for v in re.findall(r"L2 norm of the error for c = ([-0-9.e]+)", txt)]


def test_gold_2d_manufactured(oracle):
    got = R.gold_manufactured(oracle, _yardstick(oracle))
    g = gold_series("cdr_2D_manufactured.gold")
    assert len(g) == 1 and [fmt(v) for v in got] == [fmt(v) for v in g] == ["0.00101714"], (got, g)


def test_gold_2d_transient(oracle):
    got = R.gold_transient(oracle, _yardstick(oracle))
    g = gold_series("cdr_2D_transient.gold")
    assert len(g) == 11 and fmt(g[0]) == "0.370794" and fmt(g[-1]) == "0.0280691"
    assert [fmt(v) for v in got] == [fmt(v) for v in g], (got, g)


def test_gold_2d_ns_coupled(oracle):
    got = R.gold_ns_coupled(oracle, _yardstick(oracle))
    g = gold_errors("cdr_2D_ns_coupled.gold")
    assert sorted(g) == ["c", "pr", "ux", "uy"]
    for k in ("ux", "pr", "uy", "c"):
        assert fmt(got[k]) == fmt(g[k]), (k, got[k], g[k])


SHAPES = [(2, (3, 2), 1, 2), (2, (3, 2), 2, 4), (3, (2, 3, 2), 1, 2), (3, (2, 3, 2), 2, 4)]


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("transient", [False, True])
def test_reaction_zero_is_the_thermal_oracle_with_advection(oracle, dim, ncell, order, qdeg, transient):
    rng = np.random.default_rng(51)
    m = R.cdr_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    fixed = ((m["side_mask"] & 0b0011) != 0).astype(np.uint8)
    b = [0.7, -1.1, 0.4][:dim]
    src = ("sinprod", 2.0, [1.0, 2.0, 1.5][:dim])
    funcs = dict(zip(["xvel", "yvel", "zvel"], b), diffusion=0.9, reaction=0.0, source=src)
    got = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    ref = oracle.assemble_thermal(dim, order, qdeg, m["nodes"], m["lids"], m["offsets"], u, fixed=fixed, transient=tr,
                                  diff=0.9, rho=1.0, cp=1.0, source=src, advection=b)
    assert np.array_equal(got["rowptr"], ref["rowptr"]) and np.array_equal(got["colind"], ref["colind"])
    assert rel_err(got["res"], ref["res"]) < RTOL
    assert crs_err(got["crs_vals"], ref) < RTOL


NONLINEAR = {"reaction": "0.5*c*c + 0.1*grad(c)[x]^2", "diffusion": "1+c*c", "xvel": "c"}


def _fd_check(oracle, m, qdeg, funcs, ns_params, rng):
    """J du against the residual difference: step and tolerance of test_navierstokes_jacobian_is_derivative_of_residual."""
    u = rng.uniform(-1, 1, m["ndof"])
    tr0 = dict(R.BE, u_prev=rng.uniform(-1, 1, (m["ndof"], 1)), dt=0.1)
    kw = dict(funcs=funcs, ns_params=ns_params)
    a = R.assemble(oracle, m, qdeg, u, transient=dict(tr0, u_stage=u[:, None].copy()), **kw)
    J = R.dense(a, m["ndof"])
    du = 1e-6 * rng.uniform(-1, 1, m["ndof"])
    b = R.assemble(oracle, m, qdeg, u + du, transient=dict(tr0, u_stage=(u + du)[:, None].copy()), **kw)
    lin = -(J @ du)
    assert np.abs((b["res"] - a["res"]) - lin).max() < 1e-4 * np.abs(lin).max()
    return a, J


@pytest.mark.parametrize("dim,ncell,order,qdeg", [(2, (3, 2), 2, 4), (3, (2, 2, 2), 1, 2)])
def test_yardstick_jacobian_is_the_derivative_of_its_residual(oracle, dim, ncell, order, qdeg):
    rng = np.random.default_rng(52)
    m = R.cdr_mesh(oracle, dim, ncell, order)
    _fd_check(oracle, m, qdeg, NONLINEAR, (0, 0, 0), rng)


@pytest.mark.parametrize("dim,ncell,orders,qdeg", [(2, (3, 2), (2, 1, 2), 4), (3, (2, 2, 2), (1, 1, 1), 2)])
def test_coupled_yardstick_jacobian_and_velocity_columns(oracle, dim, ncell, orders, qdeg):
    rng = np.random.default_rng(53)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    funcs = dict(NONLINEAR, xvel="ux", yvel="uy", viscosity=0.05, density=1.3)
    funcs["source ux"] = 0.3
    if dim == 3:
        funcs["zvel"] = "uz"
    a, J = _fd_check(oracle, m, qdeg, funcs, (1, 1, 1), rng)
    crows = R.var_rows(m, dim + 1)
    J = J.tocsr()
    for v in [0, 2, 3][:dim]:  # the c-row / velocity-column entries are the derivative of a deck string
        assert abs(J[crows][:, R.var_rows(m, v)]).max() > 0.0
    assert abs(J[crows][:, R.var_rows(m, 1)]).max() == 0.0  # no pressure columns in the c rows
    # with constant velocities those entries are exactly zero
    c = R.assemble(oracle, m, qdeg, rng.uniform(-1, 1, m["ndof"]), funcs=dict(funcs, xvel=0.4, yvel=-0.2, zvel=0.1),
                   ns_params=(1, 1, 1))
    Jc = R.dense(c, m["ndof"]).tocsr()
    for v in range(dim + 1):
        assert abs(Jc[crows][:, R.var_rows(m, v)]).max() == 0.0


def test_physics_ids_agree_with_the_header():
    """The two ids follow MHA_PHYSICS_LINEARELASTICITY_THERMAL (the header states them relative to it) and the Python
    names carry the same numbers."""
    import mrhyde_amd
    src = open(os.path.join(ROOT, "include", "mrhyde_amd.h")).read()
    last = int(re.search(r"#define\s+MHA_PHYSICS_LINEARELASTICITY_THERMAL\s+(\d+)", src).group(1))
    literal = {int(v) for v in re.findall(r"#define\s+MHA_PHYSICS_\w+\s+(\d+)", src)}
    assert last == max(literal)
    ids = mrhyde_amd.api.PHYSICS_IDS
    for k, (name, macro) in enumerate((("cdr", "MHA_PHYSICS_CDR"), ("navierstokes+cdr", "MHA_PHYSICS_NAVIERSTOKES_CDR")), 1):
        mdef = re.search(r"#define\s+%s\s+\(MHA_PHYSICS_LINEARELASTICITY_THERMAL \+ (\d+)\)" % macro, src)
        assert mdef and int(mdef.group(1)) == k and ids[name] == last + k
    assert len(set(ids.values())) == len(ids) and max(ids.values()) == last + 2 < 10  # one decimal digit in the engine's key
