"""Pins the yardstick of the coupled linearelasticity + thermal block and of the stress output
(tests/thermoelastic_ref.py) without any GPU code: against the reference's own regression gold
(regression/thermoelastic/2D_transient, mirrored under tests/golden/reference/), against the two modules' existing
yardsticks where the coupling is off, and by invariants of the stress on warped meshes."""
import numpy as np
import pytest
import scipy.sparse as sp

import linearelasticity_ref as LE
import thermoelastic_ref as R
from ns_thermal_ref import sub_mesh
from thermoelastic_ref import RTOL, rel_err

DECK, GOLD = "thermoelastic_2D_transient.input.yaml", "thermoelastic_2D_transient.gold"


def funcs_for(dim):
    """lambda and mu non-constant in x (deck strings), non-zero sources of three kinds, thermal coefficients off their defaults."""
    f = {"lambda": "1.1+0.7*sin(0.9*x)", "mu": "0.8+0.3*x", "source dx": 0.3,
         "source dy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim]), "thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5][:dim]),
         "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3}
    if dim == 3:
        f["source dz"] = -0.2
    return f


PARAMS = {"alpha_T": 0.35, "T_ambient": 0.3}  # (the default alpha_T = 1e-6 would hide the coupling below the other terms)


def check_gold_series(series, gold):
    """"%.6g" of every one of the 33 printed errors (e, dx, dy at 11 times) equals the gold text."""
    assert all(len(gold[v]) == 11 for v in ("e", "dx", "dy")) and len(series) == 11
    nonzero = 0
    for k, errs in enumerate(series):
        for v, e in zip(("dx", "dy", "e"), errs):
            print(v, k, e, gold[v][k])
            assert "%.6g" % e == gold[v][k], (v, k, e, gold[v][k])
            nonzero += gold[v][k] != "0"
    assert nonzero == 30


def test_transient_gold(oracle):
    """regression/thermoelastic/2D_transient end to end: 20 x 20 Q1, 10 backward-Euler steps, default alpha_T and T_ambient,
    strong zero Dirichlet rows, a direct solve -- every printed digit, no tolerance."""
    gold = R.gold_series(GOLD)
    assert gold["e"][1] == "0.331419" and gold["dx"][10] == "4.75745e-08" and gold["dy"] == gold["dx"]
    deck = LE.read_deck(DECK)
    assert deck["order"] == {"e": 1, "dx": 1, "dy": 1} and deck["quadrature"] == 2

    def step(m, qdeg, u, tr, fixed, funcs):
        ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
        vals = ref["crs_vals"].copy()
        oracle.apply_dbc_diag(fixed, ref["rowptr"], ref["colind"], vals)
        return sp.csr_matrix((vals, ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2), ref["res"]

    _, series = R.run_deck_bwe(oracle, deck, step)
    check_gold_series(series, gold)


@pytest.mark.parametrize("dim,ncell,orders", [(2, (3, 2), (1, 1)), (2, (2, 2), (2, 1)), (3, (2, 1, 2), (1, 1))])
@pytest.mark.parametrize("mode", ["steady", "transient"])
def test_alpha_T_zero_is_the_two_modules_side_by_side(oracle, dim, ncell, orders, mode):
    rng = np.random.default_rng(81)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    qdeg = 2 * orders[0]
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if mode == "transient" else None
    f = funcs_for(dim)
    Rc, Jc, _ = R.element_arrays(oracle, m, qdeg, u, funcs=f, params={"alpha_T": 0.0, "T_ambient": 0.3}, transient=tr)
    n = m["lids"].shape[1]
    de = R.var_off(m, dim)
    dd = np.setdiff1d(np.arange(n), de)

    def sub(keep):
        s, rows = sub_mesh(oracle, m, keep)
        t = None if tr is None else dict(tr, u_prev=tr["u_prev"][rows], u_stage=tr["u_stage"][rows])
        pos = np.zeros(s["lids"].shape, np.int64)  # position in the coupled element of every position of the sub-element
        for k, v in enumerate(keep):
            pos[:, R.var_off(s, k)] = R.var_off(m, v)[None, :]
        assert np.array_equal(np.take_along_axis(m["lids"], pos, axis=1), rows[s["lids"]])
        return s, u[rows], t, pos

    # the displacement block: linearelasticity_ref on the mesh of dx, dy[, dz]
    s, us, ts, pos = sub(list(range(dim)))
    Rl, Jl, _ = LE.element_arrays(oracle, s, qdeg, us, funcs={k: v for k, v in f.items() if k in LE.FUNC_DEFAULTS}, transient=ts)
    E = m["nelem"]
    ar = np.arange(E)[:, None]
    assert rel_err(Rc[ar, pos], Rl) < RTOL
    assert rel_err(Jc[ar[:, :, None], pos[:, :, None], pos[:, None, :]], Jl) < RTOL
    # the e block: the thermal oracle on the mesh of e
    s, us, ts, pos = sub([dim])
    th = oracle.assemble_block(s, oracle.PHYS_THERMAL, qdeg, us, transient=ts, want_local=True,
                               funcs={k: v for k, v in f.items() if k in oracle.PHYS_FUNCS[oracle.PHYS_THERMAL]})
    assert rel_err(-Rc[ar, pos], th["local_res"]) < RTOL
    assert rel_err(Jc[ar[:, :, None], pos[:, :, None], pos[:, None, :]], th["local_J"]) < RTOL
    # no coupling either way
    assert np.all(Jc[:, dd[:, None], de[None, :]] == 0.0) and np.all(Jc[:, de[:, None], dd[None, :]] == 0.0)
    # the displacement-columns of the e row are zero for any alpha_T
    _, J2, _ = R.element_arrays(oracle, m, qdeg, u, funcs=f, params=PARAMS, transient=tr)
    assert np.all(J2[:, de[:, None], dd[None, :]] == 0.0) and np.abs(J2[:, dd[:, None], de[None, :]]).max() > 0.0


@pytest.mark.parametrize("dim,ncell,orders,plane_stress", [(2, (3, 2), (1, 1), 0), (2, (3, 2), (1, 1), 1), (2, (2, 2), (2, 1), 0),
                                                           (2, (2, 2), (2, 1), 1), (3, (2, 1, 2), (1, 1), 0)])
def test_coupling_block_is_minus_alpha_T_c_times_the_gradient_mass(oracle, dim, ncell, orders, plane_stress):
    """d res(a, d) / d e_j = -alpha_T c int d_d N_a N_j, c = 3 lambda + 2 mu, and 5 mu (not 8 mu) under incplanestress."""
    rng = np.random.default_rng(82)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    qdeg = 2 * orders[0]
    u = rng.uniform(-1, 1, m["ndof"])
    f = funcs_for(dim)
    P = dict(PARAMS, incplanestress=plane_stress)
    _, J, F = R.element_arrays(oracle, m, qdeg, u, funcs=f, params=P)
    lam, mu = F["coef"]["lambda"], F["coef"]["mu"]
    c = 5.0 * mu if plane_stress else 3.0 * lam + 2.0 * mu
    de = R.var_off(m, dim)
    for d in range(dim):
        want = -P["alpha_T"] * np.einsum("eq,eaq,ejq,eq->eaj", c, F["G"][d][..., d], F["B"][dim], F["wts"])
        got = J[:, R.var_off(m, d)[:, None], de[None, :]]
        assert rel_err(got, want) < RTOL
        if plane_stress:  # the reference's 5 mu, distinguishable from 3 (2 mu) + 2 mu
            other = -P["alpha_T"] * np.einsum("eq,eaq,ejq,eq->eaj", 8.0 * mu, F["G"][d][..., d], F["B"][dim], F["wts"])
            assert rel_err(got, other) > 1e-3


@pytest.mark.parametrize("dim,ncell,order", [(2, (3, 2), 1), (2, (2, 2), 2), (3, (2, 1, 2), 1)])
def test_coupled_jacobian_is_the_central_difference_of_the_residual(oracle, dim, ncell, order):
    """Step and bound of tests/test_linearelasticity.py: eps = 1e-5, 1e-7."""
    rng = np.random.default_rng(83)
    m = R.coupled_mesh(oracle, dim, ncell, (order, order))
    u, dlt = rng.uniform(-1, 1, m["ndof"]), rng.uniform(-1, 1, m["ndof"])
    f, qdeg, eps = funcs_for(dim), 2 * order, 1e-5
    P = dict(PARAMS, **{"include advection": 1})
    f = dict(f, bx=0.4, by=-0.6)
    tr = R.transient_state(rng, m["ndof"])
    for t in (None, tr):
        kw = dict(funcs=f, params=P, transient=t)
        _, J, _ = R.element_arrays(oracle, m, qdeg, u, **kw)
        Rp, _, _ = R.element_arrays(oracle, m, qdeg, u + eps * dlt, **kw)
        Rm, _, _ = R.element_arrays(oracle, m, qdeg, u - eps * dlt, **kw)
        Jd = np.einsum("eij,ej->ei", J, dlt[m["lids"]])
        e = np.abs((Rp - Rm) / (2 * eps) - Jd).max() / np.abs(Jd).max()
        print(e)
        assert e < 1e-7


LAM, MU, ALPHA, TAMB, E0 = 1.3, 0.7, 0.02, 0.25, 1.5


def test_free_thermal_expansion_in_3d_is_stress_free(oracle):
    m = R.coupled_mesh(oracle, 3, (2, 2, 1), (1, 1))
    x = R.dof_coordinates(oracle, m)
    s = ALPHA * (E0 - TAMB)
    u = np.zeros(m["ndof"])
    for d in range(3):
        u[R.var_rows(m, d)] = s * x[R.var_rows(m, d), d]
    u[R.var_rows(m, 3)] = E0
    out = R.stress_output(oracle, m, 2, u, funcs={"lambda": LAM, "mu": MU}, params={"alpha_T": ALPHA, "T_ambient": TAMB})
    scale = (3 * LAM + 2 * MU) * ALPHA * abs(E0 - TAMB)
    for k in ("stress", "vm", "mag"):
        assert np.abs(out[k]).max() < RTOL * scale, k
    cold = R.stress_output(oracle, m, 2, u, funcs={"lambda": LAM, "mu": MU}, params={"alpha_T": 0.0, "T_ambient": TAMB})
    assert np.abs(cold["stress"]).max() > 0.5 * scale  # the same displacements without the term are stressed


def test_the_same_state_in_2d_keeps_minus_lambda_alpha_T_e(oracle):
    """sxx = syy = (2 lambda + 2 mu) s - (3 lambda + 2 mu) s = -lambda s: what the reference's 2-D form gives."""
    m = R.coupled_mesh(oracle, 2, (3, 2), (1, 1))
    x = R.dof_coordinates(oracle, m)
    s = ALPHA * (E0 - TAMB)
    u = np.zeros(m["ndof"])
    for d in range(2):
        u[R.var_rows(m, d)] = s * x[R.var_rows(m, d), d]
    u[R.var_rows(m, 2)] = E0
    out = R.stress_output(oracle, m, 2, u, funcs={"lambda": LAM, "mu": MU}, params={"alpha_T": ALPHA, "T_ambient": TAMB})
    S = out["stress"]
    scale = (3 * LAM + 2 * MU) * s
    assert np.abs(S[..., 0, 0] + LAM * s).max() < RTOL * scale and np.abs(S[..., 1, 1] + LAM * s).max() < RTOL * scale
    assert np.abs(S[..., 0, 1]).max() < RTOL * scale and np.abs(S[..., 1, 0]).max() < RTOL * scale


def test_hydrostatic_and_pure_shear_states(oracle):
    m = LE.le_mesh(oracle, 3, (2, 1, 2), 1)
    x = R.dof_coordinates(oracle, m)
    g = 0.37
    u = np.zeros(m["ndof"])
    for d in range(3):
        u[R.var_rows(m, d)] = g * x[R.var_rows(m, d), d]
    out = R.stress_output(oracle, m, 2, u, funcs={"lambda": LAM, "mu": MU})
    sig = (3 * LAM + 2 * MU) * g
    assert np.abs(out["vm"]).max() < RTOL * abs(sig) and np.abs(out["mag"] - np.sqrt(3.0) * abs(sig)).max() < RTOL * abs(sig)
    for dim, ncell in ((2, (3, 2)), (3, (2, 1, 2))):
        m = LE.le_mesh(oracle, dim, ncell, 1)
        x = R.dof_coordinates(oracle, m)
        u = np.zeros(m["ndof"])
        u[R.var_rows(m, 0)] = g * x[R.var_rows(m, 0), 1]  # dx = g y
        out = R.stress_output(oracle, m, 2, u, funcs={"lambda": LAM, "mu": MU})
        sxy = MU * g
        assert np.abs(out["stress"][..., 0, 1] - sxy).max() < RTOL * sxy
        assert np.abs(out["vm"] - np.sqrt(3.0) * abs(sxy)).max() < RTOL * sxy and np.abs(out["mag"]).max() < RTOL * sxy


def test_public_names_of_the_coupled_block():
    import os
    import re
    import mrhyde_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mrhyde_amd.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"#define\s+(MHA_PHYSICS_[A-Z_]+)\s+(\d+)", hdr)}
    assert ids["MHA_PHYSICS_LINEARELASTICITY_THERMAL"] == max(ids.values()) and len(set(ids.values())) == len(ids)
    assert mrhyde_amd.api.PHYSICS_IDS["linearelasticity+thermal"] == ids["MHA_PHYSICS_LINEARELASTICITY_THERMAL"]
    lib = mrhyde_amd.load_library()
    for sym in ("mha_num_derived", "mha_derived_name", "mha_get_derived_values"):
        assert sym in mrhyde_amd.api.EXPORTS and hasattr(lib, sym)
    assert lib.mha_num_derived(None) == -1
