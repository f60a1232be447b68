"""Pins the yardstick of the linearelasticity block (tests/linearelasticity_ref.py) without any GPU code: against the
reference's own manufactured-solution golds (regression/le/2D_manufactured, 3D_manufactured, mirrored under
tests/golden/reference/) and by invariants of the operator on warped meshes."""
import numpy as np
import pytest

import linearelasticity_ref as R
from linearelasticity_ref import RTOL, rel_err

def funcs_for(dim):
    """lambda and mu non-constant in x (deck strings), non-zero sources of three kinds."""
    f = {"lambda": "1.1+0.7*sin(0.9*x)", "mu": "0.8+0.3*x", "source dx": 0.3,
         "source dy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim])}
    if dim == 3:
        f["source dz"] = -0.2
    return f


@pytest.mark.parametrize("deck,want", [("le_2D_manufactured", {"dx": "0.000770252", "dy": "0.00121848"}),
                                       ("le_3D_manufactured", {"dx": "0.00872827", "dy": "0.0153095", "dz": "0.0306752"})])
def test_manufactured_golds(oracle, deck, want):
    gold = R.gold_errors(deck + ".gold")
    assert gold == want
    d = R.read_deck(deck + ".input.yaml")
    errs = R.solve_deck(oracle, d)
    for v, e in zip(R.NAMES, errs):
        print(v, e, gold[v])
        assert "%.6g" % e == gold[v], (v, e, gold[v])


def rigid_modes(oracle, m):
    """The dim (dim + 1) / 2 rigid-body modes as dof vectors of an order-1 block: translations and infinitesimal
    rotations.  The coordinates are in the span of the order-1 basis (the geometry is Q1), so the position X_j of dof j
    follows from sum_j X_j N_j(q) = x(q) at the 2^dim points of the degree-2 rule."""
    dim = m["dim"]
    pb = oracle.physical_basis_var(dim, oracle.HGRAD, 1, 2, m["nodes"])
    B, ip = pb["basis"][..., 0], pb["ip"]
    assert B.shape[1] == B.shape[2]
    X = np.linalg.solve(np.transpose(B, (0, 2, 1)), ip)              # [E][card][dim]
    for e in range(m["nelem"]):  # every dof sits on a vertex of its element
        assert np.abs(X[e][:, None, :] - m["nodes"][e][None, :, :]).max(axis=2).min(axis=1).max() < 1e-12
    x = np.zeros((m["ndof"], dim))
    for v in range(dim):
        off = m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]
        x[m["lids"][:, off]] = X
    var = m["dof_var"]
    modes = [(var == d).astype(float) for d in range(dim)]
    for a in range(dim):
        for b in range(a + 1, dim):
            modes.append(np.where(var == a, -x[:, b], 0.0) + np.where(var == b, x[:, a], 0.0))
    return modes


@pytest.mark.parametrize("dim,ncell", [(2, (3, 2)), (3, (2, 2, 1))])
def test_element_jacobian_is_symmetric_and_annihilates_rigid_modes(oracle, dim, ncell):
    rng = np.random.default_rng(61)
    m = R.le_mesh(oracle, dim, ncell, 1)
    u = rng.uniform(-1, 1, m["ndof"])
    f = funcs_for(dim)
    _, J, F = R.element_arrays(oracle, m, 2, u, funcs=f)
    scale = np.abs(J).max()
    assert np.abs(J - np.transpose(J, (0, 2, 1))).max() / scale < RTOL
    modes = rigid_modes(oracle, m)
    assert len(modes) == dim * (dim + 1) // 2
    for r in modes:
        Jr = np.einsum("eij,ej->ei", J, r[m["lids"]])
        assert np.abs(Jr).max() / (scale * max(np.abs(r).max(), 1.0)) < RTOL


@pytest.mark.parametrize("dim,ncell,order", [(2, (3, 2), 1), (2, (2, 2), 2), (3, (2, 1, 2), 1)])
def test_volume_jacobian_is_the_central_difference_of_the_residual(oracle, dim, ncell, order):
    """Step and bound of tests/test_full_size_gpu.py: eps = 1e-5, 1e-7."""
    rng = np.random.default_rng(62)
    m = R.le_mesh(oracle, dim, ncell, order)
    u, dlt = rng.uniform(-1, 1, m["ndof"]), rng.uniform(-1, 1, m["ndof"])
    f, qdeg, eps = funcs_for(dim), 2 * order, 1e-5
    tr = R.transient_state(rng, m["ndof"])
    for t in (None, tr):
        _, J, _ = R.element_arrays(oracle, m, qdeg, u, funcs=f, transient=t)
        Rp, _, _ = R.element_arrays(oracle, m, qdeg, u + eps * dlt, funcs=f, transient=t)
        Rm, _, _ = R.element_arrays(oracle, m, qdeg, u - eps * dlt, funcs=f, transient=t)
        Jd = np.einsum("eij,ej->ei", J, dlt[m["lids"]])
        e = np.abs((Rp - Rm) / (2 * eps) - Jd).max() / np.abs(Jd).max()
        print(e)
        assert e < 1e-7


@pytest.mark.parametrize("dim,ncell,order,side", [(2, (3, 2), 1, "left"), (2, (2, 2), 2, "top"), (3, (2, 2, 1), 1, "front")])
@pytest.mark.parametrize("form_param", [1.0, -1.0])
def test_weak_dirichlet_jacobian_is_the_central_difference_of_its_residual(oracle, dim, ncell, order, side, form_param):
    rng = np.random.default_rng(63)
    m = R.le_mesh(oracle, dim, ncell, order)
    u, dlt = rng.uniform(-1, 1, m["ndof"]), rng.uniform(-1, 1, m["ndof"])
    f, qdeg, eps = funcs_for(dim), 2 * order, 1e-5
    be, bs = oracle.boundary_sides(dim, ncell, side)
    data = [0.4, "0.2+x*y", ("sinprod", 0.7, [1.0, 2.0, 0.5][:dim])][:dim]
    P = dict(form_param=form_param, penalty=7.0)
    kw = dict(funcs=f, params=P, transient=R.transient_state(rng, m["ndof"]))
    _, J = R.boundary_arrays(oracle, m, qdeg, u, be, bs, R.BC_WEAK_DIRICHLET, data, **kw)
    Rp, _ = R.boundary_arrays(oracle, m, qdeg, u + eps * dlt, be, bs, R.BC_WEAK_DIRICHLET, data, **kw)
    Rm, _ = R.boundary_arrays(oracle, m, qdeg, u - eps * dlt, be, bs, R.BC_WEAK_DIRICHLET, data, **kw)
    Jd = np.einsum("eij,ej->ei", J, dlt[m["lids"][be]])
    e = np.abs((Rp - Rm) / (2 * eps) - Jd).max() / np.abs(Jd).max()
    print(e)
    assert e < 1e-7
    # the Nitsche form with form_param = 1 and the Lame stress is symmetric
    if form_param == 1.0:
        assert np.abs(J - np.transpose(J, (0, 2, 1))).max() / np.abs(J).max() < RTOL
    # Neumann: no derivative array, -g_d (N_a, 1)
    Rn, Jn = R.boundary_arrays(oracle, m, qdeg, u, be, bs, R.BC_NEUMANN, data, **kw)
    assert np.abs(Jn).max() == 0.0 and np.abs(Rn).max() > 0.0


def test_incplanestress_is_the_lame_form_with_lambda_twice_mu(oracle):
    rng = np.random.default_rng(64)
    dim, ncell, order, qdeg = 2, (3, 2), 2, 4
    m = R.le_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    f = funcs_for(dim)
    a = R.assemble(oracle, m, qdeg, u, funcs=f, params={"incplanestress": 1})
    b = R.assemble(oracle, m, qdeg, u, funcs=dict(f, **{"lambda": "2*(0.8+0.3*x)"}))
    c = R.assemble(oracle, m, qdeg, u, funcs=f)
    assert rel_err(a["res"], b["res"]) < RTOL and rel_err(a["local_J"], b["local_J"]) < RTOL
    assert rel_err(a["res"], c["res"]) > 1e-3
    # on the side too: the stress of the weak-Dirichlet term changes, the b vectors and the penalty keep lambda
    be, bs = oracle.boundary_sides(dim, ncell, "right")
    data = [0.4, "0.2+x*y"]
    Ra, Ja = R.boundary_arrays(oracle, m, qdeg, u, be, bs, R.BC_WEAK_DIRICHLET, data, funcs=f, params={"incplanestress": 1})
    Rc, Jc = R.boundary_arrays(oracle, m, qdeg, u, be, bs, R.BC_WEAK_DIRICHLET, data, funcs=f)
    assert rel_err(Ra, Rc) > 1e-3 and rel_err(Ja, Jc) > 1e-3


def test_mass_of_the_restatement_is_the_oracle_mass(oracle):
    m = R.le_mesh(oracle, 3, (2, 1, 2), 1)
    for w in (None, [1.0, 0.3, 2.1]):
        assert rel_err(R.get_mass(oracle, m, 2, w), oracle.get_mass(m, 2, w)) < RTOL
