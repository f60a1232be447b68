"""GPU tests of the coupled linearelasticity + thermal block (MHA_PHYSICS_LINEARELASTICITY_THERMAL,
"linearelasticity+thermal") and of the stress output of both elasticity blocks: every case through the C ABI via
mrhyde_amd.Block, against the restatement in tests/thermoelastic_ref.py (which tests/test_thermoelastic.py pins against the
reference's gold).  Helpers and bounds are those of tests/test_ns_thermal_gpu.py, the same engine's tests."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import linearelasticity_ref as LE
import thermoelastic_ref as R
from ns_thermal_ref import sub_mesh
from test_ns_thermal_gpu import _torch, _untouched_after, check_all, configure, make_block, run_gpu, time_kw
from test_thermoelastic import DECK, GOLD, check_gold_series
from thermoelastic_ref import RTOL, crs_err, rel_err

pytestmark = pytest.mark.gpu

PHYS = "linearelasticity+thermal"
# 2-D 4x3: 12 elements at 8 per workgroup leave a partial last workgroup; Q2 displacements with Q1 e: two bases on one
# block; 3-D Q2 with Q2 e (108 dofs) and with Q1 e (89 dofs): one element per workgroup, 153 584 B and 159 888 B of the
# 163 840 B of LDS by the launcher's formula
CASES = [(2, (4, 3), (1, 1)), (2, (4, 3), (2, 1)), (3, (3, 2, 2), (1, 1)), (3, (2, 2, 2), (2, 2)), (3, (2, 2, 2), (2, 1))]
PARAMS = {"alpha_T": 0.35, "T_ambient": 0.3}  # (the default alpha_T = 1e-6 would hide the coupling below the other terms)


def funcs_for(oracle, m, qdeg, dim):
    """lambda a closed form and mu an array, both non-constant in x; sources of three kinds; thermal coefficients off
    their defaults."""
    ip = oracle.physical_basis_var(dim, oracle.HGRAD, 1, qdeg, m["nodes"])["ip"]
    f = {"lambda": ("sinprod", 1.7, [0.9, 1.1, 0.7][:dim]), "mu": ("array", 0.8 + 0.3 * ip[..., 0]), "source dx": 0.3,
         "source dy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim]), "thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5][:dim]),
         "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3}
    if dim == 3:
        f["source dz"] = -0.2
    return f


def fixed_rows(m):
    """strong-Dirichlet rows on two sides, every variable"""
    return ((m["side_mask"] & 0b1100) != 0).astype(np.uint8)


@pytest.mark.parametrize("dim,ncell,orders", CASES)
@pytest.mark.parametrize("mode", ["steady", "transient"])
def test_volume_terms_match_the_restatement_on_every_path(oracle, dim, ncell, orders, mode):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(91)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    qdeg = 2 * orders[0]
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = fixed_rows(m)
    tr = R.transient_state(rng, m["ndof"]) if mode == "transient" else None
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=PARAMS, fixed=fixed, transient=tr)
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, PARAMS)
    out = run_gpu(blk, m, u, tr, len(ref["colind"]), local=True)
    check_all(out, ref)
    for r in np.flatnonzero(fixed)[:30]:
        assert out["res3"][r] == 0.0 and np.all(out["crs_vals3"][ref["rowptr"][r]:ref["rowptr"][r + 1]] == 0.0)
    # the coupling block is there, one way only: e columns in the displacement rows, none of the displacements in e's rows
    J = sp.csr_matrix((out["crs_vals"], ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2)
    free = lambda v: np.array([r for r in R.var_rows(m, v) if not fixed[r]])
    assert abs(J[free(0)][:, R.var_rows(m, dim)]).max() > 0.0 and abs(J[free(dim)][:, R.var_rows(m, 0)]).max() == 0.0
    # strong rows: apply_dbc_diag puts the unit diagonal on them
    vals = torch.tensor(out["crs_vals3"], device="cuda")
    blk.apply_dbc_diag(vals)
    want = out["crs_vals3"].copy()
    oracle.apply_dbc_diag(fixed, ref["rowptr"], ref["colind"], want)
    assert np.array_equal(vals.cpu().numpy(), want)
    with pytest.raises(mrhyde_amd.MhaError) as ei:  # bit-reproducible mode: the affine thermal row-owner path only
        z = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), z, torch.zeros(len(ref["colind"]), dtype=torch.float64, device="cuda"),
                            deterministic=True, **time_kw(blk, tr))
    assert ei.value.code == 1 and "MHA_ASSEMBLE_DETERMINISTIC" in str(ei.value)


@pytest.mark.parametrize("dim,ncell,orders,ws", [(2, (3, 3), (2, 1), 4), (3, (3, 3, 1), (1, 1), 4), (2, (1, 1), (2, 1), 100),
                                                 (3, (1, 1, 1), (1, 1), 100)])
def test_ragged_last_workset_and_single_element_block(oracle, dim, ncell, orders, ws):
    rng = np.random.default_rng(92)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    qdeg = 2 * orders[0]
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=PARAMS, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]), workset_size=ws)
    assert m["nelem"] in (1, 9) and blk.num_worksets() == (m["nelem"] + ws - 1) // ws
    configure(blk, funcs, PARAMS)
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)


@pytest.mark.parametrize("dim,ncell,orders", CASES[:3])
@pytest.mark.parametrize("mode", ["steady", "transient"])
def test_alpha_T_zero_twin_of_the_two_blocks(oracle, dim, ncell, orders, mode):
    """alpha_T = 0: the displacement rows are a linearelasticity block's, the e rows a thermal block's -- both assembled by
    the existing modules on the same mesh."""
    rng = np.random.default_rng(93)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = fixed_rows(m)
    tr = R.transient_state(rng, m["ndof"]) if mode == "transient" else None
    qdeg = 2 * orders[0]
    funcs = funcs_for(oracle, m, qdeg, dim)
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs, {"alpha_T": 0.0, "T_ambient": 0.3})
    out = run_gpu(blk, m, u, tr, len(colind))
    J = sp.csr_matrix((out["crs_vals"], colind, rowptr), shape=(m["ndof"],) * 2)

    def twin(keep, physics, fset):
        s, rows = sub_mesh(oracle, m, keep)
        g = oracle.build_graph(s["ndof"], s["lids"])
        b = make_block(s, physics, qdeg, fixed=fixed[rows], graph=g)
        configure(b, fset, {})
        trs = None if tr is None else dict(tr, u_prev=tr["u_prev"][rows], u_stage=tr["u_stage"][rows])
        o = run_gpu(b, s, u[rows], trs, len(g[1]))
        Js = J[rows][:, rows].tocsr()
        Js.sort_indices()
        assert np.array_equal(Js.indptr, g[0]) and np.array_equal(Js.indices, g[1])
        assert rel_err(out["res"][rows], o["res"]) < RTOL
        assert crs_err(Js.data, dict(crs_vals=o["crs_vals"], rowptr=g[0])) < RTOL
        return rows

    drows = twin(list(range(dim)), "linearelasticity", {k: v for k, v in funcs.items() if k in LE.FUNC_DEFAULTS})
    erows = twin([dim], "thermal", {k: v for k, v in funcs.items() if k in oracle.PHYS_FUNCS[oracle.PHYS_THERMAL]})
    assert abs(J[drows][:, erows]).max() == 0.0 and abs(J[erows][:, drows]).max() == 0.0


def test_parameters_changed_between_assemblies_and_defaults(oracle):
    rng = np.random.default_rng(94)
    dim, orders, qdeg = 2, (2, 1), 4
    m = R.coupled_mesh(oracle, dim, (4, 3), orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    E, nq = m["nelem"], oracle.ref_sizes(dim, 1, qdeg)[1]
    funcs = dict(funcs_for(oracle, m, qdeg, dim), bx=0.4, by=("array", rng.uniform(-1, 1, (E, nq))))
    params = dict(PARAMS, **{"include advection": 1})
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)
    g = dict(rowptr=ref["rowptr"], colind=ref["colind"])
    without = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=dict(params, **{"include advection": 0}), transient=tr, **g)
    assert rel_err(without["res"], ref["res"]) > 1e-3  # the term is there
    # same block, new settings: stale arguments would show
    params2 = dict(params, alpha_T=-1.3, T_ambient=1.1, incplanestress=1)
    configure(blk, {}, params2)
    ref2 = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params2, transient=tr, **g)
    assert rel_err(ref2["res"], ref["res"]) > 1e-3
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref2)
    lame = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=dict(params2, incplanestress=0), transient=tr, **g)
    assert rel_err(lame["res"], ref2["res"]) > 1e-3
    # form_param and penalty are accepted and change nothing
    configure(blk, {}, {"form_param": -1.0, "penalty": 3.0})
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref2)
    # defaults: alpha_T = 1e-6, T_ambient = 0, lambda 1, mu 0.5, thermal coefficients 1
    blk2 = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    blk2.set_function("thermal source", 2.0)
    ref3 = R.assemble(oracle, m, qdeg, u, funcs={"thermal source": 2.0}, transient=tr, **g)
    out3 = run_gpu(blk2, m, u, tr, len(ref["colind"]), local=True)
    check_all(out3, ref3)
    # the coupling entries are 1e-6 of the others and still right entry by entry
    n = m["lids"].shape[1]
    de = R.var_off(m, dim)
    dd = np.setdiff1d(np.arange(n), de)
    want = ref3["local_J"][:, dd[:, None], de[None, :]]
    assert 0.0 < np.abs(want).max() < 1e-5 and rel_err(out3["local_J"][:, dd[:, None], de[None, :]], want) < RTOL


@pytest.mark.parametrize("dim,ncell,orders", [(2, (4, 3), (2, 1)), (3, (3, 2, 2), (1, 1))])
def test_deck_strings_in_the_coordinates(oracle, dim, ncell, orders):
    """lambda, mu and the thermal source as deck strings in x, y, z: the interpreter instantiation of the engine."""
    rng = np.random.default_rng(95)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    qdeg = 2 * orders[0]
    funcs = dict(funcs_for(oracle, m, qdeg, dim), **{"lambda": "1.1+0.7*sin(0.9*x)", "mu": "0.8+0.3*x*y",
                                                    "thermal source": "3*sin(2*x)*cos(y)" + ("+z" if dim == 3 else "")})
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=PARAMS, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, PARAMS)
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)


@pytest.mark.parametrize("dim,ncell,orders", CASES)
def test_get_mass(oracle, dim, ncell, orders):
    torch = _torch()
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    qdeg = 2 * orders[0]
    blk = make_block(m, PHYS, qdeg)
    E, n = m["lids"].shape
    for w in (None, [1.0, 1.3, 0.7, 2.1][:dim] + [0.4]):
        mass = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
        blk.get_mass(mass, w)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), R.get_mass(oracle, m, qdeg, w)) < RTOL


def test_per_variable_workset_views(oracle):
    torch = _torch()
    rng = np.random.default_rng(96)
    dim, orders, qdeg = 2, (2, 1), 4
    m = R.coupled_mesh(oracle, dim, (4, 3), orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=PARAMS, transient=tr)
    F = ref["fields"]
    ws = 5
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]), workset_size=ws)
    configure(blk, funcs, PARAMS)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    assert blk.num_worksets() == 3
    for w in (1, 2):  # a full workset and the ragged last one
        e0, e1 = ws * w, min(ws * w + ws, m["nelem"])
        blk.workset_update(w)
        blk.workset_compute_solution(ud, kw["u_prev"], kw["u_stage"])
        blk.workset_compute_residual(ud, True, kw["u_prev"], kw["u_stage"])
        for v, name in enumerate(R.var_names(dim)):
            assert rel_err(blk.workset_view_numpy("basis " + name)[..., 0], F["B"][v][e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy("basis_grad " + name), F["G"][v][e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy(name), F["val"][v].val[e0:e1]) < RTOL
            for d, c in enumerate("xy"):
                assert rel_err(blk.workset_view_numpy("grad(%s)[%s]" % (name, c)), F["grad"][v][d].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("e_t"), F["dot"][dim].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("res"), -ref["local_res"][e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("res.dx"), ref["local_J"][e0:e1]) < RTOL


def test_set_initial_set_dirichlet_and_flux_on_e_and_a_displacement(oracle):
    torch = _torch()
    rng = np.random.default_rng(97)
    dim, ncell, orders, qdeg = 2, (4, 3), (2, 1), 4
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    nd, n = m["ndof"], m["lids"].shape[1]
    rowptr, colind = oracle.build_graph(nd, m["lids"])
    fixed = ((m["side_mask"] & 1) == 1).astype(np.uint8)   # rows of the left side, every variable
    names = R.var_names(dim)
    assert all(fixed[m["dof_var"] == v].sum() > 0 for v in range(dim + 1))
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(rowptr, colind))
    # set_initial: (initial <var>, basis) per variable and the mass of every variable
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    init = {"dx": "0.3+x*y", "dy": -0.7, "e": "1+sin(x)*y"}
    for v, name in enumerate(names):
        pb = oracle.physical_basis_var(dim, oracle.HGRAD, int(m["orders"][v]), qdeg, m["nodes"])
        data = LE.func_at(oracle, init[name], pb["ip"])
        blk.set_function("initial " + name, init[name])
        oracle.project_rhs(m["lids"], R.var_off(m, v), data[..., None], pb["basis"], pb["wts"], want_rhs)
    oracle.set_initial_mass(m["lids"], R.get_mass(oracle, m, qdeg), False, rowptr, colind, want_vals)
    rhs = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.set_initial(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    # set_dirichlet: strong rows of dx and e on the left side
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    want_rhs, want_vals = np.zeros(nd), np.zeros(len(colind))
    dirichlet = {"dx": "0.5-y+0.25*nx", "dy": 0.0, "e": "2+y*y"}
    for v, name in enumerate(names):
        sb = oracle.physical_side_basis(dim, int(m["orders"][v]), qdeg, m["nodes"], be, bs)
        dip = LE.func_at(oracle, dirichlet[name], sb["ip"], nrm=sb["normals"])
        blk.set_function("Dirichlet %s left" % name, dirichlet[name])
        dvals, mass = oracle.dirichlet_boundary(n, R.var_off(m, v), dip, sb["basis"][..., None], sb["wts"], None)
        oracle.set_dirichlet_group(be, m["lids"], fixed, dvals, mass, False, rowptr, colind, want_vals, want_rhs)
        blk.add_dirichlet_group("left", name, be, bs)
    oracle.set_dirichlet_identity(m["lids"], fixed, rowptr, colind, want_vals)
    rhs, vals = torch.zeros_like(rhs), torch.zeros_like(vals)
    blk.set_dirichlet(rhs, vals)
    torch.cuda.synchronize()
    assert rel_err(rhs.cpu().numpy(), want_rhs) < RTOL and rel_err(vals.cpu().numpy(), want_vals) < RTOL
    for v in (0, dim):
        assert np.abs(want_rhs[(m["dof_var"] == v) & (fixed == 1)]).max() > 0
    # the generic Flux condition on e and on dy
    te, ts = oracle.boundary_sides(dim, ncell, "top")
    expr = "1.5 + x*nx - 2*y*ny + 0.5*sin(3*x+y)"
    for v in (dim, 1):
        sb = oracle.physical_side_basis(dim, int(m["orders"][v]), qdeg, m["nodes"], te, ts)
        flux = LE.func_at(oracle, expr, sb["ip"], nrm=sb["normals"])
        want = np.zeros(nd)
        oracle.flux_condition(te, m["lids"], R.var_off(m, v), flux, sb["wts"], sb["basis"][..., None], want, fixed=fixed)
        b2 = make_block(m, PHYS, qdeg, fixed=fixed)
        b2.set_function("Flux %s top" % names[v], expr)
        b2.add_flux_group("top", names[v], te, ts)
        res = torch.zeros(nd, dtype=torch.float64, device="cuda")
        b2.assemble_boundary(torch.tensor(rng.uniform(-1, 1, nd), device="cuda"), res, compute_jacobian=False)
        torch.cuda.synchronize()
        r = res.cpu().numpy()
        assert rel_err(r, want) < RTOL
        assert len(np.flatnonzero(r)) > 0 and set(np.flatnonzero(r)) <= set(np.flatnonzero(m["dof_var"] == v))


# 2-D Q2 + Q1 e: 18 displacement rows of 22, one wavefront per entry; 3-D Q2 + Q1 e: 81 of 89, one workgroup per entry
@pytest.mark.parametrize("dim,ncell,orders,side", [(2, (4, 3), (2, 1), "right"), (3, (3, 2, 2), (1, 1), "front"),
                                                   (3, (2, 2, 1), (2, 1), "left")])
def test_traction_group_on_the_coupled_block(oracle, dim, ncell, orders, side):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(98)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    qdeg = 2 * orders[0]
    nd = m["ndof"]
    u = rng.uniform(-1, 1, nd)
    tr = R.transient_state(rng, nd)
    fixed = ((m["side_mask"] & 0b1000) != 0).astype(np.uint8)  # top: shares rows with the right side
    funcs = funcs_for(oracle, m, qdeg, dim)
    be, bs = oracle.boundary_sides(dim, ncell, side)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    data = [0.4, "0.2+x*y-nx", rng.uniform(-1, 1, (len(be), nqs))][:dim]
    as_spec = lambda d: ("array", d) if isinstance(d, np.ndarray) else d
    vol = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=PARAMS, fixed=fixed, transient=tr)
    ref = R.add_traction(oracle, m, qdeg, vol, be, bs, [as_spec(d) for d in data], fixed=fixed)
    assert rel_err(ref["res"], vol["res"]) > 1e-3 and np.array_equal(ref["crs_vals"], vol["crs_vals"])
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, PARAMS)
    for d, name in enumerate(R.NAMES[:dim]):
        blk.set_function("Neumann %s %s" % (name, side), torch.tensor(data[d], device="cuda") if isinstance(data[d], np.ndarray) else data[d])
    blk.add_boundary_group(side, mrhyde_amd.BC_NEUMANN, be, bs)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    res = torch.zeros(nd, dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(ref["colind"]), dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    blk.assemble_boundary(ud, res, vals, **kw)
    torch.cuda.synchronize()
    e1, e2 = rel_err(res.cpu().numpy(), ref["res"]), crs_err(vals.cpu().numpy(), ref)
    print("res", e1, "crs", e2)
    assert e1 < RTOL and e2 < RTOL
    # the group alone: displacement rows of the side only, nothing on e's rows, nothing on the fixed rows
    res2 = torch.zeros_like(res)
    blk.assemble_boundary(ud, res2, None, compute_jacobian=False, **kw)
    torch.cuda.synchronize()
    r2 = res2.cpu().numpy()
    assert rel_err(r2, ref["res"] - vol["res"]) < RTOL
    assert np.all(r2[m["dof_var"] == dim] == 0.0) and np.all(r2[fixed == 1] == 0.0) and np.abs(r2).max() > 0.0


def test_the_gold_on_the_device(oracle):
    """regression/thermoelastic/2D_transient: the GPU assembles J and res of the 20 x 20 deck for 10 backward-Euler steps,
    the host solves with scipy, and all 33 printed values match the gold text."""
    torch = _torch()
    import mrhyde_amd
    gold = R.gold_series(GOLD)
    deck = LE.read_deck(DECK)
    st = {}

    def step(m, qdeg, u, tr, fixed, funcs):
        if not st:
            rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
            st.update(rowptr=rowptr, colind=colind, blk=make_block(m, PHYS, qdeg, fixed=fixed, graph=(rowptr, colind)))
            configure(st["blk"], funcs, {})
            st["blk"].set_time_integration(True, 1, 1, 0, tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
        blk = st["blk"]
        res = torch.full((m["ndof"],), 7.0, dtype=torch.float64, device="cuda")
        vals = torch.full((len(st["colind"]),), -3.0, dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, overwrite=True,
                            u_prev=torch.tensor(tr["u_prev"], device="cuda"), u_stage=torch.tensor(tr["u_stage"], device="cuda"))
        blk.apply_dbc_diag(vals)
        torch.cuda.synchronize()
        assert blk.info("last_path") == mrhyde_amd.PATH_ROW_GATHER
        return sp.csr_matrix((vals.cpu().numpy(), st["colind"], st["rowptr"]), shape=(m["ndof"],) * 2), res.cpu().numpy()

    _, series = R.run_deck_bwe(oracle, deck, step)
    check_gold_series(series, gold)


STRESS_CASES = [(2, (4, 3), 1), (2, (4, 3), 2), (3, (2, 2, 2), 1), (3, (2, 2, 2), 2)]


@pytest.mark.parametrize("dim,ncell,order", STRESS_CASES)
@pytest.mark.parametrize("coupled", [False, True])
def test_stress_output(oracle, dim, ncell, order, coupled):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(99)
    oe = 1 if (coupled and order == 2 and dim == 2) else order  # the 2-D Q2 coupled case carries a Q1 e
    m = R.coupled_mesh(oracle, dim, ncell, (order, oe)) if coupled else LE.le_mesh(oracle, dim, ncell, order)
    qdeg = 2 * order
    u = rng.uniform(-1, 1, m["ndof"])
    ip = oracle.physical_basis_var(dim, oracle.HGRAD, 1, qdeg, m["nodes"])["ip"]
    funcs = {"lambda": "1.1+0.7*sin(0.9*x)*y", "mu": ("array", 0.8 + 0.3 * ip[..., 0])}
    params = dict(PARAMS) if coupled else {}
    blk = make_block(m, PHYS if coupled else "linearelasticity", qdeg)
    # names and count through the ABI
    lib = mrhyde_amd.load_library()
    lib.mha_derived_name.restype = C.c_char_p
    lib.mha_derived_name.argtypes = [C.c_void_p, C.c_int]
    assert lib.mha_num_derived(blk._h) == 2
    assert [lib.mha_derived_name(blk._h, k) for k in (0, 1, 2, -1)] == [b"VM stress", b"MAG stress", None, None]
    assert blk.derived_names() == ["VM stress", "MAG stress"]
    ud = torch.tensor(u, device="cuda")
    E, nq = m["nelem"], ip.shape[1]
    for ps in ([0, 1] if dim == 2 else [0]):
        p = dict(params, incplanestress=ps)
        configure(blk, funcs, p)
        ref = R.stress_output(oracle, m, qdeg, u, funcs=funcs, params=p)
        scale = np.abs(ref["stress"]).max()
        stress = torch.full((E, nq, dim, dim), 5.0, dtype=torch.float64, device="cuda")
        out = blk.derived_values(ud, stress=stress)
        torch.cuda.synchronize()
        assert sorted(out) == ["MAG stress", "VM stress"] and out["VM stress"].shape == (E, nq)
        errs = [np.abs(stress.cpu().numpy() - ref["stress"]).max() / scale,
                np.abs(out["VM stress"].cpu().numpy() - ref["vm"]).max() / scale,
                np.abs(out["MAG stress"].cpu().numpy() - ref["mag"]).max() / scale]
        print("plane stress", ps, errs)
        assert max(errs) < RTOL
        # without the tensor: the same derived values
        out2 = blk.derived_values(ud)
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], out2[k])
    if coupled:  # the term is in the output: another alpha_T, other normal stresses (MAG: the 3-D VM does not see a pressure)
        configure(blk, {}, dict(alpha_T=0.0, incplanestress=0))
        cold = blk.derived_values(ud)["MAG stress"].cpu().numpy()
        assert np.abs(cold - R.stress_output(oracle, m, qdeg, u, funcs=funcs, params=dict(params, alpha_T=0.0))["mag"]).max() / scale < RTOL
        assert rel_err(cold, R.stress_output(oracle, m, qdeg, u, funcs=funcs, params=params)["mag"]) > 1e-3


def test_free_thermal_expansion_is_stress_free_on_the_device(oracle):
    torch = _torch()
    lam, mu, alpha, tamb, e0 = 1.3, 0.7, 0.02, 0.25, 1.5
    m = R.coupled_mesh(oracle, 3, (2, 2, 1), (1, 1))
    x = R.dof_coordinates(oracle, m)
    s = alpha * (e0 - tamb)
    u = np.zeros(m["ndof"])
    for d in range(3):
        u[R.var_rows(m, d)] = s * x[R.var_rows(m, d), d]
    u[R.var_rows(m, 3)] = e0
    blk = make_block(m, PHYS, 2)
    configure(blk, {"lambda": lam, "mu": mu}, {"alpha_T": alpha, "T_ambient": tamb})
    E, nq = m["nelem"], 8
    stress = torch.full((E, nq, 3, 3), 5.0, dtype=torch.float64, device="cuda")
    out = blk.derived_values(torch.tensor(u, device="cuda"), stress=stress)
    torch.cuda.synchronize()
    scale = (3 * lam + 2 * mu) * alpha * abs(e0 - tamb)
    for a in (stress, out["VM stress"], out["MAG stress"]):
        assert float(a.abs().max()) < RTOL * scale
    blk.set_physics_parameter("alpha_T", 0.0)  # the same displacements without the term are stressed
    assert float(blk.derived_values(torch.tensor(u, device="cuda"))["MAG stress"].abs().max()) > 0.5 * scale


def test_other_modules_have_no_derived_values(oracle):
    torch = _torch()
    import mrhyde_amd
    m = oracle.mesh_multi(2, (3, 2), [oracle.HGRAD], [1])
    blk = make_block(m, "thermal", 2)
    assert blk.derived_names() == [] and mrhyde_amd.load_library().mha_num_derived(blk._h) == 0
    ud = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    stress = torch.full((m["nelem"], 4, 2, 2), 5.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.derived_values(ud, stress=stress)
    torch.cuda.synchronize()
    assert ei.value.code == 1 and "derived" in str(ei.value) and bool((stress == 5.0).all())
    m3 = oracle.mesh_multi(2, (3, 2), [oracle.HGRAD] * 3, [1, 1, 1])
    assert make_block(m3, "navierstokes", 2).derived_names() == []


def test_options_that_are_not_built_are_refused(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(100)
    dim, ncell, orders, qdeg = 2, (4, 3), (1, 1), 2
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    funcs = funcs_for(oracle, m, qdeg, dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=PARAMS)
    nd, nnz = m["ndof"], len(ref["colind"])
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, PARAMS)
    ud = torch.tensor(u, device="cuda")
    # settings of the reference's constructor whose terms are not built
    for name, value in (("use crystal elasticity", 1), ("Biot", 1), ("use Lame parameters", 0)):
        msg = _untouched_after(lambda r, v: blk.set_physics_parameter(name, value), nd, nnz)
        assert name in msg
    for name, value in (("use crystal elasticity", 0), ("Biot", 0), ("use Lame parameters", 1)):
        blk.set_physics_parameter(name, value)  # the values that leave them off are accepted
    # the bit-reproducible mode
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, deterministic=True), nd, nnz)
    assert "MHA_ASSEMBLE_DETERMINISTIC" in msg
    # weak-Dirichlet and interface groups: refused when added, nothing kept
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    for bc in (mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE):
        msg = _untouched_after(lambda r, v: blk.add_boundary_group("left", bc, be, bs), nd, nnz)
        assert "MHA_BC_WEAK_DIRICHLET" in msg and "MHA_BC_INTERFACE" in msg and blk.num_boundary_groups() == 0
    # a thermal group on e: a Neumann side that carries data for e is thermal's own condition -- refused, nothing written;
    # thermal's weak-Dirichlet and interface conditions on e are the two types refused above
    gid = blk.add_boundary_group("left", mrhyde_amd.BC_NEUMANN, be, bs)
    blk.set_function("Neumann dx left", 0.5)
    blk.set_function("Neumann e left", 4.0)
    msg = _untouched_after(lambda r, v: blk.assemble_boundary(ud, r, v), nd, nnz)
    assert "on e" in msg
    # computeFlux
    nqs = oracle.side_sizes(dim, qdeg)[1]
    flux = torch.full((len(be), nqs), 4.0, dtype=torch.float64, device="cuda")
    msg = _untouched_after(lambda r, v: blk.compute_flux(gid, ud, flux), nd, nnz)
    assert "computeFlux" in msg and bool((flux == 4.0).all())
    # nothing above changed the block: it still assembles the restatement's operator
    check_all(run_gpu(blk, m, u, None, nnz, local=True), ref)
    # a deck string that reads a solution field: refused at launch, outputs untouched
    blk.set_function("thermal diffusion", "1+e*e")
    for kw in (dict(path=mrhyde_amd.PATH_POINT_ENGINE), dict(path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True)):
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, **kw), nd, nnz)
        assert "thermal module" in msg
    blk.set_function("thermal diffusion", 1.7)
    blk.set_function("mu", "0.5+dx*dx")
    stress = torch.full((m["nelem"], 4, 2, 2), 5.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.derived_values(ud, stress=stress)
    torch.cuda.synchronize()
    assert ei.value.code == 1 and bool((stress == 5.0).all())
    # the variable list: dim + 1 HGRAD variables, the displacements of one order
    H = oracle.HGRAD
    for d, variables, order_text in ((2, [(H, 1)] * 2, "dx, dy, e"), (3, [(H, 1)] * 3, "dx, dy, dz, e"),
                                     (2, [(H, 1), (H, 1), (oracle.HVOL, 0)], "dx, dy, e")):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            mrhyde_amd.Block(d, quadrature=2, physics=PHYS, variables=variables)
        assert ei.value.code == 1 and order_text in str(ei.value)
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=4, physics=PHYS, variables=[(H, 2), (H, 1), (H, 1)])
    assert ei.value.code == 1 and "same order" in str(ei.value)
    # the plain block's refusal of an e variable names this module
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=2, physics="linearelasticity", variables=[(H, 1)] * 3)
    assert "thermoelastic" in str(ei.value) and "linearelasticity+thermal" in str(ei.value)
