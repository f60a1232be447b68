"""GPU tests of the coupled navierstokes + thermal block (MHA_PHYSICS_NAVIERSTOKES_THERMAL, "navierstokes+thermal"):
every case through the C ABI via mrhyde_amd.Block, against the restatement of the two reference loop nests in
tests/ns_thermal_ref.py (which tests/test_ns_thermal.py pins against the CPU oracle)."""
import numpy as np
import pytest
import scipy.sparse as sp

import ns_thermal_ref as R
from ns_thermal_ref import RTOL, crs_err, rel_err

pytestmark = pytest.mark.gpu

PHYS = "navierstokes+thermal"
MODES = {"plain": dict(), "supg+pspg transient": dict(useSUPG=1, usePSPG=1), "fix_uz": dict(fix_uz_offsets=1)}
FUNCS = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5]), "source uz": -0.2, "viscosity": 0.05,
         "density": 1.3, "thermal source": ("sinprod", 3.0, [2.0, 1.0, 1.5]), "thermal diffusion": 1.7,
         "specific heat": 1.4}
CASES = [(2, (4, 3), (1, 1, 1)), (2, (3, 2), (2, 1, 2)), (3, (2, 3, 2), (1, 1, 1))]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def funcs_for(dim, extra=None):
    out = {}
    for k, v in FUNCS.items():
        out[k] = (v[0], v[1], v[2][:dim]) if isinstance(v, tuple) else v
    if dim == 2:
        out.pop("source uz")
    out.update(extra or {})
    return out


def make_block(m, physics, qdeg, fixed=None, graph=None, workset_size=100):
    import mrhyde_amd
    blk = mrhyde_amd.Block(m["dim"], quadrature=qdeg, physics=physics, workset_size=workset_size,
                           variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], fixed)
    blk.set_orientation(m["orient"])
    blk.set_graph(*graph) if graph is not None else blk.set_graph()
    return blk


def configure(blk, funcs, params):
    torch = _torch()
    for k, v in funcs.items():
        if isinstance(v, tuple) and v[0] == "array":
            v = torch.tensor(np.ascontiguousarray(v[1]), device="cuda")
        blk.set_function(k, v)
    for k, v in params.items():
        blk.set_physics_parameter(k, v)


def time_kw(blk, tr):
    torch = _torch()
    if tr is None:
        return {}
    blk.set_time_integration(True, 2, 2, 1, tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
    return dict(u_prev=torch.tensor(tr["u_prev"], device="cuda"), u_stage=torch.tensor(tr["u_stage"], device="cuda"))


def run_gpu(blk, m, u, tr, nnz, local=False):
    """The assembly paths of the multi-variable blocks, as tests/test_multi_gpu.py exercises them."""
    torch = _torch()
    import mrhyde_amd
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_POINT_ENGINE, **kw)
    out = dict(res=res.cpu().numpy(), crs_vals=vals.cpu().numpy())
    if local:
        E, n = m["lids"].shape
        lJ = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
        lr = torch.zeros((E, n), dtype=torch.float64, device="cuda")
        blk.compute_local_jacres(ud, lJ, lr, **kw)
        out["local_J"], out["local_res"] = lJ.cpu().numpy(), lr.cpu().numpy()
        res2, vals2 = torch.zeros_like(res), torch.zeros_like(vals)
        blk.assemble_jacres(ud, res2, vals2, path=mrhyde_amd.PATH_LOCAL_THEN_SCATTER, **kw)
        out["res2"], out["crs_vals2"] = res2.cpu().numpy(), vals2.cpu().numpy()
        # row-gather path: overwrite semantics on garbage, then accumulate on top
        res3, vals3 = torch.full_like(res, 7.0), torch.full_like(vals, -3.0)
        blk.assemble_jacres(ud, res3, vals3, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
        r3, v3 = res3.cpu().numpy().copy(), vals3.cpu().numpy().copy()
        out["res3"], out["crs_vals3"] = r3, v3
        blk.assemble_jacres(ud, res3, vals3, path=mrhyde_amd.PATH_ROW_GATHER, **kw)
        assert rel_err(res3.cpu().numpy(), 2 * r3) < 1e-14 and rel_err(vals3.cpu().numpy(), 2 * v3) < 1e-14
        # residual-only pass leaves the matrix alone
        blk.assemble_jacres(ud, res3, vals3, path=mrhyde_amd.PATH_ROW_GATHER, compute_jacobian=False, overwrite=True, **kw)
        assert rel_err(res3.cpu().numpy(), r3) < 1e-14 and rel_err(vals3.cpu().numpy(), 2 * v3) < 1e-14
        # AUTO takes the row gather on this block
        res4, vals4 = torch.full_like(res, 1.0), torch.full_like(vals, 2.0)
        blk.assemble_jacres(ud, res4, vals4, overwrite=True, **kw)
        assert blk.info("last_path") == mrhyde_amd.PATH_ROW_GATHER
        assert rel_err(res4.cpu().numpy(), r3) < 1e-14 and rel_err(vals4.cpu().numpy(), v3) < 1e-14
    torch.cuda.synchronize()
    return out


def check_all(out, ref):
    for k in ("res", "local_res", "local_J"):
        e = rel_err(out[k], ref[k])
        print(k, e)
        assert e < RTOL, k
    for k in ("crs_vals", "crs_vals2", "crs_vals3"):
        e = crs_err(out[k], ref)
        print(k, e)
        assert e < RTOL, k
    assert rel_err(out["res2"], ref["res"]) < RTOL and rel_err(out["res3"], ref["res"]) < RTOL


def fixed_rows(m):
    """strong-Dirichlet rows on two sides: the velocities and e, not the pressure"""
    return (((m["side_mask"] & 0b1100) != 0) & (m["dof_var"] != 1)).astype(np.uint8)


@pytest.mark.parametrize("dim,ncell,orders", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_coupled_block_matches_the_restatement(oracle, dim, ncell, orders, mode):
    rng = np.random.default_rng(51)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = fixed_rows(m)
    tr = R.transient_state(rng, m["ndof"]) if mode.startswith("supg") else None
    funcs, params = funcs_for(dim), dict(MODES[mode], beta=0.7, T_ambient=0.3)
    qdeg = 2 * orders[0]
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, fixed=fixed, transient=tr)
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    out = run_gpu(blk, m, u, tr, len(ref["colind"]), local=True)
    check_all(out, ref)
    for r in np.flatnonzero(fixed)[:30]:
        assert out["res3"][r] == 0.0 and np.all(out["crs_vals3"][ref["rowptr"][r]:ref["rowptr"][r + 1]] == 0.0)
    J = sp.csr_matrix((out["crs_vals"], ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2)
    free = lambda v: np.array([r for r in R.var_rows(m, v) if not fixed[r]])
    # the coupling blocks are there: e columns in the momentum rows, velocity columns in the energy rows
    assert abs(J[free(2)][:, R.var_rows(m, dim + 1)]).max() > 0.0 and abs(J[free(dim + 1)][:, R.var_rows(m, 0)]).max() > 0.0
    if dim == 3 and mode != "fix_uz":  # the reference's uz-offset quirk: uz rows stay empty, buoyancy included
        assert np.all(out["res"][m["dof_var"] == 3] == 0.0)
    import mrhyde_amd
    with pytest.raises(mrhyde_amd.MhaError):  # bit-reproducible mode: the affine thermal row-owner path only
        torch = _torch()
        z = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), z, torch.zeros(len(ref["colind"]), dtype=torch.float64, device="cuda"),
                            deterministic=True, **time_kw(blk, tr))


@pytest.mark.parametrize("dim,ncell,orders", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_beta_zero_twin_of_the_existing_kernels(oracle, dim, ncell, orders, mode):
    """beta = 0: the momentum / continuity rows are a navierstokes block's, the energy rows a thermal block's whose
    advection is the state's velocity at the points -- both assembled by the existing kernels on the same mesh."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(52)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = fixed_rows(m)
    tr = R.transient_state(rng, m["ndof"]) if mode.startswith("supg") else None
    funcs, params = funcs_for(dim), dict(MODES[mode], beta=0.0, T_ambient=0.3)
    qdeg = 2 * orders[0]
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    blk = make_block(m, PHYS, qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs, params)
    out = run_gpu(blk, m, u, tr, len(colind))
    J = sp.csr_matrix((out["crs_vals"], colind, rowptr), shape=(m["ndof"],) * 2)

    def twin(keep, physics, fset, pset):
        s, rows = R.sub_mesh(oracle, m, keep)
        g = oracle.build_graph(s["ndof"], s["lids"])
        b = make_block(s, physics, qdeg, fixed=fixed[rows], graph=g)
        configure(b, fset, pset)
        trs = None if tr is None else dict(tr, u_prev=tr["u_prev"][rows], u_stage=tr["u_stage"][rows])
        o = run_gpu(b, s, u[rows], trs, len(g[1]))
        Js = J[rows][:, rows].tocsr()
        Js.sort_indices()
        assert np.array_equal(Js.indptr, g[0]) and np.array_equal(Js.indices, g[1])
        assert rel_err(out["res"][rows], o["res"]) < RTOL
        assert crs_err(Js.data, dict(crs_vals=o["crs_vals"], rowptr=g[0])) < RTOL
        return rows

    nsf = {k: v for k, v in funcs.items() if k in oracle.PHYS_FUNCS[oracle.PHYS_NAVIERSTOKES]}
    nrows = twin(list(range(dim + 1)), "navierstokes", nsf, MODES[mode])
    assert abs(J[nrows][:, R.var_rows(m, dim + 1)]).max() == 0.0
    F = R.fields_at_points(oracle, m, qdeg, u, tr)
    thf = {"thermal source": funcs["thermal source"], "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3}
    for d, k in enumerate(["bx", "by", "bz"][:dim]):
        thf[k] = ("array", F["val"][[0, 2, 3][d]].val)
    twin([dim + 1], "thermal", thf, {"include advection": 1})


def test_include_advection_and_parameters_changed_between_assemblies(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(53)
    dim, orders, qdeg = 2, (2, 1, 2), 4
    m = R.coupled_mesh(oracle, dim, (3, 2), orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    E, nq = m["nelem"], oracle.ref_sizes(dim, 1, qdeg)[1]
    funcs = funcs_for(dim, {"bx": 0.4, "by": ("array", rng.uniform(-1, 1, (E, nq)))})
    params = {"useSUPG": 1, "usePSPG": 1, "beta": 0.7, "T_ambient": 0.3, "include advection": 1}
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs, params)
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)
    without = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=dict(params, **{"include advection": 0}), transient=tr)
    assert rel_err(without["res"], ref["res"]) > 1e-3  # the term is there
    # same block, new settings
    params2 = dict(params, beta=-1.3, T_ambient=1.1)
    configure(blk, {}, params2)
    ref2 = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params2, transient=tr, rowptr=ref["rowptr"], colind=ref["colind"])
    assert rel_err(ref2["res"], ref["res"]) > 1e-3
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref2)
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.set_physics_parameter("form_param", 2.0)
    assert ei.value.code != 0 and "no parameter" in str(ei.value)
    # defaults: T_ambient 0, beta 1, density shared by both modules
    blk2 = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    blk2.set_function("density", 1.9)
    blk2.set_function("source uy", -1.0)
    ref3 = R.assemble(oracle, m, qdeg, u, funcs={"density": 1.9, "source uy": -1.0}, transient=tr, rowptr=ref["rowptr"],
                      colind=ref["colind"])
    check_all(run_gpu(blk2, m, u, tr, len(ref["colind"]), local=True), ref3)


@pytest.mark.parametrize("dim,ncell,orders,ws", [(2, (3, 3), (2, 1, 2), 4), (3, (3, 1, 2), (1, 1, 1), 4), (2, (1, 1), (2, 1, 2), 100),
                                                 (3, (1, 1, 1), (1, 1, 1), 100)])
def test_ragged_last_workset_and_single_element_block(oracle, dim, ncell, orders, ws):
    rng = np.random.default_rng(54)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs, params = funcs_for(dim), dict(useSUPG=1, usePSPG=1, beta=0.7, T_ambient=0.3)
    qdeg = 2 * orders[0]
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]), workset_size=ws)
    assert blk.num_worksets() == (m["nelem"] + ws - 1) // ws and (m["nelem"] % ws != 0 or m["nelem"] == 1)
    configure(blk, funcs, params)
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)


@pytest.mark.parametrize("dim,ncell,orders", CASES)
def test_get_mass_on_the_coupled_block(oracle, dim, ncell, orders):
    torch = _torch()
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    qdeg = 2 * orders[0]
    blk = make_block(m, PHYS, qdeg)
    E, n = m["lids"].shape
    wts = [1.0, 0.0, 1.3, 0.7, 2.1][:dim + 2]
    for w in (None, wts):
        mass = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
        blk.get_mass(mass, w)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), oracle.get_mass(m, qdeg, w)) < RTOL


def test_workset_views_on_the_coupled_block(oracle):
    torch = _torch()
    rng = np.random.default_rng(55)
    dim, orders, qdeg = 2, (2, 1, 2), 4
    m = R.coupled_mesh(oracle, dim, (3, 3), orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs, params = funcs_for(dim), dict(useSUPG=1, usePSPG=1, beta=0.7, T_ambient=0.3)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, transient=tr)
    F = ref["fields"]
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]), workset_size=4)
    configure(blk, funcs, params)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    names = F["names"]
    for w in range(blk.num_worksets()):
        e0, e1 = 4 * w, min(4 * w + 4, m["nelem"])
        blk.workset_update(w)
        blk.workset_compute_solution(ud, kw["u_prev"], kw["u_stage"])
        blk.workset_compute_residual(ud, True, kw["u_prev"], kw["u_stage"])
        for v, name in enumerate(names):
            assert rel_err(blk.workset_view_numpy("basis " + name)[..., 0], F["B"][v][e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy("basis_grad " + name), F["G"][v][e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy(name), F["val"][v].val[e0:e1]) < RTOL
            assert rel_err(blk.workset_view_numpy(name + "_t"), F["dot"][v].val[e0:e1]) < RTOL
            for d, c in enumerate("xy"):
                assert rel_err(blk.workset_view_numpy("grad(%s)[%s]" % (name, c)), F["grad"][v][d].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("res"), -ref["local_res"][e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("res.dx"), ref["local_J"][e0:e1]) < RTOL


@pytest.mark.parametrize("dim,ncell,orders", CASES)
def test_deck_strings_in_the_coordinates(oracle, dim, ncell, orders):
    """Deck strings in x, y, z, t run the interpreter instantiation of the engine under the default scratch limit."""
    rng = np.random.default_rng(56)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs, params = funcs_for(dim), dict(useSUPG=1, usePSPG=1, beta=0.7, T_ambient=0.3)
    qdeg = 2 * orders[0]
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, transient=tr)
    blk = make_block(m, PHYS, qdeg, graph=(ref["rowptr"], ref["colind"]))
    text = dict(funcs)
    text["source uy"] = "sin(x)*sin(2*y)" + ("*sin(0.5*z)" if dim == 3 else "")
    text["thermal source"] = "3*sin(2*x)*sin(y)" + ("*sin(1.5*z)" if dim == 3 else "")
    text["density"] = "1.3+0*x"
    configure(blk, text, params)
    check_all(run_gpu(blk, m, u, tr, len(ref["colind"]), local=True), ref)


def _untouched_after(call, ndof, nnz):
    torch = _torch()
    import mrhyde_amd
    res = torch.full((ndof,), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((nnz,), -3.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        call(res, vals)
    torch.cuda.synchronize()
    assert ei.value.code == 1, ei.value  # MHA_ERR_INVALID
    assert bool((res == 7.0).all()) and bool((vals == -3.0).all())
    return str(ei.value)


def test_3d_q2_shape_is_refused_and_nothing_is_written(oracle):
    """3-D Q2/Q1/Q2 at 27 points: 116 dofs, 20 slots -- the per-element arrays alone need 177 KB of the 160 KB of LDS.
    The launcher's LDS check refuses the shape before anything is written (running it in chunks of points is not built)."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(57)
    m = R.coupled_mesh(oracle, 3, (2, 1, 1), (2, 1, 2))
    assert m["lids"].shape[1] == 116
    blk = make_block(m, PHYS, 4)
    configure(blk, funcs_for(3), dict(beta=0.7))
    rowptr, colind = blk.get_graph()
    ud = torch.tensor(rng.uniform(-1, 1, m["ndof"]), device="cuda")
    for kw in (dict(path=mrhyde_amd.PATH_POINT_ENGINE), dict(path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True),
               dict(path=mrhyde_amd.PATH_LOCAL_THEN_SCATTER), dict(path=mrhyde_amd.PATH_ROW_GATHER, compute_jacobian=False)):
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, **kw), m["ndof"], len(colind))
        assert "of LDS" in msg
    E, n = m["lids"].shape
    lJ = torch.full((E, n, n), 5.0, dtype=torch.float64, device="cuda")
    lr = torch.full((E, n), 5.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        blk.compute_local_jacres(ud, lJ, lr)
    assert ei.value.code == 1
    torch.cuda.synchronize()
    assert bool((lJ == 5.0).all()) and bool((lr == 5.0).all())


def test_thermal_boundary_groups_and_field_reading_strings_are_refused(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(58)
    dim, ncell, orders, qdeg = 2, (4, 3), (1, 1, 1), 2
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    blk = make_block(m, PHYS, qdeg)
    configure(blk, funcs_for(dim), dict(beta=0.7))
    rowptr, colind = blk.get_graph()
    ud = torch.tensor(rng.uniform(-1, 1, m["ndof"]), device="cuda")
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    for bc in (mrhyde_amd.BC_NEUMANN, mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            blk.add_boundary_group("left", bc, be, bs)
        assert ei.value.code == 1 and "not built for the coupled block" in str(ei.value)
    assert blk.num_boundary_groups() == 0
    # the generic Flux condition works per variable, on e and on a velocity
    nd, nnz = m["ndof"], len(colind)
    blk.set_function("Flux e left", 2.5)
    blk.add_flux_group("left", "e", be, bs)
    res = torch.zeros(nd, dtype=torch.float64, device="cuda")
    blk.assemble_boundary(ud, res, None, compute_jacobian=False)
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    touched = np.flatnonzero(r)
    assert len(touched) > 0 and set(touched) <= set(R.var_rows(m, dim + 1))
    # a deck string that reads a solution field: refused at launch, outputs untouched
    blk.set_function("thermal diffusion", "1+e*e")
    msg = _untouched_after(lambda r_, v_: blk.assemble_jacres(ud, r_, v_, path=mrhyde_amd.PATH_POINT_ENGINE), nd, nnz)
    assert "thermal module" in msg
    _untouched_after(lambda r_, v_: blk.assemble_jacres(ud, r_, v_, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True), nd, nnz)
    # the wrong variable list is refused with the order in the message
    H = oracle.HGRAD
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=2, physics=PHYS, variables=[(H, 1)] * 3)
    assert ei.value.code == 1 and "ux, pr, uy, e" in str(ei.value)
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(3, quadrature=2, physics=PHYS, variables=[(H, 1)] * 4)
    assert "ux, pr, uy, uz, e" in str(ei.value)


def test_midsize_128_squared_transient_supg_pspg(oracle):
    """2-D 128 x 128, Q2/Q1/Q2, transient with SUPG + PSPG: the element arrays of a strided sample of 1 024 elements
    against the restatement evaluated on those elements only, the row-gather CRS against the scatter of the GPU's own
    element arrays, and the assembled matrix against a central difference of the assembled residual (step and bound of
    tests/test_full_size_gpu.py)."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(59)
    dim, orders, qdeg = 2, (2, 1, 2), 4
    m = R.coupled_mesh(oracle, dim, (128, 128), orders)
    nd = m["ndof"]
    u = rng.uniform(-1, 1, nd)
    tr = R.transient_state(rng, nd)
    fixed = fixed_rows(m)
    funcs, params = funcs_for(dim), dict(useSUPG=1, usePSPG=1, beta=0.7, T_ambient=0.3)
    blk = make_block(m, PHYS, qdeg, fixed=fixed)
    configure(blk, funcs, params)
    rowptr, colind = blk.get_graph()
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    E, n = m["lids"].shape
    lJ = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
    lr = torch.zeros((E, n), dtype=torch.float64, device="cuda")
    blk.compute_local_jacres(ud, lJ, lr, **kw)
    sample = np.arange(5, E, 16)
    assert len(sample) >= 1000
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, params=params, transient=tr, elems=sample)
    lJh, lrh = lJ.cpu().numpy(), lr.cpu().numpy()
    eJ, er = rel_err(lJh[sample], ref["local_J"]), rel_err(lrh[sample], ref["local_res"])
    print("sample local_J", eJ, "local_res", er)
    assert eJ < RTOL and er < RTOL
    res = torch.full((nd,), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((len(colind),), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    torch.cuda.synchronize()
    # every row: the reference scatter of the element arrays the sample has just pinned
    glob = R.scatter(m, -lrh, lJh, m["lids"], fixed, rowptr, colind)
    del lJh
    e1, e2 = rel_err(res.cpu().numpy(), glob["res"]), crs_err(vals.cpu().numpy(), glob)
    print("global res", e1, "crs", e2)
    assert e1 < RTOL and e2 < RTOL
    # directional derivative of the whole residual against the assembled matrix
    dlt = rng.uniform(-1, 1, nd)
    eps = 1e-5
    rp_, rm_ = torch.zeros_like(res), torch.zeros_like(res)
    blk.assemble_jacres(torch.tensor(u + eps * dlt, device="cuda"), rp_, None, compute_jacobian=False,
                        path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    blk.assemble_jacres(torch.tensor(u - eps * dlt, device="cuda"), rm_, None, compute_jacobian=False,
                        path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    torch.cuda.synchronize()
    Jd = sp.csr_matrix((vals.cpu().numpy(), colind, rowptr), shape=(nd, nd)) @ dlt
    fd = -(rp_ - rm_).cpu().numpy() / (2 * eps)  # the vector holds -res.val()
    e3 = np.abs(fd - Jd).max() / np.abs(Jd).max()
    print("directional derivative", e3)
    assert e3 < 1e-7
