"""GPU tests of the cdr module ("cdr", MHA_PHYSICS_CDR) and of the coupled navierstokes + cdr block ("navierstokes+cdr",
MHA_PHYSICS_NAVIERSTOKES_CDR): every case through the C ABI via mrhyde_amd.Block, against the restatement in
tests/cdr_ref.py (which tests/test_cdr.py pins against the reference's golds and the CPU oracle).

Shapes: the smallest at which each instantiation family of the point engine is reached -- 2-D Q1 3x2 (eight elements per
workgroup, compile-time point count), 2-D Q2 3x2, 3-D Q1 2x3x2, 3-D Q2 2x2x2 (the large-element form); the meshes are
warped, so no element is affine.  Tolerances: RTOL = 1e-12 on residuals relative to the array's largest entry and, per
CRS entry, 1e-12 max(|ref|, 1e-3 rowmax) (cdr_ref.crs_err); golds as "%.6g" strings."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cdr_ref as R
from cdr_ref import RTOL, crs_err, rel_err

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
SHAPES = [(2, (3, 2), 1, 2), (2, (3, 2), 2, 4), (3, (2, 3, 2), 1, 2), (3, (2, 2, 2), 2, 4)]
COUPLED = [(2, (3, 2), (1, 1, 1), 2), (2, (3, 2), (2, 1, 2), 4), (2, (3, 2), (2, 1, 1), 4), (3, (2, 2, 2), (1, 1, 1), 2)]
# the function sets: constants and a closed form; deck strings in the coordinates; deck strings that read the fields,
# one of them through another named function ("kappa0")
FUNC_SETS = {
    "constants": lambda dim: {"source": ("sinprod", 2.0, [1.0, 2.0, 1.5][:dim]), "diffusion": 0.9, "specific heat": 1.4,
                              "density": 1.3, "reaction": 0.6, "xvel": 0.7, "yvel": -1.1, "zvel": 0.4},
    "coordinates": lambda dim: {"source": "2*sin(x)*sin(2*y)", "diffusion": "0.9+0.1*x*y", "specific heat": 1.4,
                                "density": "1.3+0*x", "reaction": "0.6*x", "xvel": "0.7-y", "yvel": "x*x",
                                "zvel": "0.4+x" + ("+z" if dim == 3 else "")},
    "fields": lambda dim: {"source": "2*sin(x)*sin(2*y)", "reaction": "0.5*c*c + 0.1*grad(c)[x]^2", "diffusion": "kappa0+c*c",
                           "kappa0": "1+0.1*x", "xvel": "c", "yvel": "0.3*c_t" if dim == 2 else "0.3+grad(c)[z]",
                           "density": 1.3},
}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def fmt(x):
    return "%.6g" % x


def make_block(m, physics, qdeg, fixed=None, graph=None, workset_size=100):
    import mrhyde_amd
    blk = mrhyde_amd.Block(m["dim"], quadrature=qdeg, physics=physics, workset_size=workset_size,
                           variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], fixed)
    blk.set_orientation(m["orient"])
    blk.set_graph(*graph) if graph is not None else blk.set_graph()
    return blk


def configure(blk, funcs, params=None):
    torch = _torch()
    for k, v in funcs.items():
        if isinstance(v, tuple) and v[0] == "array":
            v = torch.tensor(np.ascontiguousarray(v[1]), device="cuda")
        blk.set_function(k, v)
    for k, v in (params or {}).items():
        blk.set_physics_parameter(k, v)


def time_kw(blk, tr):
    torch = _torch()
    if tr is None:
        blk.set_time_integration(False)
        return {}
    ns, nst = tr["u_prev"].shape[1], tr["u_stage"].shape[1]
    blk.set_time_integration(True, ns, nst, tr["stage"], tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
    return dict(u_prev=torch.tensor(tr["u_prev"], device="cuda"), u_stage=torch.tensor(tr["u_stage"], device="cuda"))


def run_paths(blk, m, u, tr, ref):
    """The atomic, two-step and row-gather paths; overwrite onto garbage, accumulate, residual-only.  Each against ref."""
    torch = _torch()
    import mrhyde_amd
    kw = time_kw(blk, tr)
    nnz = len(ref["colind"])
    ud = torch.tensor(u, device="cuda")
    out = {}
    for name, path in (("atomic", mrhyde_amd.PATH_POINT_ENGINE), ("two-step", mrhyde_amd.PATH_LOCAL_THEN_SCATTER)):
        res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(nnz, dtype=torch.float64, device="cuda")
        blk.assemble_jacres(ud, res, vals, path=path, **kw)
        out[name] = (res.cpu().numpy(), vals.cpu().numpy())
    res3, vals3 = torch.full((m["ndof"],), 7.0, dtype=torch.float64, device="cuda"), torch.full((nnz,), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res3, vals3, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
    r3, v3 = res3.cpu().numpy().copy(), vals3.cpu().numpy().copy()
    out["row-gather"] = (r3, v3)
    blk.assemble_jacres(ud, res3, vals3, path=mrhyde_amd.PATH_ROW_GATHER, **kw)  # accumulates on top
    assert rel_err(res3.cpu().numpy(), 2 * r3) < 1e-14 and rel_err(vals3.cpu().numpy(), 2 * v3) < 1e-14
    blk.assemble_jacres(ud, res3, vals3, path=mrhyde_amd.PATH_ROW_GATHER, compute_jacobian=False, overwrite=True, **kw)
    assert rel_err(res3.cpu().numpy(), r3) < 1e-14 and rel_err(vals3.cpu().numpy(), 2 * v3) < 1e-14  # matrix left alone
    res4, vals4 = torch.full_like(res3, 1.0), torch.full_like(vals3, 2.0)
    blk.assemble_jacres(ud, res4, vals4, overwrite=True, **kw)  # AUTO takes the row gather on these blocks
    assert blk.info("last_path") == mrhyde_amd.PATH_ROW_GATHER
    assert rel_err(res4.cpu().numpy(), r3) < 1e-14 and rel_err(vals4.cpu().numpy(), v3) < 1e-14
    torch.cuda.synchronize()
    for name, (r, v) in out.items():
        er, ev = rel_err(r, ref["res"]), crs_err(v, ref)
        print(name, "res", er, "crs", ev)
        assert er < RTOL and ev < RTOL, name
    return out


def _cdr_case(oracle, dim, ncell, order, seed, transient):
    rng = np.random.default_rng(seed)
    m = R.cdr_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    fixed = ((m["side_mask"] & 0b0011) != 0).astype(np.uint8)
    return rng, m, u, tr, fixed


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("fset", list(FUNC_SETS))
@pytest.mark.parametrize("transient", [False, True])
def test_cdr_matches_the_yardstick(oracle, dim, ncell, order, qdeg, fset, transient):
    rng, m, u, tr, fixed = _cdr_case(oracle, dim, ncell, order, 61, transient)
    funcs = FUNC_SETS[fset](dim)
    if dim == 2:
        funcs.pop("zvel", None)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    blk = make_block(m, "cdr", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    configure(blk, funcs)
    out = run_paths(blk, m, u, tr, ref)
    r3, v3 = out["row-gather"]
    for r in np.flatnonzero(fixed)[:30]:  # fixed rows: nothing written but the overwrite's zeros
        assert r3[r] == 0.0 and np.all(v3[ref["rowptr"][r]:ref["rowptr"][r + 1]] == 0.0)


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
def test_defaults_are_the_reference_defaults(oracle, dim, ncell, order, qdeg):
    """No function set: reaction 1 and velocities 1 (cdr.cpp:40-48), not thermal's zeros."""
    rng, m, u, tr, fixed = _cdr_case(oracle, dim, ncell, order, 62, True)
    ref = R.assemble(oracle, m, qdeg, u, fixed=fixed, transient=tr)
    zero = R.assemble(oracle, m, qdeg, u, funcs=dict(reaction=0.0, xvel=0.0, yvel=0.0, zvel=0.0), fixed=fixed, transient=tr)
    assert rel_err(zero["res"], ref["res"]) > 1e-3 and rel_err(zero["crs_vals"], ref["crs_vals"]) > 1e-3
    blk = make_block(m, "cdr", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    run_paths(blk, m, u, tr, ref)
    blk.set_function("SUPG tau", 3.0)  # accepted, and as in the reference read by no term
    run_paths(blk, m, u, tr, ref)


@pytest.mark.parametrize("dim,ncell,order,qdeg", SHAPES)
@pytest.mark.parametrize("transient", [False, True])
def test_cdr_equals_thermal_with_advection_on_the_device(oracle, dim, ncell, order, qdeg, transient):
    """Two modules that share no point function: reaction 0, density = specific heat = 1, b = the velocity."""
    torch = _torch()
    import mrhyde_amd
    rng, m, u, tr, fixed = _cdr_case(oracle, dim, ncell, order, 63, transient)
    b = [0.7, -1.1, 0.4][:dim]
    src = ("sinprod", 2.0, [1.0, 2.0, 1.5][:dim])
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    got = {}
    for phys, funcs, params in (("cdr", dict(zip(["xvel", "yvel", "zvel"], b), diffusion=0.9, reaction=0.0, source=src), {}),
                                ("thermal", dict(zip(["bx", "by", "bz"], b), **{"thermal diffusion": 0.9, "thermal source": src}),
                                 {"include advection": 1})):
        blk = make_block(m, phys, qdeg, fixed=fixed, graph=(rowptr, colind))
        configure(blk, funcs, params)
        kw = time_kw(blk, tr)
        res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
        got[phys] = (res.cpu().numpy(), vals.cpu().numpy())
    assert rel_err(got["cdr"][0], got["thermal"][0]) < RTOL
    assert crs_err(got["cdr"][1], dict(crs_vals=got["thermal"][1], rowptr=rowptr)) < RTOL


@pytest.mark.parametrize("adjoint,lump", [(True, False), (False, True), (True, True)])
def test_scatter_options_on_cdr(oracle, adjoint, lump):
    """isAdjoint_ / lump_mass_ of the reference's scatter (assemblyManager.cpp:4124-4133), as the other engine blocks
    check them: from the yardstick's element arrays."""
    torch = _torch()
    import mrhyde_amd
    dim, ncell, order, qdeg = 2, (3, 2), 2, 4
    rng, m, u, tr, fixed = _cdr_case(oracle, dim, ncell, order, 68, True)
    funcs = FUNC_SETS["fields"](dim)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr)
    _, Jloc, _ = R.cdr_row(oracle, m, qdeg, u, funcs=funcs, transient=tr)
    rowptr, colind = ref["rowptr"], ref["colind"]
    expect = np.zeros(len(colind))
    n = m["lids"].shape[1]
    for e, L in enumerate(m["lids"]):
        for i in range(n):
            r = L[i]
            if fixed[r]:
                continue
            lo, hi = rowptr[r], rowptr[r + 1]
            for j in range(n):
                v = Jloc[e][i, i] if adjoint else Jloc[e][i, j]
                c = r if lump else L[j]
                expect[lo + np.searchsorted(colind[lo:hi], c)] += v
    blk = make_block(m, "cdr", qdeg, fixed=fixed, graph=(rowptr, colind))
    configure(blk, funcs)
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.full((len(colind),), 9.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, overwrite=True, adjoint=adjoint, lump_mass=lump,
                        **time_kw(blk, tr))
    torch.cuda.synchronize()
    assert blk.info("last_path") == mrhyde_amd.PATH_ROW_GATHER
    scale = np.abs(ref["crs_vals"]).max()
    got = vals.cpu().numpy()
    assert np.abs(expect).max() > 1e-3 * scale and np.abs(got - expect).max() / scale < RTOL
    assert rel_err(res.cpu().numpy(), ref["res"]) < RTOL


def coupled_fixed(m):
    """strong-Dirichlet rows on two sides: the velocities and c, not the pressure"""
    return (((m["side_mask"] & 0b1100) != 0) & (m["dof_var"] != 1)).astype(np.uint8)


def coupled_funcs(dim, constant_velocity=False):
    f = {"source ux": 0.3, "source uy": ("sinprod", 1.0, [1.0, 2.0, 0.5][:dim]), "viscosity": 0.05, "density": 1.3,
         "source": ("sinprod", 3.0, [2.0, 1.0, 1.5][:dim]), "diffusion": 0.4, "specific heat": 1.4, "reaction": "0.5*c*c",
         "xvel": "ux", "yvel": "uy"}
    if dim == 3:
        f.update({"source uz": -0.2, "zvel": "uz"})
    if constant_velocity:
        f.update(dict(zip(["xvel", "yvel", "zvel"][:dim], [0.4, -0.2, 0.1])))
    return f


@pytest.mark.parametrize("dim,ncell,orders,qdeg", COUPLED)
@pytest.mark.parametrize("transient", [False, True])
def test_coupled_block_matches_the_yardstick(oracle, dim, ncell, orders, qdeg, transient):
    rng = np.random.default_rng(64)
    m = R.coupled_mesh(oracle, dim, ncell, orders)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    fixed = coupled_fixed(m)
    params = dict(useSUPG=1, usePSPG=1)
    crows = R.var_rows(m, dim + 1)
    free_c = np.array([r for r in crows if not fixed[r]])
    for const in (False, True):
        funcs = coupled_funcs(dim, const)
        ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, ns_params=(1, 1, 0), fixed=fixed, transient=tr)
        blk = make_block(m, "navierstokes+cdr", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
        configure(blk, funcs, params)
        out = run_paths(blk, m, u, tr, ref)
        J = sp.csr_matrix((out["atomic"][1], ref["colind"], ref["rowptr"]), shape=(m["ndof"],) * 2).tocsr()
        Jr = R.dense(ref, m["ndof"]).tocsr()
        for v in [0, 2, 3][:dim]:
            blockmax = abs(J[free_c][:, R.var_rows(m, v)]).max()
            if const:  # constant velocities: the coupling entries are exactly zero
                assert blockmax == 0.0
            else:      # the derivative of xvel: 'ux' ...: there, and compared like every other entry above
                assert blockmax > 0.0 and abs(Jr[free_c][:, R.var_rows(m, v)]).max() > 0.0
        assert abs(J[free_c][:, R.var_rows(m, 1)]).max() == 0.0
        # the navierstokes rows equal those of a plain navierstokes block on the same cells
        ns, rows = R.N.sub_mesh(oracle, m, list(range(dim + 1)))
        g = oracle.build_graph(ns["ndof"], ns["lids"])
        nb = make_block(ns, "navierstokes", qdeg, fixed=fixed[rows], graph=g)
        configure(nb, {k: v for k, v in funcs.items() if k in R.NS_FUNC_NAMES}, params)
        trs = None if tr is None else dict(tr, u_prev=tr["u_prev"][rows], u_stage=tr["u_stage"][rows])
        torch = _torch()
        import mrhyde_amd
        kw = time_kw(nb, trs)
        res = torch.zeros(ns["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(g[1]), dtype=torch.float64, device="cuda")
        nb.assemble_jacres(torch.tensor(u[rows], device="cuda"), res, vals, path=mrhyde_amd.PATH_POINT_ENGINE, **kw)
        Js = J[rows][:, rows].tocsr()
        Js.sort_indices()
        assert np.array_equal(Js.indptr, g[0]) and np.array_equal(Js.indices, g[1])
        assert rel_err(out["atomic"][0][rows], res.cpu().numpy()) < RTOL
        assert crs_err(Js.data, dict(crs_vals=vals.cpu().numpy(), rowptr=g[0])) < RTOL
        assert abs(J[rows][:, crows]).max() == 0.0  # no c columns in the navierstokes rows


def _device_assembler(oracle, physics, params=None):
    """assemble_fn of the gold drivers in cdr_ref: device assembly (row gather, overwrite), host matrix."""
    torch = _torch()
    import mrhyde_amd
    state = {}

    def assemble(m, u, funcs, fixed, tr):
        if "blk" not in state:
            g = oracle.build_graph(m["ndof"], m["lids"])
            blk = make_block(m, physics, 2, fixed=fixed, graph=g)
            configure(blk, funcs, params)
            state.update(blk=blk, g=g)
        blk, (rowptr, colind) = state["blk"], state["g"]
        kw = time_kw(blk, tr)
        res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True, **kw)
        v = vals.cpu().numpy()
        oracle.apply_dbc_diag(fixed, rowptr, colind, v)
        return sp.csr_matrix((v, colind, rowptr), shape=(m["ndof"],) * 2), res.cpu().numpy()
    return assemble, state


def test_gold_2d_manufactured_on_the_device(oracle):
    fn, _ = _device_assembler(oracle, "cdr")
    got = R.gold_manufactured(oracle, fn)
    g = [float(v) for v in re.findall(r"error for c = ([-0-9.e]+)", open(os.path.join(GOLD, "cdr_2D_manufactured.gold")).read())]
    assert [fmt(v) for v in got] == [fmt(v) for v in g] == ["0.00101714"], (got, g)


def test_gold_2d_transient_on_the_device(oracle):
    torch = _torch()
    fn, state = _device_assembler(oracle, "cdr")

    def initial(m):
        """set_initial with c: 'exp(bubble)': the consistent mass and (initial c, basis) from the device, host solve"""
        fixed = (m["side_mask"] != 0).astype(np.uint8)
        g = oracle.build_graph(m["ndof"], m["lids"])
        blk = make_block(m, "cdr", 2, fixed=fixed, graph=g)
        blk.set_function("bubble", R.BUBBLE_T)
        blk.set_function("initial c", "exp(bubble)")
        rhs = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(g[1]), dtype=torch.float64, device="cuda")
        blk.set_initial(rhs, vals)
        import scipy.sparse.linalg as spla
        M = sp.csr_matrix((vals.cpu().numpy(), g[1], g[0]), shape=(m["ndof"],) * 2)
        return spla.spsolve(M.tocsc(), rhs.cpu().numpy())

    got = R.gold_transient(oracle, fn, initial=initial)
    g = [float(v) for v in re.findall(r"error for c = ([-0-9.e]+)", open(os.path.join(GOLD, "cdr_2D_transient.gold")).read())]
    assert len(g) == 11 and [fmt(v) for v in got] == [fmt(v) for v in g], (got, g)


def test_gold_2d_ns_coupled_on_the_device(oracle):
    fn, _ = _device_assembler(oracle, "navierstokes+cdr", dict(usePSPG=1))
    got = R.gold_ns_coupled(oracle, fn)
    txt = open(os.path.join(GOLD, "cdr_2D_ns_coupled.gold")).read()
    g = {k: float(v) for k, v in re.findall(r"L2 norm of the error for (\w+) = ([-0-9.e]+)", txt)}
    assert sorted(g) == ["c", "pr", "ux", "uy"]
    for k in g:
        assert fmt(got[k]) == fmt(g[k]), (k, got[k], g[k])


def test_views_mass_flux_on_both_blocks(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(65)
    # cdr: the solution fields of the workset, the mass, computeFlux = zeros
    dim, ncell, order, qdeg = 2, (3, 3), 2, 4
    m = R.cdr_mesh(oracle, dim, ncell, order)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"])
    funcs = FUNC_SETS["fields"](dim)
    funcs.pop("zvel", None)
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, transient=tr)
    F = ref["fields"]
    blk = make_block(m, "cdr", qdeg, graph=(ref["rowptr"], ref["colind"]), workset_size=4)
    configure(blk, funcs)
    kw = time_kw(blk, tr)
    ud = torch.tensor(u, device="cuda")
    for w in range(blk.num_worksets()):
        e0, e1 = 4 * w, min(4 * w + 4, m["nelem"])
        blk.workset_update(w)
        blk.workset_compute_solution(ud, kw["u_prev"], kw["u_stage"])
        assert rel_err(blk.workset_view_numpy("c"), F["val"][0].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("c_t"), F["dot"][0].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("grad(c)[x]"), F["grad"][0][0].val[e0:e1]) < RTOL
        assert rel_err(blk.workset_view_numpy("grad(c)[y]"), F["grad"][0][1].val[e0:e1]) < RTOL
    E, n = m["lids"].shape
    mass = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
    blk.get_mass(mass, None)
    torch.cuda.synchronize()
    assert rel_err(mass.cpu().numpy(), oracle.get_mass(m, qdeg, None)) < RTOL
    be, bs = oracle.boundary_sides(dim, ncell, "left")
    gid = blk.add_boundary_group("left", mrhyde_amd.BC_NEUMANN, be, bs)
    nqs = oracle.side_sizes(dim, qdeg)[1]
    flux = torch.full((len(be), nqs), 4.0, dtype=torch.float64, device="cuda")
    dfl = torch.full((len(be), nqs, n), 4.0, dtype=torch.float64, device="cuda")
    blk.compute_flux(gid, ud, flux, dfl, **kw)
    torch.cuda.synchronize()
    assert bool((flux == 0.0).all()) and bool((dfl == 0.0).all())
    # boundary groups on a cdr block add nothing (cdr::boundaryResidual is empty in the reference)
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(ref["colind"]), dtype=torch.float64, device="cuda")
    blk.assemble_boundary(ud, res, vals, **kw)
    torch.cuda.synchronize()
    assert bool((res == 0.0).all()) and bool((vals == 0.0).all())
    # coupled block: the mass of every variable and the generic Flux condition on c
    dim, ncell, orders, qdeg = 2, (3, 2), (2, 1, 2), 4
    mc = R.coupled_mesh(oracle, dim, ncell, orders)
    fixed = coupled_fixed(mc)
    cb = make_block(mc, "navierstokes+cdr", qdeg, fixed=fixed)
    E, n = mc["lids"].shape
    wts = [1.0, 0.0, 1.3, 2.1]
    for w in (None, wts):
        mass = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
        cb.get_mass(mass, w)
        torch.cuda.synchronize()
        assert rel_err(mass.cpu().numpy(), oracle.get_mass(mc, qdeg, w)) < RTOL
    te, ts = oracle.boundary_sides(dim, ncell, "left")
    sb = oracle.physical_side_basis(dim, orders[2], qdeg, mc["nodes"], te, ts)
    x, y, nx, ny = sb["ip"][..., 0], sb["ip"][..., 1], sb["normals"][..., 0], sb["normals"][..., 1]
    fl = 1.5 + x * nx - 2 * y * ny + 0.5 * np.sin(3 * x + y)
    off = mc["offsets"][mc["varptr"][dim + 1]:mc["varptr"][dim + 2]]
    want = np.zeros(mc["ndof"])
    oracle.flux_condition(te, mc["lids"], off, fl, sb["wts"], sb["basis"][..., None], want, fixed=fixed)
    cb.set_function("Flux c left", "1.5 + x*nx - 2*y*ny + 0.5*sin(3*x+y)")
    cb.add_flux_group("left", "c", te, ts)
    res = torch.zeros(mc["ndof"], dtype=torch.float64, device="cuda")
    cb.assemble_boundary(torch.tensor(rng.uniform(-1, 1, mc["ndof"]), device="cuda"), res, None, compute_jacobian=False)
    torch.cuda.synchronize()
    assert np.abs(want).max() > 0 and rel_err(res.cpu().numpy(), want) < RTOL


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


def test_refusals(oracle):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(66)
    H = oracle.HGRAD
    # field-reading functions stay refused, with the old message, on the modules that have no such instantiation
    for phys, mesh, fname in (("navierstokes", oracle.mesh_multi(2, (3, 2), [H] * 3, [1, 1, 1]), "viscosity"),
                              ("linearelasticity", oracle.mesh_multi(2, (3, 2), [H] * 2, [1, 1]), "mu"),
                              ("porousMixed", oracle.mesh_multi(2, (3, 2), [oracle.HVOL, oracle.HDIV], [0, 1]), "total_mobility")):
        blk = make_block(mesh, phys, 2)
        var0 = {"navierstokes": "ux", "linearelasticity": "dx", "porousMixed": "p"}[phys]
        blk.set_function(fname, "1+%s*%s" % (var0, var0))
        _, colind = blk.get_graph()
        ud = torch.tensor(rng.uniform(-1, 1, mesh["ndof"]), device="cuda")
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, path=mrhyde_amd.PATH_POINT_ENGINE), mesh["ndof"], len(colind))
        assert "functions of the solution fields are built for the thermal module" in msg, (phys, msg)
    # coupled block: a navierstokes function that reads a field, by name
    m = R.coupled_mesh(oracle, 2, (3, 2), (1, 1, 1))
    blk = make_block(m, "navierstokes+cdr", 2)
    _, colind = blk.get_graph()
    nd, nnz = m["ndof"], len(colind)
    ud = torch.tensor(rng.uniform(-1, 1, nd), device="cuda")
    blk.set_function("viscosity", "0.05+c*c")
    msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, path=mrhyde_amd.PATH_POINT_ENGINE), nd, nnz)
    assert "'viscosity' reads solution fields" in msg
    blk.set_function("viscosity", 0.05)
    # boundary groups of the modules and computeFlux on the coupled block
    be, bs = oracle.boundary_sides(2, (3, 2), "left")
    for bc in (mrhyde_amd.BC_NEUMANN, mrhyde_amd.BC_WEAK_DIRICHLET, mrhyde_amd.BC_INTERFACE):
        with pytest.raises(mrhyde_amd.MhaError) as ei:
            blk.add_boundary_group("left", bc, be, bs)
        assert ei.value.code == 1 and "not built for the coupled block" in str(ei.value)
    # the row-owner path and the deterministic mode on cdr: refused by name, not by accident
    mc = R.cdr_mesh(oracle, 2, (3, 2), 1)
    cb = make_block(mc, "cdr", 2)
    _, cc = cb.get_graph()
    uc = torch.tensor(rng.uniform(-1, 1, mc["ndof"]), device="cuda")
    msg = _untouched_after(lambda r, v: cb.assemble_jacres(uc, r, v, path=2), mc["ndof"], len(cc))  # MHA_PATH_ROW_OWNER
    assert "assembly path 2 is not available for this physics module" in msg
    msg = _untouched_after(lambda r, v: cb.assemble_jacres(uc, r, v, deterministic=True), mc["ndof"], len(cc))
    assert "MHA_ASSEMBLE_DETERMINISTIC" in msg
    # an unknown identifier in a cdr string
    cb.set_function("reaction", "0.5*c*q7")
    msg = _untouched_after(lambda r, v: cb.assemble_jacres(uc, r, v), mc["ndof"], len(cc))
    assert "q7" in msg
    # wrong variable lists, with the order in the message
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=2, physics="cdr", variables=[(H, 1)] * 2)
    assert ei.value.code == 1 and "one HGRAD variable (c)" in str(ei.value)
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=2, physics="cdr", variables=[(oracle.HVOL, 0)])
    assert ei.value.code == 1
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(2, quadrature=2, physics="navierstokes+cdr", variables=[(H, 1)] * 3)
    assert ei.value.code == 1 and "ux, pr, uy, c" in str(ei.value)
    with pytest.raises(mrhyde_amd.MhaError) as ei:
        mrhyde_amd.Block(3, quadrature=2, physics="navierstokes+cdr", variables=[(H, 1)] * 4)
    assert "ux, pr, uy, uz, c" in str(ei.value)


def test_3d_q2_coupled_shape_is_refused_and_nothing_is_written(oracle):
    """3-D Q2/Q1/Q2/Q2/Q2 at 27 points: the per-element arrays exceed the LDS; the launcher's message covers it."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(67)
    m = R.coupled_mesh(oracle, 3, (2, 1, 1), (2, 1, 2))
    assert m["lids"].shape[1] == 116
    blk = make_block(m, "navierstokes+cdr", 4)
    _, colind = blk.get_graph()
    ud = torch.tensor(rng.uniform(-1, 1, m["ndof"]), device="cuda")
    for kw in (dict(path=mrhyde_amd.PATH_POINT_ENGINE), dict(path=mrhyde_amd.PATH_ROW_GATHER, overwrite=True)):
        msg = _untouched_after(lambda r, v: blk.assemble_jacres(ud, r, v, **kw), m["ndof"], len(colind))
        assert "of LDS" in msg
