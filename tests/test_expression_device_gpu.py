"""GPU tests of the two device deck-string interpreters (kernels/device_math.hpp: eval_expression on doubles,
eval_expression_dual on value + one directional derivative), operator by operator: every entry of the table in
tests/expression_cases.py through the C ABI against the yardsticks that tests/test_expression.py pins against mpmath
(cdr_ref.assemble / oracle_lib.deck_eval_ad for strings that may read the fields, the C oracle for the thermal kernels).

Shapes: the smallest that reach each instantiation, as tests/test_cdr_gpu.py states them -- cdr 2-D Q1 3x2, 3-D Q1 2x3x2,
and for the Dual sweep 2-D Q2 3x2 (the other engine form); warped meshes.  One block per shape is reused across the
table, which also exercises the recompile and re-upload of the programs when a function is replaced.
Tolerances: the project's own, RTOL = 1e-12 through rel_err and crs_err; 1e-14 between the two interpreters on the same
coordinate string.  A sweep collects the entries that miss and reports them together."""
import numpy as np
import pytest

import cdr_ref as R
import expression_cases as X
from cdr_ref import RTOL, crs_err, rel_err
from test_cdr_gpu import _torch, configure, coupled_fixed, make_block, run_paths, time_kw

pytestmark = pytest.mark.gpu


def set_funcs(blk, funcs):
    for k, v in funcs.items():
        blk.set_function(k, v)


def assemble(blk, m, ud, kw, nnz, **opts):
    """One overwriting assembly onto garbage (MHA_PATH_AUTO unless opts says otherwise) -> (res, vals) as numpy."""
    torch = _torch()
    res = torch.full((m["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((nnz,), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, overwrite=True, **dict(kw, **opts))
    torch.cuda.synchronize()
    return res.cpu().numpy(), vals.cpu().numpy()


def sweep_block(oracle, shape, transient):
    torch = _torch()
    dim, ncell, order, qdeg = X.SHAPES[shape]
    m, u, tr, fixed = X.sweep_case(oracle, shape, transient)
    g = oracle.build_graph(m["ndof"], m["lids"])
    blk = make_block(m, "cdr", qdeg, fixed=fixed, graph=g)
    blk.set_time(X.TIME)
    return blk, m, torch.tensor(u, device="cuda"), time_kw(blk, tr), g


def against(ref, g, res, vals):
    assert np.array_equal(ref["rowptr"], g[0]) and np.array_equal(ref["colind"], g[1])
    return rel_err(res, ref["res"]), crs_err(vals, ref)


# ---- a. the opcode sweep ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["2d-q1", "3d-q1"])
@pytest.mark.parametrize("slot", ["source", "diffusion"])
def test_coordinate_strings_in_both_interpreters(oracle, shape, slot):
    """Every coordinate string with all other functions constant (EXPR = 1, the double interpreter), and again with
    reaction: '0*c', which forces the Dual instantiation (EXPR = 2) and contributes exact zeros: both against the same
    reference, and against each other to 1e-14.  The twelve-entry string of the stack limit runs here in both."""
    dim = X.SHAPES[shape][0]
    blk, m, ud, kw, g = sweep_block(oracle, shape, False)
    nnz, bad = len(g[1]), []
    for s, item, _ in X.entries(X.COORD, dim) + [(X.COORD_ALL, "all rules", None), (X.STACK12, "kExprStack entries", None)]:
        ref = X.sweep_reference(oracle, shape, s, slot)
        set_funcs(blk, X.sweep_funcs(dim, s, slot))
        r1, v1 = assemble(blk, m, ud, kw, nnz)
        blk.set_function("reaction", "0*c")
        r2, v2 = assemble(blk, m, ud, kw, nnz)
        figs = against(ref, g, r1, v1) + against(ref, g, r2, v2) + (rel_err(r2, r1), rel_err(v2, v1))
        print("%-40s double res %.1e crs %.1e | Dual res %.1e crs %.1e | between %.1e %.1e" % ((s[:40],) + figs))
        if not (max(figs[:4]) < RTOL and max(figs[4:]) < 1e-14):
            bad.append((s, item, figs))
    assert not bad, bad


@pytest.mark.parametrize("shape", list(X.SHAPES))
@pytest.mark.parametrize("transient", [False, True])
@pytest.mark.parametrize("slot", ["source", "diffusion"])
def test_field_strings_in_the_dual_interpreter(oracle, shape, transient, slot):
    """Every field string as `source` (the value slot is the function itself) and as `diffusion` (it meets
    fv[1] / (fv[3] * fv[2]) and the gradient slots); steady, and on cdr_ref.transient_state, where c_t and the
    alpha_u / alpha_t seeding matter.  The reference asserts that no integration point sits on a kink."""
    dim = X.SHAPES[shape][0]
    blk, m, ud, kw, g = sweep_block(oracle, shape, transient)
    nnz, bad = len(g[1]), []
    for s, item, _ in X.entries(X.FIELD, dim) + [(X.field_all("c", True), "all rules", None),
                                                 (X.STACK12_FIELD, "kExprStack entries", None)]:
        ref = X.sweep_reference(oracle, shape, s, slot, transient)
        set_funcs(blk, X.sweep_funcs(dim, s, slot))
        figs = against(ref, g, *assemble(blk, m, ud, kw, nnz))
        print("%-40s res %.1e crs %.1e" % ((s[:40],) + figs))
        if not max(figs) < RTOL:
            bad.append((s, item, figs))
    assert not bad, bad


def test_all_rules_string_through_every_path(oracle):
    """The field all-rules string as source and diffusion at once: the atomic, two-step and row-gather paths."""
    shape = "2d-q2"
    dim, ncell, order, qdeg = X.SHAPES[shape]
    m, u, tr, fixed = X.sweep_case(oracle, shape, True)
    funcs = X.sweep_funcs(dim, X.field_all("c", True), "source", {"diffusion": X.field_all("c", True)})
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr, time=X.TIME)
    blk = make_block(m, "cdr", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    blk.set_time(X.TIME)
    configure(blk, funcs)
    run_paths(blk, m, u, tr, ref)


# ---- b. the coupled block ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transient", [False, True])
def test_coupled_block_strings(oracle, transient):
    """navierstokes+cdr 2-D Q1/Q1/Q1: strings that read the other variables, and the all-rules string; 'source ux' is the
    coordinate all-rules string, which the EXPR = 2 kernel of this block runs through the double interpreter."""
    torch = _torch()
    rng = np.random.default_rng(X.SEED + 1)
    m = R.coupled_mesh(oracle, 2, (3, 2), (1, 1, 1))
    u = rng.uniform(-1, 1, m["ndof"])
    tr = R.transient_state(rng, m["ndof"]) if transient else None
    fixed = coupled_fixed(m)
    g = oracle.build_graph(m["ndof"], m["lids"])
    blk = make_block(m, "navierstokes+cdr", 2, fixed=fixed, graph=g)
    blk.set_time(X.TIME)
    configure(blk, {"viscosity": 0.05, "density": 1.3, "source ux": X.COORD_ALL}, dict(useSUPG=1, usePSPG=1))
    ud, kw, bad = torch.tensor(u, device="cuda"), time_kw(blk, tr), []
    for s, item, _ in X.COUPLED + [(X.field_all("c", True), "all rules", None)]:
        funcs = X.sweep_funcs(2, s, "source", {"viscosity": 0.05, "density": 1.3})
        ref = R.assemble(oracle, m, 2, u, funcs=dict(funcs, **{"source ux": ("expr", X.COORD_ALL, X.TIME)}), ns_params=(1, 1, 0),
                         fixed=fixed, transient=tr, rowptr=g[0], colind=g[1], time=X.TIME)
        set_funcs(blk, funcs)
        figs = against(ref, g, *assemble(blk, m, ud, kw, len(g[1])))
        print("%-40s res %.1e crs %.1e" % ((s[:40],) + figs))
        if not max(figs) < RTOL:
            bad.append((s, item, figs))
    assert not bad, bad


# ---- c. thermal -----------------------------------------------------------------------------------------------------------------

def _perturb(m, rng, amp=0.04):
    v = m["verts"].copy()
    inner = np.all((v > 1e-12) & (v < 1 - 1e-12), axis=1)
    v[inner] += amp * rng.uniform(-1, 1, (int(inner.sum()), v.shape[1]))
    m["verts"], m["nodes"] = v, np.ascontiguousarray(v[m["cell2vert"]])
    return m


def thermal_block(m, dim, order, qdeg, fixed, graph):
    import mrhyde_amd
    blk = mrhyde_amd.Block(dim, order, quadrature=qdeg)
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], fixed)
    blk.set_graph(*graph)
    blk.set_time(X.TIME)
    return blk


@pytest.mark.parametrize("dim,order,ncell", [(2, 2, (3, 2)), (3, 1, (2, 3, 2))])
def test_thermal_diffusion_all_rules_of_the_fields(oracle, dim, order, ncell):
    """'thermal diffusion' = the field all-rules string on e, as test_nonlinear_diffusion_deck_string runs "1+e*e"."""
    torch = _torch()
    import mrhyde_amd
    qdeg = 2 * order
    rng = np.random.default_rng(X.SEED + 2)
    m = _perturb(oracle.mesh_structured(dim, order, ncell), rng)
    u = rng.uniform(-1, 1, m["ndof"])
    fixed = m["boundary"]
    g = oracle.build_graph(m["ndof"], m["lids"])
    funcs = {"thermal source": "2*sin(pi*x)*y + 0.1*e", "thermal diffusion": X.field_all("e")}
    ref = oracle.assemble_thermal_fields(dim, order, qdeg, m["nodes"], m["lids"], m["offsets"], u, funcs, fixed=fixed,
                                         rowptr=g[0], colind=g[1], time=X.TIME)
    blk = thermal_block(m, dim, order, qdeg, fixed, g)
    set_funcs(blk, funcs)
    ud = torch.tensor(u, device="cuda")
    for path in (mrhyde_amd.PATH_AUTO, mrhyde_amd.PATH_POINT_ENGINE):
        res, vals = assemble(blk, m, ud, {}, len(g[1]), path=path)
        assert blk.info("last_path") in (mrhyde_amd.PATH_ROW_GATHER, mrhyde_amd.PATH_POINT_ENGINE)
        figs = (rel_err(res, ref["res"]), crs_err(vals, dict(ref, rowptr=g[0])))
        print("path", path, "res %.1e crs %.1e" % figs)
        assert max(figs) < RTOL


def test_thermal_dedicated_kernels_all_rules_of_the_coordinates(oracle):
    """The coordinate all-rules string through each dedicated kernel family with an EXPR instantiation: the general
    row-owner kernel (PATH_AUTO) and the element kernel (PATH_ELEMENT_ATOMIC) on a perturbed 3-D Q2 3x2x2 mesh, source and
    diffusion; the affine residual / row-owner pair on an unperturbed 2-D Q1 mesh, where the source is the one function
    evaluated per point."""
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(X.SEED + 3)
    s, t = X.COORD_ALL, X.TIME
    m = _perturb(oracle.mesh_multi(3, (3, 2, 2), [oracle.HGRAD], [2]), rng)
    u = rng.uniform(-1, 1, m["ndof"])
    ref = oracle.assemble_block(m, oracle.PHYS_THERMAL, 4, u, funcs={"thermal source": ("expr", s, t), "thermal diffusion": ("expr", s, t)})
    g = (ref["rowptr"], ref["colind"])
    blk = thermal_block(m, 3, 2, 4, None, g)
    set_funcs(blk, {"thermal source": s, "thermal diffusion": s})
    ud = torch.tensor(u, device="cuda")
    for path, want in ((mrhyde_amd.PATH_AUTO, mrhyde_amd.PATH_ROW_OWNER), (mrhyde_amd.PATH_ELEMENT_ATOMIC, mrhyde_amd.PATH_ELEMENT_ATOMIC)):
        res, vals = assemble(blk, m, ud, {}, len(g[1]), path=path)
        assert blk.info("last_path") == want
        figs = (rel_err(res, ref["res"]), crs_err(vals, ref))
        print("general, path", path, "res %.1e crs %.1e" % figs)
        assert max(figs) < RTOL
    ma = oracle.mesh_multi(2, (5, 4), [oracle.HGRAD], [1])
    ua = rng.uniform(-1, 1, ma["ndof"])
    refa = oracle.assemble_block(ma, oracle.PHYS_THERMAL, 2, ua, funcs={"thermal source": ("expr", s, t), "thermal diffusion": 1.7})
    ga = (refa["rowptr"], refa["colind"])
    ba = thermal_block(ma, 2, 1, 2, None, ga)
    set_funcs(ba, {"thermal source": s, "thermal diffusion": 1.7})
    uad = torch.tensor(ua, device="cuda")
    res, vals = assemble(ba, ma, uad, {}, len(ga[1]), path=mrhyde_amd.PATH_ROW_OWNER)
    assert ba.info("num_affine_elems") == ma["nelem"] and ba.info("last_path") == mrhyde_amd.PATH_ROW_OWNER
    assert ba.info("row_owner_kind") == 1
    figs = (rel_err(res, refa["res"]), crs_err(vals, refa))
    print("affine pair res %.1e crs %.1e" % figs)
    assert max(figs) < RTOL
    res, vals = assemble(ba, ma, uad, {}, len(ga[1]), path=mrhyde_amd.PATH_ROW_OWNER, compute_jacobian=False)
    assert rel_err(res, refa["res"]) < RTOL  # the residual kernel alone


# ---- d. the matrix-free products ----------------------------------------------------------------------------------------------

def test_matrix_free_products_with_the_all_rules_string(oracle):
    """apply_jacobian (forward, transposed), jacobian_diagonal and apply_jacobian_multi with K = 3 on cdr 2-D Q1 3x2 with
    the field all-rules string, by the criteria of tests/test_jacobian_apply_gpu.py and test_jacobian_diag_multi_gpu.py."""
    from test_jacobian_apply_gpu import check_products
    from test_jacobian_diag_multi_gpu import check_case
    shape = "2d-q1"
    dim, ncell, order, qdeg = X.SHAPES[shape]
    m, u, tr, fixed = X.sweep_case(oracle, shape, True)
    funcs = {"source": X.field_all("c", True), "diffusion": "0.5+0.1*c*c"}
    ref = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr, time=X.TIME)
    blk = make_block(m, "cdr", qdeg, fixed=fixed, graph=(ref["rowptr"], ref["colind"]))
    blk.set_time(X.TIME)
    configure(blk, funcs)
    check_products(blk, m, u, tr, fixed, ref, 301)
    check_case((blk, m, u, tr, fixed, ref), 302, (3,))


# ---- e. side kernels with the normals ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,ncell", [(3, (2, 2, 2)), (2, (3, 2))])
def test_side_data_with_normals(oracle, dim, ncell):
    """Thermal Neumann and weak-Dirichlet data as a deck string in the coordinates AND the unit normal (and h, 0) on a
    warped Q1 block: against the same formula in numpy at the oracle's side points and normals, handed to the oracle as
    per-point data."""
    torch = _torch()
    from test_boundary_gpu import SIDES2, SIDES3, warped
    order, qdeg = 1, 2
    s = X.SIDE_3D if dim == 3 else X.SIDE_2D
    m = warped(oracle, dim, order, ncell)
    rng = np.random.default_rng(X.SEED + 4)
    u = rng.uniform(-1, 1, m["ndof"])
    rowptr, colind = oracle.build_graph(m["ndof"], m["lids"])
    blk = thermal_block(m, dim, order, qdeg, None, (rowptr, colind))
    blk.set_function("thermal diffusion", 1.7)
    vals_ref, res_ref = np.zeros(rowptr[-1]), np.zeros(m["ndof"])
    for i, name in enumerate(SIDES3 if dim == 3 else SIDES2):
        bc = 1 if i < 2 else 2  # two Neumann sides, the others weak Dirichlet
        be, bs = oracle.boundary_sides(dim, ncell, name)
        sb = oracle.physical_side_basis(dim, order, qdeg, m["nodes"], be, bs)
        x, y, nx, ny = sb["ip"][..., 0], sb["ip"][..., 1], sb["normals"][..., 0], sb["normals"][..., 1]
        if dim == 3:
            z, nz = sb["ip"][..., 2], sb["normals"][..., 2]
            data = 1.5 + x * nx - 2 * y * ny + z * nz + 0.5 * np.sin(3 * x + y - z)
            swapped = 1.5 + x * ny - 2 * y * nz + z * nx + 0.5 * np.sin(3 * x + y - z)
        else:
            data = 1.5 + x * nx - 2 * y * ny + 0.5 * np.sin(3 * x + y)
            swapped = 1.5 + x * ny - 2 * y * nx + 0.5 * np.sin(3 * x + y)
        assert np.abs(data - swapped).max() > 0.1  # on every side the components of the normal are told apart
        assert np.abs(sb["normals"]).min() > 1e-6  # warped: no side is axis-aligned
        oracle.assemble_thermal_boundary(dim, order, qdeg, m["nodes"], m["lids"], m["offsets"], u, be, bs, bc, ("array", data),
                                         rowptr=rowptr, colind=colind, crs_vals=vals_ref, res=res_ref, diff=1.7)
        blk.add_boundary_group(name, bc, be, bs)
        blk.set_function(("Neumann e " if bc == 1 else "Dirichlet e ") + name, s)
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.assemble_boundary(torch.tensor(u, device="cuda"), res, vals)
    torch.cuda.synchronize()
    assert np.abs(vals_ref).max() > 0 and np.abs(res_ref).max() > 0
    figs = (rel_err(res.cpu().numpy(), res_ref), rel_err(vals.cpu().numpy(), vals_ref))
    print("res %.1e crs %.1e" % figs)
    assert max(figs) < RTOL


# ---- f. time ----------------------------------------------------------------------------------------------------------------------

def test_time_in_a_field_string(oracle):
    """set_time, assemble, set_time, assemble on one block: each assembly against the yardstick at its own time."""
    shape = "2d-q1"
    dim, ncell, order, qdeg = X.SHAPES[shape]
    blk, m, ud, kw, g = sweep_block(oracle, shape, False)
    _, u, tr, fixed = X.sweep_case(oracle, shape, False)
    funcs = X.sweep_funcs(dim, "t*c + cos(3*t)*x", "source", {"diffusion": "0.5+t*c*c"})
    set_funcs(blk, funcs)
    refs = {}
    for t in (0.37, 0.9):
        blk.set_time(t)
        refs[t] = R.assemble(oracle, m, qdeg, u, funcs=funcs, fixed=fixed, transient=tr, rowptr=g[0], colind=g[1], time=t)
        figs = against(refs[t], g, *assemble(blk, m, ud, kw, len(g[1])))
        print("t = %g: res %.1e crs %.1e" % ((t,) + figs))
        assert max(figs) < RTOL
    assert rel_err(refs[0.9]["res"], refs[0.37]["res"]) > 1e-3 and rel_err(refs[0.9]["crs_vals"], refs[0.37]["crs_vals"]) > 1e-3


# ---- the edges of the program: inlining (the stack limit runs in the sweeps) ---------------------------------------------

def test_three_levels_of_inlined_functions(oracle):
    """f1 names f2 names f3, constants at every level, the string names them twice: the constant indices are shifted more
    than once.  Every named function is set after the string that names it.  A cycle is refused at assembly."""
    import mrhyde_amd
    shape = "2d-q1"
    dim = X.SHAPES[shape][0]
    blk, m, ud, kw, g = sweep_block(oracle, shape, False)
    named = {k: v for k, v in X.INLINE.items() if k != "source"}
    ref = X.sweep_reference(oracle, shape, X.INLINE["source"], extra=named)
    set_funcs(blk, X.sweep_funcs(dim, X.INLINE["source"], "source"))
    for k in ("f1", "f3", "f2"):
        blk.set_function(k, named[k])
    res, vals = assemble(blk, m, ud, kw, len(g[1]))
    figs = against(ref, g, res, vals)
    print("res %.1e crs %.1e" % figs)
    assert max(figs) < RTOL
    flat = X.sweep_reference(oracle, shape, "(1.25+(0.75*(0.125*c+x)-3.5)*2.5)*(1.25+(0.75*(0.125*c+x)-3.5)*2.5)+(0.75*(0.125*c+x)-3.5)")
    assert rel_err(ref["res"], flat["res"]) < 1e-14 and rel_err(ref["crs_vals"], flat["crs_vals"]) < 1e-14
    blk.set_function("f3", "f1")
    torch = _torch()
    r = torch.full((m["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    v = torch.full((len(g[1]),), -3.0, dtype=torch.float64, device="cuda")
    with pytest.raises(mrhyde_amd.MhaError) as e:
        blk.assemble_jacres(ud, r, v, overwrite=True, **kw)
    torch.cuda.synchronize()
    assert e.value.code == 1
    assert bool((r == 7.0).all()) and bool((v == -3.0).all())
