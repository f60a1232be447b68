"""The yardstick of the coupled navierstokes + thermal block (MHA_PHYSICS_NAVIERSTOKES_THERMAL): the two reference
loop nests restated on the numpy forward-AD class of tests/oracle_lib.py.

TEST INFRASTRUCTURE (the checker), imported by tests/test_ns_thermal.py and tests/test_ns_thermal_gpu.py only.

  * seeding: Workset::computeSolnTransientSeeded, seedwhat 1 (src/tools/workset.cpp:589-623) -- AD arrays of width
    n = dofs per element, variable v / dof j seeded at LID position off(v, j);
  * navierstokes::volumeResidual with have_energy (src/physics/navierstokes.cpp:82-849, computeTau :1054-1079): the
    2-D and 3-D branches, the buoyancy terms, the undivided PSPG buoyancy term, the uz block scattered through uy's offsets
    (:688) unless fix_uz_offsets;
  * thermal::volumeResidual with have_nsvel and have_advection (src/physics/thermal.cpp:71-165);
  * the scatter of assemblyManager.cpp:4031-4145: -res.val() into the vector, +res.dx(col) into the CRS, fixed rows
    skipped; local_res / local_J in the updateRes / updateJac convention (LID-position order).

Variables: ux, pr, uy[, uz], e -- the reference's list when navierstokes is imported before thermal.  "density" is one
function read by both modules (FunctionManager::addFunction keeps the first tree of a name, functionManager.cpp:48-68).
"""
import numpy as np

RTOL = 1e-12

FUNC_DEFAULTS = {"source ux": 0.0, "source pr": 0.0, "source uy": 0.0, "source uz": 0.0, "density": 1.0, "viscosity": 1.0,
                 "thermal source": 0.0, "thermal diffusion": 1.0, "specific heat": 1.0, "bx": 0.0, "by": 0.0, "bz": 0.0}
PARAM_DEFAULTS = {"useSUPG": 0, "usePSPG": 0, "fix_uz_offsets": 0, "T_ambient": 0.0, "beta": 1.0, "include advection": 0}


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def crs_err(a, ref, factor=1.0):
    """Per-entry relative error of a CRS value array with a cancellation floor of a thousandth of the row's largest
    entry, beside the array-relative measure (the project's measure for CRS values)."""
    a, b = np.asarray(a), factor * np.asarray(ref["crs_vals"])
    rowptr = np.asarray(ref["rowptr"])
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    rowmax = np.zeros(len(rowptr) - 1)
    np.maximum.at(rowmax, rows, np.abs(b))
    den = np.maximum(np.maximum(np.abs(b), 1e-3 * rowmax[rows]), 1e-300)
    return max(float((np.abs(a - b) / den).max()), rel_err(a, b))


def warp(m):
    """Smooth warp of every vertex: non-affine elements, non-constant Jacobians."""
    v = m["verts"].copy()
    dim = v.shape[1]
    w = v.copy()
    w[:, 0] += 0.06 * np.sin(1.3 * v[:, 1] + 0.4) + (0.04 * v[:, 2] ** 2 if dim == 3 else 0.0)
    w[:, 1] += 0.05 * np.cos(1.1 * v[:, 0]) * (1 + 0.5 * v[:, 1])
    if dim == 3:
        w[:, 2] += 0.05 * v[:, 0] * v[:, 1] + 0.03 * np.sin(2.0 * v[:, 2])
    m["verts"] = w
    m["nodes"] = np.ascontiguousarray(w[m["cell2vert"]])
    return m


def coupled_mesh(oracle, dim, ncell, orders, do_warp=True):
    """orders = (velocity, pressure, energy) -> mesh_multi of ux, pr, uy[, uz], e."""
    ov, op, oe = orders
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * (dim + 2), [ov, op] + [ov] * (dim - 1) + [oe])
    return warp(m) if do_warp else m


def sub_mesh(oracle, m, keep):
    """The mesh of the variables `keep` (indices into m's variable list) on the same cells: mesh_multi numbers the dofs
    of a variable list from the cell topology alone, so the vertices agree.  -> (mesh, rows): rows[r] = the row of the
    full mesh that row r of the sub-mesh is (matched through (variable, element, dof))."""
    dim = m["dim"]
    types, orders = [int(m["types"][v]) for v in keep], [int(m["orders"][v]) for v in keep]
    s = oracle.mesh_multi(dim, m["ncell"], types, orders)
    s["verts"] = m["verts"].copy()
    s["nodes"] = np.ascontiguousarray(s["verts"][s["cell2vert"]])
    assert np.array_equal(s["cell2vert"], m["cell2vert"])
    rows = np.full(s["ndof"], -1, np.int64)
    for k, v in enumerate(keep):
        so = s["offsets"][s["varptr"][k]:s["varptr"][k + 1]]
        mo = m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]
        rows[s["lids"][:, so]] = m["lids"][:, mo]
    assert (rows >= 0).all() and len(np.unique(rows)) == len(rows)
    return s, rows


def transient_state(rng, ndof):
    A, b, bdf = np.array([[0.5, 0.0], [0.3, 0.7]]), np.array([0.4, 0.6]), np.array([1.5, -2.0, 0.5])
    return dict(u_prev=rng.uniform(-1, 1, (ndof, 2)), u_stage=rng.uniform(-1, 1, (ndof, 2)), stage=1, butcher_A=A,
                butcher_b=b, bdf=bdf, dt=0.05)


def _func_at_ip(spec, ip, elems):
    """A named function at the integration points [E][q]: number | ("const", v) | ("sinprod", amp, freq) | ("array", a)."""
    E, nq, dim = ip.shape
    if isinstance(spec, (int, float)):
        return np.full((E, nq), float(spec))
    if spec[0] == "const":
        return np.full((E, nq), float(spec[1]))
    if spec[0] == "sinprod":
        v = np.full((E, nq), float(spec[1]))
        for d in range(dim):
            v = v * np.sin(spec[2][d] * ip[..., d])
        return v
    if spec[0] == "array":
        return np.asarray(spec[1], dtype=np.float64)[elems]
    raise ValueError(spec)


def fields_at_points(oracle, m, qdeg, u, transient=None, elems=None):
    """The seeded solution fields of every variable at the integration points.
    -> dict(names, val[v], dot[v], grad[v][d] (ADView [E][q], width n), B[v], G[v], off[v], wts, ip, h, lids)."""
    AD = oracle.ADView
    dim, nv = m["dim"], len(m["types"])
    elems = np.arange(m["nelem"]) if elems is None else np.asarray(elems)
    nodes, lids = m["nodes"][elems], m["lids"][elems]
    E, n = lids.shape
    names = ["ux", "pr", "uy"] + (["uz"] if dim == 3 else []) + ["e"]
    if transient is None:
        alpha_u, alpha_t = 1.0, 0.0
    else:
        t = transient
        A, b, bdf, st, dt = t["butcher_A"], t["butcher_b"], t["bdf"], t["stage"], t["dt"]
        alpha_u, timewt = A[st, st] / b[st], 1.0 / dt / b[st]
        alpha_t = bdf[0] * timewt
    out = dict(names=names, val=[], dot=[], grad=[], B=[], G=[], off=[], lids=lids, n=n, elems=elems)
    cache = {}
    for v in range(nv):
        order = int(m["orders"][v])
        if order not in cache:
            cache[order] = oracle.physical_basis_var(dim, oracle.HGRAD, order, qdeg, nodes)
        pb = cache[order]
        B, G = pb["basis"][..., 0], pb["grad"]                     # [E][card][q], [E][card][q][dim]
        off = np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]])
        rows = lids[:, off]
        cu = u[rows]
        if transient is None:
            sv, sd = cu, np.zeros_like(cu)
        else:
            up, us = t["u_prev"][rows], t["u_stage"][rows]         # [E][card][steps], [E][card][stages]
            beta_u = (1.0 - alpha_u) * up[..., 0]
            for s in range(st):
                beta_u = beta_u + A[st, s] / b[s] * (us[..., s] - up[..., 0])
            beta_t = np.zeros_like(cu)
            for s in range(1, len(bdf)):
                beta_t = beta_t + bdf[s] * up[..., s - 1]
            beta_t = beta_t * timewt
            sv, sd = alpha_u * cu + beta_u, alpha_t * cu + beta_t
        nq = B.shape[2]

        def field(coef, T, scale):
            dx = np.zeros((E, nq, n))
            dx[:, :, off] = scale * np.transpose(T, (0, 2, 1))
            return AD(np.einsum("ej,ejq->eq", coef, T), dx)
        out["val"].append(field(sv, B, alpha_u))
        out["dot"].append(field(sd, B, alpha_t))
        out["grad"].append([field(sv, G[..., d], alpha_u) for d in range(dim)])
        out["B"].append(B)
        out["G"].append(G)
        out["off"].append(off)
        out["wts"], out["ip"] = pb["wts"], pb["ip"]
    out["h"] = out["wts"].sum(axis=1) ** (1.0 / dim)              # Workset::getElementSize
    return out


def element_arrays(oracle, m, qdeg, u, *, funcs=None, params=None, transient=None, elems=None, momentum_sources=None):
    """res(elem, pos) and its derivative array, both modules -> (R [E][n], J [E][n][n]) in LID-position order, plus the
    field dict.  momentum_sources: optional replacement [dim] of the momentum rows' source arrays (tests)."""
    AD = oracle.ADView
    dim = m["dim"]
    F = fields_at_points(oracle, m, qdeg, u, transient, elems)
    E, n = F["lids"].shape
    w, ip, h = F["wts"], F["ip"], F["h"]
    fs = dict(FUNC_DEFAULTS)
    fs.update(funcs or {})
    assert set(fs) == set(FUNC_DEFAULTS), set(fs) - set(FUNC_DEFAULTS)
    P = dict(PARAM_DEFAULTS)
    P.update(params or {})
    assert set(P) == set(PARAM_DEFAULTS), set(P) - set(PARAM_DEFAULTS)
    fv = {k: _func_at_ip(s, ip, F["elems"]) for k, s in fs.items()}
    dens, visc = fv["density"], fv["viscosity"]
    vn = [0, 2, 3][:dim]
    prn, en = 1, dim + 1
    src = [fv["source ux"], fv["source uy"], fv["source uz"]][:dim]
    if momentum_sources is not None:
        src = list(momentum_sources)
    vel = [F["val"][v] for v in vn]
    pr, T = F["val"][prn], F["val"][en]
    R, J = np.zeros((E, n)), np.zeros((E, n, n))
    zero = AD(np.zeros_like(w), W=n)

    def add_rows(var, Fv, Fg):
        """res(elem, off(var, dof)) += sum_pt Fv basis + sum_d Fg[d] basis_grad[d]   (weights already in Fv, Fg)"""
        B, G, off = F["B"][var], F["G"][var], F["off"][var]
        rv = np.einsum("eq,ejq->ej", Fv.val, B)
        rdx = np.einsum("eqw,ejq->ejw", Fv.dx, B)
        for d in range(dim):
            if Fg[d] is None:
                continue
            rv = rv + np.einsum("eq,ejq->ej", Fg[d].val, G[..., d])
            rdx = rdx + np.einsum("eqw,ejq->ejw", Fg[d].dx, G[..., d])
        R[:, off] += rv
        J[:, off, :] += rdx

    tau = None
    if P["useSUPG"] or P["usePSPG"]:  # computeTau (navierstokes.cpp:1054-1079)
        C1, C2, C3 = 4.0, 2.0, (2.0 if transient is not None else 0.0)
        dt = float(transient["dt"]) if transient is not None else 1.0
        nvel = zero
        for d in range(dim):
            nvel = nvel + vel[d] * vel[d]
        big = nvel.val > 1e-12
        sq = np.sqrt(np.where(big, nvel.val, 1.0))
        nvel = AD(np.where(big, sq, nvel.val), np.where(big[..., None], nvel.dx / (2.0 * sq[..., None]), nvel.dx))
        hh = np.broadcast_to(h[:, None], w.shape)  # (full shape: the AD class lifts arrays of its own shape)
        # (ADView on the left of every mixed product: numpy would broadcast an array on the left over the object)
        t = (nvel * (C2 / hh)) * (nvel * (C2 / hh)) + ((C1 * visc / hh / hh) ** 2 + (C3 / dt) ** 2)
        tau = 1.0 / AD(np.sqrt(t.val), t.dx / (2.0 * np.sqrt(t.val))[..., None])
    buoy = (T - float(P["T_ambient"])) * float(P["beta"])  # params(1) * (E - params(0))
    stab = []
    for i in range(dim):
        v = vn[i]
        # the uz block goes through uy's offsets (navierstokes.cpp:688) unless fix_uz_offsets
        rowvar = vn[1] if (dim == 3 and i == 2 and not P["fix_uz_offsets"]) else v
        gu = F["grad"][v]
        conv = zero
        for d in range(dim):
            conv = conv + vel[d] * gu[d]
        Fv = (F["dot"][v] + conv - src[i]) * (dens * w)
        Fg = [(gu[d] * visc - (pr if d == i else 0.0)) * w for d in range(dim)]
        add_rows(rowvar, Fv, Fg)
        add_rows(rowvar, buoy * (dens * src[i] * w), [None] * dim)                      # energy contribution
        sr = F["dot"][v] * dens + conv * dens + F["grad"][prn][i] - dens * src[i]
        stab.append(sr)
        if P["useSUPG"]:
            add_rows(rowvar, zero, [tau * sr * vel[d] * w for d in range(dim)])
            sre = buoy * (dens * src[i])
            add_rows(rowvar, zero, [tau * sre * vel[d] * w for d in range(dim)])
    divu = zero
    for i in range(dim):
        divu = divu + F["grad"][vn[i]][i]
    add_rows(prn, divu * w, [None] * dim)
    if P["usePSPG"]:
        add_rows(prn, zero, [stab[d] * (tau * (w / dens)) for d in range(dim)])
        # the buoyancy part is not divided by the density (navierstokes.cpp:480-483, 833-838)
        add_rows(prn, zero, [buoy * (dens * src[d]) * (tau * w) for d in range(dim)])
    # thermal (thermal.cpp:125-163)
    ge = F["grad"][en]
    Fv = (F["dot"][en] * (dens * fv["specific heat"]) - fv["thermal source"]) * w
    adv = zero
    for d in range(dim):
        adv = adv + vel[d] * ge[d]                                                      # have_nsvel
    if P["include advection"]:
        for d, k in enumerate(["bx", "by", "bz"][:dim]):
            adv = adv + ge[d] * fv[k]
    add_rows(en, Fv + adv * w, [ge[d] * (fv["thermal diffusion"] * w) for d in range(dim)])
    return R, J, F


def scatter(m, R, J, lids, fixed=None, rowptr=None, colind=None, oracle=None):
    """-res.val() into the vector, +res.dx(col) into the CRS, fixed rows skipped (assemblyManager.cpp:4031-4145)."""
    ndof = m["ndof"]
    if rowptr is None:
        rowptr, colind = oracle.build_graph(ndof, m["lids"])
    E, n = lids.shape
    res, vals = np.zeros(ndof), np.zeros(rowptr[-1])
    rows = lids.astype(np.int64)
    live = np.ones((E, n), bool) if fixed is None else (np.asarray(fixed)[rows] == 0)
    np.add.at(res, rows[live], -R[live])
    crs_rows = np.repeat(np.arange(ndof, dtype=np.int64), np.diff(rowptr))
    keys = crs_rows * ndof + np.asarray(colind, dtype=np.int64)
    assert np.all(np.diff(keys) > 0), "CRS columns must be sorted within rows"
    want = rows[:, :, None] * ndof + rows[:, None, :]
    idx = np.searchsorted(keys, want)
    assert np.array_equal(keys[np.minimum(idx, len(keys) - 1)], want), "an element's column is missing from the graph"
    mask = np.broadcast_to(live[:, :, None], (E, n, n))
    np.add.at(vals, idx[mask], J[mask])
    return dict(rowptr=rowptr, colind=colind, res=res, crs_vals=vals)


def assemble(oracle, m, qdeg, u, *, funcs=None, params=None, fixed=None, transient=None, rowptr=None, colind=None,
             elems=None, momentum_sources=None, want_global=True):
    """The coupled block's res / crs_vals / local_J / local_res (elems: a subset -> local arrays of those elements only)."""
    R, J, F = element_arrays(oracle, m, qdeg, u, funcs=funcs, params=params, transient=transient, elems=elems,
                             momentum_sources=momentum_sources)
    out = dict(local_res=-R, local_J=J, fields=F)
    if want_global and elems is None:
        out.update(scatter(m, R, J, F["lids"], fixed, rowptr, colind, oracle))
    return out


def var_rows(m, v):
    """Global rows of variable v."""
    off = m["offsets"][m["varptr"][v]:m["varptr"][v + 1]]
    return np.unique(m["lids"][:, off])
