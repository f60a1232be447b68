"""The yardstick of the helmholtz module (MHA_PHYSICS_HELMHOLTZ): helmholtz::volumeResidual and ::boundaryResidual
restated, loop by loop, on the numpy forward-AD class of tests/oracle_lib.py.

TEST INFRASTRUCTURE (the checker), imported by tests/test_helmholtz.py and tests/test_helmholtz_gpu.py only.

  * seeding: Workset::computeSolnTransientSeeded, seedwhat 1 (src/tools/workset.cpp:589-623), through
    ns_thermal_ref.fields_at_points for the volume and side_fields below for the sides -- AD arrays as wide as the block;
  * the functions: deck strings in the coordinates with the deck's other strings as named helpers (oracle_lib.deck_eval_ad
    on plain arrays), numbers, ("sinprod", amp, freq) and ("array", a);
  * helmholtz::volumeResidual (src/physics/helmholtz.cpp:137-193, the non-fractional branch): the loop over the basis
    index i with vr = ureal's basis i and vi = uimag's basis i kept as SEPARATE arrays, the expressions of :175-193 term
    by term -- nothing of the device's collapsed form (vr = vi) is used;
  * helmholtz::boundaryResidual (:320-375) on the entries of a "Neumann" side, again with vr and vi apart;
  * the scatter of assemblyManager.cpp:4031-4145 (ns_thermal_ref.scatter).
"""
import numpy as np

import ns_thermal_ref as N
from cdr_ref import dense, l2_error  # noqa: F401  (re-exported)
from ns_thermal_ref import RTOL, crs_err, rel_err, transient_state, var_rows, warp  # noqa: F401  (re-exported)

# reference defaults: every function "0.0" (helmholtz.cpp:41-70)
VOLUME_FUNCS = ("c2r_x", "c2i_x", "c2r_y", "c2i_y", "c2r_z", "c2i_z", "omega2r", "omega2i", "source_r", "source_i")
SIDE_FUNCS = ("c2r_x", "c2i_x", "c2r_y", "c2i_y", "c2r_z", "c2i_z", "robin_alpha_r", "robin_alpha_i", "source_r_side",
              "source_i_side")
UNUSED_FUNCS = ("omegar", "omegai", "alphaHr", "alphaHi", "alphaTr", "alphaTi", "freqExp")
SIDE_NAMES = {2: ("bottom", "right", "top", "left"), 3: ("bottom", "right", "top", "left", "back", "front")}


def helmholtz_mesh(oracle, dim, ncell, order, do_warp=True, orders=None):
    m = oracle.mesh_multi(dim, ncell, [oracle.HGRAD] * 2, list(orders) if orders else [order, order])
    return warp(m) if do_warp else m


def func_at(oracle, spec, ip, elems, strings, nrm=None):
    """One named function at the points ip [K][q][dim] as a plain array [K][q]."""
    K, nq, dim = ip.shape
    if isinstance(spec, str):
        fields = {c: ip[..., d] for d, c in enumerate("xyz"[:dim])}
        fields["t"] = np.zeros((K, nq))
        for d, c in enumerate(["nx", "ny", "nz"]):
            fields[c] = nrm[..., d] if (nrm is not None and d < dim) else np.zeros((K, nq))
        for c in ["z"][:3 - dim] + ["h"]:
            fields[c] = np.zeros((K, nq))
        return np.broadcast_to(np.asarray(oracle.deck_eval_ad(spec, fields, strings), dtype=np.float64), (K, nq)).copy()
    return N._func_at_ip(spec, ip, elems)


def _functions(oracle, funcs, names, ip, elems, nrm=None):
    fs = {k: 0.0 for k in VOLUME_FUNCS + SIDE_FUNCS + UNUSED_FUNCS}
    fs.update(funcs or {})
    strings = {k: (v if isinstance(v, str) else repr(float(v))) for k, v in fs.items() if isinstance(v, (str, int, float))}
    return {k: func_at(oracle, fs[k], ip, elems, strings, nrm) for k in names}


def volume_arrays(oracle, m, qdeg, u, *, funcs=None, transient=None, elems=None):
    """res(elem, off(var, i)) and its derivative array of helmholtz::volumeResidual -> (R [E][n], J [E][n][n]) in
    LID-position order, plus the field dict."""
    dim = m["dim"]
    assert len(m["types"]) == 2
    F = N.fields_at_points(oracle, m, qdeg, u, transient, elems)
    E, n = F["lids"].shape
    w = F["wts"]
    fv = _functions(oracle, funcs, VOLUME_FUNCS, F["ip"], F["elems"])
    ur_num, ui_num = 0, 1
    Ur, Ui = F["val"][ur_num], F["val"][ui_num]
    dUr, dUi = F["grad"][ur_num], F["grad"][ui_num]
    urbasis, uibasis = F["B"][ur_num], F["B"][ui_num]                 # [E][card][q]
    urbasis_grad, uibasis_grad = F["G"][ur_num], F["G"][ui_num]       # [E][card][q][dim]
    c2r = [fv["c2r_x"], fv["c2r_y"], fv["c2r_z"]]
    c2i = [fv["c2i_x"], fv["c2i_y"], fv["c2i_z"]]
    omega2r, omega2i, source_r, source_i = fv["omega2r"], fv["omega2i"], fv["source_r"], fv["source_i"]
    R, J = np.zeros((E, n)), np.zeros((E, n, n))
    for i in range(urbasis.shape[1]):  # "what if ui uses a different basis?" (helmholtz.cpp:155): it is indexed by i too
        vr, vi = urbasis[:, i, :], uibasis[:, i, :]
        dvr = [urbasis_grad[:, i, :, d] for d in range(dim)]
        dvi = [uibasis_grad[:, i, :, d] for d in range(dim)]
        # (ADView on the left of every mixed product: numpy would broadcast an array on the left over the object)
        # :175-182
        r = -((Ur * vr + Ui * vi) * omega2r) + (Ui * vr - Ur * vi) * omega2i
        for d in range(dim):
            r = r + (dUr[d] * dvr[d] + dUi[d] * dvi[d]) * c2r[d] - (dUi[d] * dvr[d] - dUr[d] * dvi[d]) * c2i[d]
        r = (r - (source_r * vr + source_i * vi)) * w
        R[:, F["off"][ur_num][i]] += r.val.sum(axis=1)
        J[:, F["off"][ur_num][i], :] += r.dx.sum(axis=1)
        # :186-193
        r = -((Ui * vr - Ur * vi) * omega2r) - (Ur * vr + Ui * vi) * omega2i
        for d in range(dim):
            r = r + (dUi[d] * dvr[d] - dUr[d] * dvi[d]) * c2r[d] + (dUr[d] * dvr[d] + dUi[d] * dvi[d]) * c2i[d]
        r = (r - (source_i * vr - source_r * vi)) * w
        R[:, F["off"][ui_num][i]] += r.val.sum(axis=1)
        J[:, F["off"][ui_num][i], :] += r.dx.sum(axis=1)
    return R, J, F


def side_fields(oracle, m, qdeg, u, belem, bside, transient=None):
    """The seeded side fields of both variables on the entries (belem, bside): evaluateSideSolutionField
    (workset.cpp:1069-1176).  -> dict(val[v], grad[v][d] (ADView [K][qs], width n), B[v], wts, normals, ip, lids)."""
    AD = oracle.ADView
    dim = m["dim"]
    belem = np.asarray(belem, dtype=np.int32)
    lids = m["lids"][belem]
    K, n = lids.shape
    if transient is None:
        alpha_u = 1.0
    else:
        t = transient
        A, b, st = t["butcher_A"], t["butcher_b"], t["stage"]
        alpha_u = A[st, st] / b[st]
    out = dict(val=[], grad=[], B=[], G=[], off=[], lids=lids, n=n)
    for v in range(2):
        sb = oracle.physical_side_basis(dim, int(m["orders"][v]), qdeg, m["nodes"], belem, bside)
        B, G = sb["basis"], sb["basis_grad"]                          # [K][card][qs], [K][card][qs][dim]
        off = np.asarray(m["offsets"][m["varptr"][v]:m["varptr"][v + 1]])
        rows = lids[:, off]
        cu = u[rows]
        if transient is None:
            sv = cu
        else:
            up, us = t["u_prev"][rows], t["u_stage"][rows]
            beta_u = (1.0 - alpha_u) * up[..., 0]
            for s in range(st):
                beta_u = beta_u + A[st, s] / b[s] * (us[..., s] - up[..., 0])
            sv = alpha_u * cu + beta_u
        nqs = B.shape[2]

        def field(T):
            dx = np.zeros((K, nqs, n))
            dx[:, :, off] = alpha_u * np.transpose(T, (0, 2, 1))
            return AD(np.einsum("kj,kjq->kq", sv, T), dx)
        out["val"].append(field(B))
        out["grad"].append([field(G[..., d]) for d in range(dim)])
        out["B"].append(B)
        out["off"].append(off)
        out["wts"], out["normals"], out["ip"] = sb["wts"], sb["normals"], sb["ip"]
    return out


def side_arrays(oracle, m, qdeg, u, belem, bside, *, funcs=None, transient=None):
    """helmholtz::boundaryResidual on the entries of a side whose condition is "Neumann" (helmholtz.cpp:320-375) ->
    (R [K][n], J [K][n][n]) in LID-position order, plus the side field dict."""
    dim = m["dim"]
    S = side_fields(oracle, m, qdeg, u, belem, bside, transient)
    K, n = S["lids"].shape
    w, nrm = S["wts"], S["normals"]
    fv = _functions(oracle, funcs, SIDE_FUNCS, S["ip"], np.arange(K), nrm)
    ur_num, ui_num = 0, 1
    ur, ui = S["val"][ur_num], S["val"][ui_num]
    dur, dui = S["grad"][ur_num], S["grad"][ui_num]
    c2r = [fv["c2r_x"], fv["c2r_y"], fv["c2r_z"]]
    c2i = [fv["c2i_x"], fv["c2i_y"], fv["c2i_z"]]
    ar, ai = fv["robin_alpha_r"], fv["robin_alpha_i"]
    source_r_side, source_i_side = fv["source_r_side"], fv["source_i_side"]
    durdn, duidn = dur[0] * nrm[..., 0], dui[0] * nrm[..., 0]                                   # :328-344
    for d in range(1, dim):
        durdn, duidn = durdn + dur[d] * nrm[..., d], duidn + dui[d] * nrm[..., d]
    c2durdn = (dur[0] * c2r[0] - dui[0] * c2i[0]) * nrm[..., 0]                                  # :346-355
    c2duidn = (dui[0] * c2r[0] + dur[0] * c2i[0]) * nrm[..., 0]
    for d in range(1, dim):
        c2durdn = c2durdn + (dur[d] * c2r[d] - dui[d] * c2i[d]) * nrm[..., d]
        c2duidn = c2duidn + (dui[d] * c2r[d] + dur[d] * c2i[d]) * nrm[..., d]
    urbasis, uibasis = S["B"][ur_num], S["B"][ui_num]
    R, J = np.zeros((K, n)), np.zeros((K, n, n))
    for i in range(urbasis.shape[1]):
        vr, vi = urbasis[:, i, :], uibasis[:, i, :]
        r = ((((ur * vr + ui * vi) * ar - (ui * vr - ur * vi) * ai) + (durdn * vr + duidn * vi)    # :363-366
              - (source_r_side * vr + source_i_side * vi)) - (c2durdn * vr + c2duidn * vi)) * w
        R[:, S["off"][ur_num][i]] += r.val.sum(axis=1)
        J[:, S["off"][ur_num][i], :] += r.dx.sum(axis=1)
        r = ((((ui * vr - ur * vi) * ar + (ur * vr + ui * vi) * ai) + (duidn * vr - durdn * vi)    # :370-373
              - (source_i_side * vr - source_r_side * vi)) - (c2duidn * vr - c2durdn * vi)) * w
        R[:, S["off"][ui_num][i]] += r.val.sum(axis=1)
        J[:, S["off"][ui_num][i], :] += r.dx.sum(axis=1)
    return R, J, S


def assemble(oracle, m, qdeg, u, *, funcs=None, fixed=None, transient=None, rowptr=None, colind=None, sides=None):
    """res / crs_vals of a helmholtz block: the volume terms and, with sides = [(belem, bside), ...], the Robin terms of
    those Neumann groups on top."""
    R, J, F = volume_arrays(oracle, m, qdeg, u, funcs=funcs, transient=transient)
    out = N.scatter(m, R, J, F["lids"], fixed, rowptr, colind, oracle)
    out["fields"] = F
    for belem, bside in (sides or []):
        add = assemble_sides(oracle, m, qdeg, u, belem, bside, funcs=funcs, fixed=fixed, transient=transient,
                             rowptr=out["rowptr"], colind=out["colind"])
        out["res"] += add["res"]
        out["crs_vals"] += add["crs_vals"]
    return out


def assemble_sides(oracle, m, qdeg, u, belem, bside, *, funcs=None, fixed=None, transient=None, rowptr=None, colind=None):
    """The Robin terms of one Neumann group alone."""
    R, J, S = side_arrays(oracle, m, qdeg, u, belem, bside, funcs=funcs, transient=transient)
    out = N.scatter(m, R, J, S["lids"], fixed, rowptr, colind, oracle)
    out["side_fields"] = S
    return out


def all_sides_group(oracle, m):
    """Entries of EVERY local side id: each named side of the structured mesh, concatenated."""
    be, bs = zip(*[oracle.boundary_sides(m["dim"], m["ncell"], nm) for nm in SIDE_NAMES[m["dim"]]])
    return np.concatenate(be).astype(np.int32), np.concatenate(bs).astype(np.int32)


# regression/helmholtz/manufactured_solution/input.yaml: the Functions block, as written there
GOLD_FUNCS = {
    "source_r_side": "2.0*pi*cos(2*pi*x)*sin(2*pi*y)",
    "source_i_side": "2.0*pi*cos(2*pi*x)*sin(2*pi*y)",
    "omega": "1.0",
    "scoeff": "8*pi*pi*(x*x-2*x-1)-1.0",
    "scoeffi": "8*pi*pi*(x*x+2*x-1)-1.0",
    "srcoeff": "2.0-2*x",
    "sicoeff": "-2.0-2*x",
    "source_r": "scoeff*sin(2*pi*x)*sin(2*pi*y) + srcoeff*2*pi*cos(2*pi*x)*sin(2*pi*y)",
    "source_i": "scoeffi*sin(2*pi*x)*sin(2*pi*y) + sicoeff*2*pi*cos(2*pi*x)*sin(2*pi*y)",
    "c2r_x": "x*x-1.0",
    "c2i_x": "2.0*x",
    "c2r_y": "x*x-1.0",
    "c2i_y": "2.0*x",
    "omega2r": "1.0",
    "omega2i": "0.0",
}


def gold_manufactured(oracle, assemble_fn, ncell=(100, 100)):
    """regression/helmholtz/manufactured_solution: Q1 / Q1, 2x2 Gauss, ureal = uimag = 0 strongly on left / top / bottom,
    the Neumann (Robin) condition on right, from u = 0; the problem is linear: ONE direct solve.
    assemble_fn(m, u, funcs, fixed, (belem, bside)) -> (J csr with identity fixed rows, rhs = -res).
    -> [L2 error of ureal, L2 error of uimag] against sin(2 pi x) sin(2 pi y)."""
    import scipy.sparse.linalg as spla
    m = helmholtz_mesh(oracle, 2, ncell, 1, do_warp=False)
    fixed = ((m["side_mask"] & 0b1101) != 0).astype(np.uint8)  # left, bottom, top
    belem, bside = oracle.boundary_sides(2, ncell, "right")
    u = np.zeros(m["ndof"])
    J, rhs = assemble_fn(m, u, dict(GOLD_FUNCS), fixed, (belem, bside))
    u = u + spla.spsolve(J.tocsc(), rhs)
    true = lambda x: np.sin(2 * np.pi * x[..., 0]) * np.sin(2 * np.pi * x[..., 1])
    return [l2_error(oracle, m, 2, u, v, true) for v in range(2)]


def with_identity_rows(ref, fixed, ndof):
    """The yardstick's matrix with 1 on the diagonal of the fixed rows, and rhs = the assembled vector (-res.val())."""
    import scipy.sparse as sp
    J = dense(ref, ndof).tolil()
    for r in np.flatnonzero(fixed):
        J[r, r] = 1.0
    return sp.csr_matrix(J), ref["res"].copy()
