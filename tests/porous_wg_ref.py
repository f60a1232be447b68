"""Yardstick of the porousWeakGalerkin element step: plain numpy loops over the four residual formulas

    R_pint   = int (div t - source) q
    R_u      = int u . v + pint div v  -  sum_faces int_F pbndry (v . n)
    R_t      = int (perm u + t) . s
    R_pbndry = - sum_faces int_F (t . n) mu

(reference: porousWeakGalerkin::volumeResidual + faceResidual, src/physics/porousWeakGalerkin.cpp:94-323, 424-505) on
general quads and hexes, in float64 or numpy.longdouble.  It shares nothing with the device code: geometry, quadrature,
RT0 tables, elimination and the distance d = |got - yardstick| / (2^-53 S) are those of tests/porous_hybrid_ref.py (numpy
alone).  Every value comes with its scale S, the sum of the absolute values of the terms it is the sum of.

Unknowns of an element: pint, the 2 dim dofs of u, the 2 dim dofs of t (dof 2 c + s as in porous_hybrid_ref), then the
2 dim traces pbndry in the reference's HFACE order; n_int = 1 + 4 dim, n = 1 + 6 dim.  The block is

             pint   u     t     lambda          M_fg = (v_f, v_g)     K_fg = (perm v_f, v_g)
    pint  [   0     0     B^T    0  ]           B_f = (1, div v_f)    C_k = <v_f(k) . n, 1> on face k
    u     [   B     M     0    -C^T ]
    t     [   0     K     M      0  ]
    lam   [   0     0    -C      0  ]

closed_form() is the elimination the fused kernel uses, stated here and checked against condense() of the full block."""
import numpy as np

from porous_hybrid_ref import (LD, U, face_dir, tensor_rule, face_rule, geometry, geometry_scale, det_cof, rt0,  # noqa: F401
                               solve_batched, condense, distance, trace_system, warp, errors, face_centroids, pi_of,
                               gold_source, GEOMETRIES, COEFFICIENTS, make_mesh, family)


def dof_of_face(k):
    """HFACE face k -> flux dof 2 c + s."""
    c, s = face_dir(k)
    return 2 * c + s


def local_matrices(nodes, perm, source, T=np.float64, nq1=2):
    """The raw (unsigned) local matrices in type T with their scales: dict(M, K [E][NU][NU], B [E][NU], C [E][NU][NU]
    (C[e][g][k] = <v_g . n, 1> on face k, dense as the reference's loops are), src [E] = int source, and S_* of each)."""
    nodes = np.asarray(nodes, np.float64).astype(T)
    E, _, dim = nodes.shape
    NU = 2 * dim
    pts, wref = tensor_rule(dim, nq1, T)
    x, J = geometry(nodes, pts)
    SJ, _ = geometry_scale(nodes, pts)
    det, _ = det_cof(J)
    w = wref[None, :] * det
    phi, div = rt0(pts, dim)
    pm = np.asarray(perm(x)).astype(T)
    src = np.asarray(source(x)).astype(T)
    out = dict(src=np.sum(src * w, axis=1), S_src=np.sum(np.abs(src * w), axis=1), perm=pm)
    M, K, SM, SK = (np.zeros((E, NU, NU), T) for _ in range(4))
    B, SB = np.zeros((E, NU), T), np.zeros((E, NU), T)
    for f in range(NU):
        cf = f >> 1
        dv = div[f] / det * w
        B[:, f], SB[:, f] = dv.sum(1), np.abs(dv).sum(1)
        vf = phi[None, :, f] / det
        for g in range(NU):
            cg = g >> 1
            vg = phi[None, :, g] / det
            for d in range(dim):
                term = J[:, :, d, cg] * J[:, :, d, cf] * vg * vf * w
                mag = np.abs(SJ[:, :, d, cg] * SJ[:, :, d, cf] * vg * vf * w)
                M[:, f, g] += term.sum(1)
                SM[:, f, g] += mag.sum(1)
                K[:, f, g] += (pm * term).sum(1)
                SK[:, f, g] += (np.abs(pm) * mag).sum(1)
    C, SC = np.zeros((E, NU, NU), T), np.zeros((E, NU, NU), T)
    for k in range(NU):
        ck, sk = face_dir(k)
        fp, fw = face_rule(dim, k, nq1, T)
        _, Jf = geometry(nodes, fp)
        SJf, Scof = geometry_scale(nodes, fp)
        detf, cof = det_cof(Jf)
        nw = (1 if sk else -1) * cof[:, :, :, ck] * fw[None, :, None]
        phif, _ = rt0(fp, dim)
        for g in range(NU):
            cg = g >> 1
            vg = phif[None, :, g] / detf
            for d in range(dim):
                C[:, g, k] += (vg * Jf[:, :, d, cg] * nw[:, :, d]).sum(1)
                SC[:, g, k] += (np.abs(vg) * SJf[:, :, d, cg] * Scof[:, :, d, ck] * fw[None, :]).sum(1)
    out.update(M=M, K=K, B=B, C=C, S_M=SM, S_K=SK, S_B=SB, S_C=SC)
    return out


def signs_of(orient, E, dim, T):
    """orient [E][4 dim] (u's signs, then t's) or None -> (su, st) [E][2 dim] in type T."""
    NU = 2 * dim
    if orient is None:
        return np.ones((E, NU), T), np.ones((E, NU), T)
    o = np.asarray(orient, np.float64).astype(T)
    assert o.shape == (E, 2 * NU)
    return o[:, :NU], o[:, NU:]


def element_blocks(nodes, orient, state, lam, perm, source, T=np.float64, nq1=2):
    """The uncondensed element arrays in type T.  nodes [E][2^dim][dim]; orient [E][4 dim] (+-1) or None; state
    [E][1 + 4 dim] = pint, u, t; lam [E][2 dim]; perm(x) -> [E][P], source(x) -> [E][P].
    -> dict(res = -res.val(), blocks = d res / d unknown, S_res, S_blocks, cond_M [E], perm_ratio [E])."""
    m = local_matrices(nodes, perm, source, T, nq1)
    E, NU = m["B"].shape
    dim = NU // 2
    NI, N = 1 + 2 * NU, 1 + 3 * NU
    su, st = signs_of(orient, E, dim, T)
    state, lam = np.asarray(state, np.float64).astype(T), np.asarray(lam, np.float64).astype(T)
    coef, S = np.zeros((E, N, N), T), np.zeros((E, N, N), T)
    iu, it, il = slice(1, 1 + NU), slice(1 + NU, NI), slice(NI, N)
    coef[:, 0, it], S[:, 0, it] = st * m["B"], m["S_B"]
    coef[:, iu, 0], S[:, iu, 0] = su * m["B"], m["S_B"]
    coef[:, iu, iu], S[:, iu, iu] = su[:, :, None] * su[:, None, :] * m["M"], m["S_M"]
    coef[:, it, iu], S[:, it, iu] = st[:, :, None] * su[:, None, :] * m["K"], m["S_K"]
    coef[:, it, it], S[:, it, it] = st[:, :, None] * st[:, None, :] * m["M"], m["S_M"]
    coef[:, iu, il], S[:, iu, il] = -su[:, :, None] * m["C"], m["S_C"]
    coef[:, il, it], S[:, il, it] = -np.swapaxes(st[:, :, None] * m["C"], 1, 2), np.swapaxes(m["S_C"], 1, 2)
    full = np.concatenate([state, lam], axis=1)
    val = np.einsum("erc,ec->er", coef, full)
    S_val = np.einsum("erc,ec->er", S, np.abs(full))
    val[:, 0] -= m["src"]
    S_val[:, 0] += m["S_src"]
    pm = np.abs(m["perm"].astype(np.float64))
    return dict(res=-val, blocks=coef, S_res=S_val, S_blocks=S,
                cond_M=np.array([np.linalg.cond(a) for a in m["M"].astype(np.float64)]), perm_ratio=pm.max(1) / pm.min(1))


def volume_block(nodes, orient, perm, source, nq1=2):
    """The volume terms alone (volumeResidual), float64: the interior block [E][NI][NI] and the state-free part of
    res.val() [E][NI] (row pint: -int source)."""
    E = np.asarray(nodes).shape[0]
    dim = np.asarray(nodes).shape[2]
    NI = 1 + 4 * dim
    a = element_blocks(nodes, orient, np.zeros((E, NI)), np.zeros((E, 2 * dim)), perm, source, np.float64, nq1)
    return a["blocks"][:, :NI, :NI], -a["res"][:, :NI]


def cholesky_inverse(M):
    """Mi = M^-1 through M = L L^T, column by column, in M's type.  -> (Mi, every pivot positive [E])."""
    E, n, _ = M.shape
    T = M.dtype.type
    L = np.zeros_like(M)
    ok = np.ones(E, bool)
    for j in range(n):
        dj = M[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1)
        ok &= dj > 0
        dj = np.where(dj > 0, dj, T(1))
        L[:, j, j] = np.sqrt(dj)
        for i in range(j + 1, n):
            L[:, i, j] = (M[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    Li = np.zeros_like(M)
    for j in range(n):
        Li[:, j, j] = 1 / L[:, j, j]
        for i in range(j + 1, n):
            Li[:, i, j] = -np.sum(L[:, i, j:i] * Li[:, j:i, j], axis=1) / L[:, i, i]
    return np.einsum("eki,ekj->eij", Li, Li), ok


def closed_form(nodes, orient, state, lam, perm, source, T=np.float64, nq1=2):
    """The elimination of the fused kernel, in the raw basis (the signs multiply the state on the way in and du on the
    way out; S and g do not see them):  Mi = M^-1 (Cholesky), W = Mi K Mi, Z = W B, sigma = B^T W B,
        dp = (r_p - B^T Mi r_t + Z^T r_u) / sigma,   du = Mi (r_u - B dp),   dt = Mi (r_t - K du),
        S_ab = C_a C_b (W_ab - Z_a Z_b / sigma),     g_a = r_lambda,a + C_a dt_a        (faces and dofs paired)
    -> dict(schur, gvec, du, singular [E])."""
    m = local_matrices(nodes, perm, source, T, nq1)
    E, NU = m["B"].shape
    dim = NU // 2
    su, st = signs_of(orient, E, dim, T)
    state, lam = np.asarray(state, np.float64).astype(T), np.asarray(lam, np.float64).astype(T)
    p, u, t = state[:, 0], su * state[:, 1:1 + NU], st * state[:, 1 + NU:]
    fk = [dof_of_face(k) for k in range(NU)]
    M, K, B = m["M"], m["K"], m["B"]
    C = np.stack([m["C"][:, fk[k], k] for k in range(NU)], axis=1)  # [E][face]
    Cf = np.zeros_like(C)  # indexed by dof
    lamf = np.zeros_like(C)
    for k in range(NU):
        Cf[:, fk[k]], lamf[:, fk[k]] = C[:, k], lam[:, k]
    mv = lambda A, v: np.einsum("eij,ej->ei", A, v)
    r_p = -(np.sum(B * t, axis=1) - m["src"])
    r_u = -(p[:, None] * B + mv(M, u) - Cf * lamf)
    r_t = -(mv(K, u) + mv(M, t))
    r_l = C * np.stack([t[:, fk[k]] for k in range(NU)], axis=1)
    Mi, ok = cholesky_inverse(M)
    W = np.einsum("eij,ejk,ekl->eil", Mi, K, Mi)
    Z = mv(W, B)
    sigma = np.sum(B * Z, axis=1)
    ok &= sigma > 0
    sigma = np.where(sigma > 0, sigma, T(1))
    dp = (r_p - np.sum(B * mv(Mi, r_t), axis=1) + np.sum(Z * r_u, axis=1)) / sigma
    du = mv(Mi, r_u - B * dp[:, None])
    dt = mv(Mi, r_t - mv(K, du))
    schur = np.zeros((E, NU, NU), T)
    gvec = np.zeros((E, NU), T)
    for a in range(NU):
        gvec[:, a] = r_l[:, a] + C[:, a] * dt[:, fk[a]]
        for b in range(NU):
            schur[:, a, b] = C[:, a] * C[:, b] * (W[:, fk[a], fk[b]] - Z[:, fk[a]] * Z[:, fk[b]] / sigma)
    return dict(schur=schur, gvec=gvec, du=np.concatenate([dp[:, None], su * du, st * dt], axis=1), singular=~ok)


# ---- functions of the decks and of the tests ---------------------------------------------------------------------------
PERM_CONSTANT, SOURCE_CONSTANT = 1.5, 0.7
PERM_DECK, SOURCE_DECK = "1.0+x*x+y", "sin(2*pi*x)*y"  # perm in [1, 3] on the unit square: ratio <= 3 within an element


def const_perm(v):
    return lambda x: np.full(x.shape[:2], v, x.dtype)


def element_perm(edata):
    """'use permeability data': perm = data(elem, 0)."""
    return lambda x: np.broadcast_to(np.asarray(edata, np.float64).astype(x.dtype)[:, None], x.shape[:2])


def deck_perm(x):
    return 1 + x[:, :, 0] * x[:, :, 0] + x[:, :, 1]


def deck_source(x):
    return np.sin(2 * pi_of(x) * x[:, :, 0]) * x[:, :, 1]


MIXED = "element data + deck source"  # 'use permeability data' beside a deck-string source: one kernel variant carries both
MIXED_GEOMETRIES = ("2d 3x5 warped", "3d 3x2x2 warped")


def coefficients(kind, mesh, seed=11):
    """-> (perm(x), source(x), element data or None) of a coefficient family on a mesh."""
    if kind == "constant":
        return const_perm(PERM_CONSTANT), const_perm(SOURCE_CONSTANT), None
    if kind == "element data":
        edata = 10.0 ** np.random.default_rng(seed).uniform(-3, 3, mesh["nelem"])  # permeabilities spanning 1e-3 .. 1e3
        return element_perm(edata), const_perm(SOURCE_CONSTANT), edata
    if kind == MIXED:
        edata = 10.0 ** np.random.default_rng(seed).uniform(-3, 3, mesh["nelem"])
        return element_perm(edata), deck_source, edata
    assert kind == "deck strings"
    return deck_perm, deck_source, None


def random_state(mesh, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (mesh["nelem"], 1 + 4 * mesh["dim"])), rng.uniform(-1, 1, mesh["ntrace"])


def gold_true(sign):
    """pint = pbndry = prod sin(2 pi x_d); u = +grad p (sign = 1), t = -grad p (sign = -1)."""
    def true(x):
        dim, pi = x.shape[2], pi_of(x)
        s, c = np.sin(2 * pi * x), np.cos(2 * pi * x)
        v = np.stack([sign * 2 * pi * c[:, :, d] * np.prod(np.delete(s, d, axis=2), axis=2) for d in range(dim)], axis=2)
        return np.prod(s, axis=2), v
    return true


def nearest_data(mesh, points, values):
    """import_mesh_data of the reference (src/interfaces/meshInterface.cpp): the value of the data point nearest to the
    element's centre (mean of its vertices), ties to the lowest index."""
    cen = np.asarray(mesh["nodes"], np.float64).mean(axis=1)
    d2 = ((cen[:, None, :] - np.asarray(points, np.float64)[None, :, :]) ** 2).sum(axis=2)
    return np.asarray(values, np.float64)[np.argmin(d2, axis=1)]


def solve_mesh(mesh, perm, source, lam0, nq1=2):
    """The two-call solve in float64 on the yardstick (porous_hybrid_ref.solve_mesh on this module's block).
    -> (state [E][1 + 4 dim], lam [ntrace], gvec of the second step)."""
    E, dim = mesh["nelem"], mesh["dim"]
    NI = 1 + 4 * dim
    orient = mesh["orient"][:, 1:]
    tl, fixed = mesh["trace_lids"], mesh["trace_side"] != 0
    state, lam = np.zeros((E, NI)), np.array(lam0, np.float64)
    c = condense(element_blocks(mesh["nodes"], orient, state, lam[tl], perm, source, np.float64, nq1), NI)
    Mt, rhs = trace_system(c["schur"], c["gvec"], tl, mesh["ntrace"], fixed)
    lam = lam + np.linalg.solve(Mt, rhs)
    c = condense(element_blocks(mesh["nodes"], orient, state, lam[tl], perm, source, np.float64, nq1), NI)
    return state + c["du"], lam, c["gvec"]


def four_errors(mesh, state, lam, true_u=None, true_t=None, nq1=2):
    """The reference's printed norms in its order pint, pbndry, u, t, by porous_hybrid_ref.errors on (pint, u) and
    (pint, t)."""
    NU = 2 * mesh["dim"]
    mu = dict(mesh, orient=mesh["orient"][:, :1 + NU])
    mt = dict(mesh, orient=np.concatenate([mesh["orient"][:, :1], mesh["orient"][:, 1 + NU:]], axis=1))
    ep, eu, ef = errors(mu, state[:, :1 + NU], lam, true=true_u or gold_true(1), nq1=nq1)
    _, et, _ = errors(mt, np.concatenate([state[:, :1], state[:, 1 + NU:]], axis=1), lam, true=true_t or gold_true(-1), nq1=nq1)
    return ep, ef, eu, et


# K: the largest d of the float64 yardstick against the 80-bit one per input family, measured by tests/test_porous_wg.py
# and recorded as the next integer above 1.25 times the measurement; that test fails when a measurement exceeds its
# constant, or when a family's largest falls below a quarter of a constant above 1.  The device bound is max(8 K, 8).
# "blocks": res and blocks of the plain kernel; "condensed": schur, gvec, du on the componentwise scale.  Measured values
# are tabulated in profiles/porous_weak_galerkin.md.
K_YARDSTICK = {
    ("regular", "constant"): dict(blocks=2, condensed=1),
    ("regular", "element data"): dict(blocks=3, condensed=1),
    ("regular", "deck strings"): dict(blocks=3, condensed=1),
    ("regular", MIXED): dict(blocks=3, condensed=1),
    ("row of 67", "constant"): dict(blocks=19, condensed=1),
    ("row of 67", "element data"): dict(blocks=19, condensed=1),
    ("row of 67", "deck strings"): dict(blocks=19, condensed=1),
    ("stretched", "constant"): dict(blocks=2, condensed=1),
    ("stretched", "element data"): dict(blocks=3, condensed=1),
    ("stretched", "deck strings"): dict(blocks=4, condensed=1),
}
# Guards asserted on every compared case (the issue's): cond_2 of the local mass matrix M, and perm's largest over
# smallest value within an element.
COND_GUARD, PERM_RATIO_GUARD = 1.0e7, 10.0


def bound(fam, group):
    return max(8.0 * K_YARDSTICK[fam][group], 8.0)
