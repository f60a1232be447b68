"""Yardstick of the porousMixedHybridized element step: plain numpy loops over the three residual formulas

    R_u = int (Kinv u) . v - p div v + sum_faces int_F lambda v . n
    R_p = int (-div u + source) q
    R_lambda = - sum_faces int_F (u . n) mu

(reference: porousMixedHybrid::volumeResidual + faceResidual, src/physics/porousMixedHybridized.cpp:72-189, 287-362) on
general quads and hexes, in any numpy float type: float64, or numpy.longdouble (the 80-bit format of x86) where precision
is measured.  It shares nothing with the device code or with the C oracle: its own RT0 / HFACE-0 tables, its own side
geometry (the cofactor of the cell Jacobian, no tangents), its own Gaussian elimination.  Every value comes with its
scale S, the sum of the absolute values of the terms it is the sum of -- down to the vertex terms x_v dN_v of the cell
Jacobian, whose cancellation an implementation that reads vertex coordinates cannot avoid --; d = |got - yardstick| / (2^-53 S) is the distance
the tests assert on (profiles/extended_precision_yardstick.md).

Unknowns of an element: p, the 2 dim flux dofs (dof 2 c + s: the raw function (1 -/+ xi_c) / 2 e_c, low / high face of
direction c; physical J phi / det J, times the orientation sign), then the 2 dim traces in the reference's HFACE order
left, bottom, right, top[, front, back] (src/tools/Intrepid2_HFACE_HEX_In_FEMdef.hpp:97-269)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def face_dir(k):
    """HFACE face k -> (direction c, 0 low / 1 high)."""
    return (k & 1, k >> 1) if k < 4 else (2, k - 4)


def vertex_signs(dim):
    """Reference coordinates of the shards vertices: quad (-1,-1), (1,-1), (1,1), (-1,1); hex the same at z = -1, then +1."""
    q = [(-1, -1), (1, -1), (1, 1), (-1, 1)]
    return np.array(q if dim == 2 else [v + (z,) for z in (-1, 1) for v in q], dtype=np.float64)


def gauss(n, T):
    """n-point Gauss-Legendre rule on [-1, 1] in type T."""
    if n == 1:
        return np.array([0], T), np.array([2], T)
    if n == 2:
        a = np.sqrt(T(1) / T(3))
        return np.array([-a, a], T), np.array([1, 1], T)
    assert n == 3
    a = np.sqrt(T(3) / T(5))
    return np.array([-a, 0, a], T), np.array([T(5) / T(9), T(8) / T(9), T(5) / T(9)], T)


def tensor_rule(dim, n, T):
    x, w = gauss(n, T)
    g = np.meshgrid(*([x] * dim), indexing="ij")
    gw = np.meshgrid(*([w] * dim), indexing="ij")
    pts = np.stack([a.ravel() for a in g], axis=1)
    wts = np.prod(np.stack([a.ravel() for a in gw], axis=1), axis=1)
    return pts.astype(T), wts.astype(T)


def face_rule(dim, k, n, T):
    """Points (cell reference coordinates) and reference weights of face k."""
    c, s = face_dir(k)
    p, w = tensor_rule(dim - 1, n, T)
    pts = np.empty((len(w), dim), T)
    pts[:, c] = T(1) if s else T(-1)
    pts[:, [d for d in range(dim) if d != c]] = p
    return pts, w


def geometry(nodes, pts):
    """x [E][P][dim], J [E][P][dim][dim] (J_ic = d x_i / d xi_c) of the multilinear map at reference points pts [P][dim]."""
    T = nodes.dtype.type
    dim = nodes.shape[2]
    sg = vertex_signs(dim).astype(T)
    half = T(1) / T(2)
    fac = half * (1 + sg[None, :, :] * pts[:, None, :])  # [P][V][dim]
    N = np.prod(fac, axis=2)
    dN = np.empty(fac.shape, T)
    for c in range(dim):
        others = np.prod(np.delete(fac, c, axis=2), axis=2)
        dN[:, :, c] = half * sg[None, :, c] * others
    x = np.einsum("evi,pv->epi", nodes, N)
    J = np.einsum("evi,pvc->epic", nodes, dN)
    return x, J


def geometry_scale(nodes, pts):
    """Magnitudes of the sums behind J and its cofactor: SJ_ic = sum_v |x_vi| |dN_v / dxi_c|, Scof from SJ by the cofactor
    formulas with every sign positive.  An entry of J that is zero by cancellation between vertices (an axis-aligned cell)
    has a scale, and an implementation leaves round-off of that size there."""
    T = nodes.dtype.type
    dim = nodes.shape[2]
    sg = vertex_signs(dim).astype(T)
    half = T(1) / T(2)
    fac = half * (1 + sg[None, :, :] * pts[:, None, :])
    dN = np.empty(fac.shape, T)
    for c in range(dim):
        dN[:, :, c] = half * np.prod(np.delete(fac, c, axis=2), axis=2)
    SJ = np.einsum("evi,pvc->epic", np.abs(nodes), np.abs(dN))
    if dim == 2:
        Scof = np.stack([np.stack([SJ[..., 1, 1], SJ[..., 1, 0]], -1), np.stack([SJ[..., 0, 1], SJ[..., 0, 0]], -1)], -2)
        return SJ, Scof
    Scof = np.empty(SJ.shape, T)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            Scof[..., i, j] = SJ[..., i1, j1] * SJ[..., i2, j2] + SJ[..., i1, j2] * SJ[..., i2, j1]
    return SJ, Scof


def det_cof(J):
    """det J and the cofactor matrix det J J^-T ([..][dim][dim]) by the explicit formulas."""
    if J.shape[-1] == 2:
        a, b, c, d = J[..., 0, 0], J[..., 0, 1], J[..., 1, 0], J[..., 1, 1]
        det = a * d - b * c
        cof = np.stack([np.stack([d, -c], -1), np.stack([-b, a], -1)], -2)
        return det, cof
    cof = np.empty(J.shape, J.dtype)
    for i in range(3):
        for j in range(3):
            i1, i2 = (i + 1) % 3, (i + 2) % 3
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            cof[..., i, j] = J[..., i1, j1] * J[..., i2, j2] - J[..., i1, j2] * J[..., i2, j1]
    det = J[..., 0, 0] * cof[..., 0, 0] + J[..., 0, 1] * cof[..., 0, 1] + J[..., 0, 2] * cof[..., 0, 2]
    return det, cof


def rt0(pts, dim):
    """Raw RT0 tables at reference points: phi [P][2 dim] (the component along e_c), reference divergence [2 dim]."""
    T = pts.dtype.type
    half = T(1) / T(2)
    phi = np.stack([half * (1 + (1 if f & 1 else -1) * pts[:, f >> 1]) for f in range(2 * dim)], axis=1)
    div = np.array([half if f & 1 else -half for f in range(2 * dim)], T)
    return phi, div


def element_blocks(nodes, orient, state, lam, kinv, source, T=np.float64, nq1=2):
    """The uncondensed element arrays in type T, from inputs given in float64 (exact in T).
    nodes [E][2^dim][dim]; orient [E][2 dim] (+-1) or None; state [E][1 + 2 dim] = p, u; lam [E][2 dim];
    kinv(x) -> [E][P][dim] and source(x) -> [E][P] for points x [E][P][dim] of type T.
    -> dict(res, blocks, S_res, S_blocks): res = -res.val(), blocks = d res / d unknown, and their scales."""
    nodes = np.asarray(nodes, np.float64).astype(T)
    E, _, dim = nodes.shape
    NU, NI = 2 * dim, 1 + 2 * dim
    N = NI + NU
    sg = np.ones((E, NU), T) if orient is None else np.asarray(orient, np.float64).astype(T)
    state, lam = np.asarray(state, np.float64).astype(T), np.asarray(lam, np.float64).astype(T)
    coef, S = np.zeros((E, N, N), T), np.zeros((E, N, N), T)
    # ---- volume ----
    pts, wref = tensor_rule(dim, nq1, T)
    x, J = geometry(nodes, pts)
    SJ, _ = geometry_scale(nodes, pts)
    det, _ = det_cof(J)
    w = wref[None, :] * det
    phi, div = rt0(pts, dim)
    K = np.asarray(kinv(x)).astype(T)
    src = np.asarray(source(x)).astype(T)
    data, S_data = np.sum(src * w, axis=1), np.sum(np.abs(src * w), axis=1)
    for f in range(NU):
        cf = f >> 1
        dv = sg[:, f, None] * div[f] / det * w  # div v_f w  [E][P]
        coef[:, 0, 1 + f] -= dv.sum(1)
        S[:, 0, 1 + f] += np.abs(dv).sum(1)
        coef[:, 1 + f, 0] -= dv.sum(1)
        S[:, 1 + f, 0] += np.abs(dv).sum(1)
        vf = sg[:, f, None] * phi[None, :, f] / det
        for g in range(NU):
            cg = g >> 1
            vg = sg[:, g, None] * phi[None, :, g] / det
            for d in range(dim):
                term = K[:, :, d] * J[:, :, d, cg] * J[:, :, d, cf] * vg * vf * w
                coef[:, 1 + f, 1 + g] += term.sum(1)
                S[:, 1 + f, 1 + g] += np.abs(K[:, :, d] * SJ[:, :, d, cg] * SJ[:, :, d, cf] * vg * vf * w).sum(1)
    # ---- faces: n w = sigma cof[:, c] w_ref on the face xi_c = sigma ----
    for k in range(NU):
        ck, sk = face_dir(k)
        fp, fw = face_rule(dim, k, nq1, T)
        _, Jf = geometry(nodes, fp)
        SJf, Scof = geometry_scale(nodes, fp)
        detf, cof = det_cof(Jf)
        nw = (1 if sk else -1) * cof[:, :, :, ck] * fw[None, :, None]  # [E][P][dim]
        phif, _ = rt0(fp, dim)
        for g in range(NU):
            cg = g >> 1
            for d in range(dim):
                vg = sg[:, g, None] * phif[None, :, g] / detf
                term = vg * Jf[:, :, d, cg] * nw[:, :, d]
                mag = np.abs(vg) * SJf[:, :, d, cg] * Scof[:, :, d, ck] * fw[None, :]
                coef[:, 1 + g, NI + k] += term.sum(1)
                S[:, 1 + g, NI + k] += mag.sum(1)
                coef[:, NI + k, 1 + g] -= term.sum(1)
                S[:, NI + k, 1 + g] += mag.sum(1)
    full = np.concatenate([state, lam], axis=1)
    val = np.einsum("erc,ec->er", coef, full)
    S_val = np.einsum("erc,ec->er", S, np.abs(full))
    val[:, 0] += data
    S_val[:, 0] += S_data
    return dict(res=-val, blocks=coef, S_res=S_val, S_blocks=S)


def solve_batched(A, B):
    """X with A X = B for stacks A [E][m][m], B [E][m][r]: Gaussian elimination with partial pivoting in A's type."""
    A, B = A.copy(), B.copy()
    E, m, _ = A.shape
    ar = np.arange(E)
    for j in range(m):
        piv = j + np.argmax(np.abs(A[:, j:, j]), axis=1)
        for M in (A, B):
            tmp = M[ar, piv].copy()
            M[ar, piv] = M[:, j]
            M[:, j] = tmp
        for i in range(j + 1, m):
            fct = A[:, i, j] / A[:, j, j]
            A[:, i, :] -= fct[:, None] * A[:, j, :]
            B[:, i, :] -= fct[:, None] * B[:, j, :]
    X = np.empty_like(B)
    for i in range(m - 1, -1, -1):
        X[:, i, :] = (B[:, i, :] - np.einsum("ek,ekr->er", A[:, i, i + 1:], X[:, i + 1:, :])) / A[:, i, i, None]
    return X


def condense(arr, n_int):
    """Static condensation as mha_batched_condense defines it, with the componentwise first-order scales
    S_X = |A_uu^-1| (S_[A_ul | r_u] + S_Auu |X|),  S_S = S_All + S_Alu |X| + |A_lu| S_X   (likewise g; du: S_X's last column)."""
    Bk, r, SB, Sr = arr["blocks"], arr["res"], arr["S_blocks"], arr["S_res"]
    ni = n_int
    E, n, _ = Bk.shape
    T = Bk.dtype.type
    Auu, Aul, Alu, All = Bk[:, :ni, :ni], Bk[:, :ni, ni:], Bk[:, ni:, :ni], Bk[:, ni:, ni:]
    rhs = np.concatenate([Aul, r[:, :ni, None]], axis=2)
    S_rhs = np.concatenate([SB[:, :ni, ni:], Sr[:, :ni, None]], axis=2)
    X = solve_batched(Auu, rhs)
    inv = solve_batched(Auu, np.broadcast_to(np.eye(ni, dtype=T), (E, ni, ni)).copy())
    S_X = np.einsum("eij,ejr->eir", np.abs(inv), S_rhs + np.einsum("eij,ejr->eir", SB[:, :ni, :ni], np.abs(X)))
    low = np.concatenate([All, r[:, ni:, None]], axis=2)
    S_low = np.concatenate([SB[:, ni:, ni:], Sr[:, ni:, None]], axis=2)
    out = low - np.einsum("eai,eir->ear", Alu, X)
    S_out = S_low + np.einsum("eai,eir->ear", SB[:, ni:, :ni], np.abs(X)) + np.einsum("eai,eir->ear", np.abs(Alu), S_X)
    return dict(schur=out[:, :, :-1], gvec=out[:, :, -1], du=X[:, :, -1], S_schur=S_out[:, :, :-1], S_gvec=S_out[:, :, -1],
                S_du=S_X[:, :, -1], cond=np.array([np.linalg.cond(a) for a in Auu.astype(np.float64)]))


def distance(got, ref, S):
    """Largest d = |got - ref| / (2^-53 S) over the entries; where S == 0 the entry must be exactly 0.0 (else inf); a
    value that is not finite counts as infinite.  -> (d, flat index)."""
    got = np.asarray(got, np.float64)
    ref, S = np.asarray(ref), np.asarray(S)
    err = np.abs(got.astype(LD) - ref.astype(LD))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(S > 0, err / (LD(U) * S.astype(LD)), np.where(got == 0.0, LD(0), LD(np.inf)))
    d = np.where(np.isfinite(got), d, LD(np.inf)).astype(np.float64)
    if d.size == 0:
        return 0.0, -1
    k = int(np.argmax(d))
    return float(d.ravel()[k]), k


# ---- functions of the decks ------------------------------------------------------------------------------------------
def const_kinv(vals):
    return lambda x: np.broadcast_to(np.asarray(vals, np.float64)[:x.shape[2]].astype(x.dtype), x.shape)


def element_kinv(edata):
    """'use permeability data': Kinv_dd = 1 / data(elem, 0)."""
    return lambda x: np.broadcast_to((1 / np.asarray(edata, np.float64).astype(x.dtype))[:, None, None], x.shape)


def deck_kinv(x):
    """Kinv_xx: '1.0+x*x+y', Kinv_yy = Kinv_zz = 1."""
    K = np.ones(x.shape, x.dtype)
    K[:, :, 0] = 1 + x[:, :, 0] * x[:, :, 0] + x[:, :, 1]
    return K


def pi_of(x):
    return x.dtype.type(np.pi)  # the deck's `pi` is the double constant


def deck_source(x):
    """source: 'sin(2*pi*x)*y'."""
    return np.sin(2 * pi_of(x) * x[:, :, 0]) * x[:, :, 1]


def gold_source(x):
    """The decks' source: 8 pi^2 sin(2 pi x) sin(2 pi y) in 2-D, 12 pi^2 sin sin sin in 3-D."""
    dim, pi = x.shape[2], pi_of(x)
    return 4 * dim * (pi * pi) * np.prod(np.sin(2 * pi * x), axis=2)


def gold_true(x):
    """p = lambda = prod sin(2 pi x_d); u = -grad p."""
    dim, pi = x.shape[2], pi_of(x)
    s, c = np.sin(2 * pi * x), np.cos(2 * pi * x)
    p = np.prod(s, axis=2)
    u = np.stack([-2 * pi * c[:, :, d] * np.prod(np.delete(s, d, axis=2), axis=2) for d in range(dim)], axis=2)
    return p, u


# ---- whole mesh ----------------------------------------------------------------------------------------------------
def trace_system(schur, gvec, trace_lids, ntrace, fixed):
    """Dense trace matrix and right-hand side from the condensed element arrays; fixed rows: identity, zero."""
    E, nt = trace_lids.shape
    M, rhs = np.zeros((ntrace, ntrace)), np.zeros(ntrace)
    for a in range(nt):
        np.add.at(rhs, trace_lids[:, a], gvec[:, a])
        for b in range(nt):
            np.add.at(M, (trace_lids[:, a], trace_lids[:, b]), schur[:, a, b])
    fx = np.asarray(fixed, bool)
    M[fx, :] = 0.0
    M[fx, fx] = 1.0
    rhs[fx] = 0.0
    return M, rhs


def solve_mesh(mesh, kinv, source, lam0, nq1=2):
    """The two-call solve in float64 on the yardstick: step at (0, lam0), trace solve with the boundary rows fixed, step
    again, u += du.  mesh: dict of mrhyde_amd.mesh_porous_hybrid form.  lam0 [ntrace]: zero but for the Dirichlet values.
    -> (state [E][1 + 2 dim], lam [ntrace], gvec of the second step)."""
    E, dim = mesh["nelem"], mesh["dim"]
    NI = 1 + 2 * dim
    orient = mesh["orient"][:, 1:]
    tl, fixed = mesh["trace_lids"], mesh["trace_side"] != 0
    state, lam = np.zeros((E, NI)), np.array(lam0, np.float64)
    c = condense(element_blocks(mesh["nodes"], orient, state, lam[tl], kinv, source, np.float64, nq1), NI)
    M, rhs = trace_system(c["schur"], c["gvec"], tl, mesh["ntrace"], fixed)
    lam = lam + np.linalg.solve(M, rhs)
    c = condense(element_blocks(mesh["nodes"], orient, state, lam[tl], kinv, source, np.float64, nq1), NI)
    return state + c["du"], lam, c["gvec"]


def errors(mesh, state, lam, true=gold_true, nq1=2):
    """The reference's three error loops (PostprocessManager::computeError, src/managers/postprocessManager.cpp:1255-1268
    "L2", :1385-1434 "L2 VECTOR", :1437-1473 "L2 FACE") from element states [E][1 + 2 dim] and traces lam [ntrace]:
    sqrt(sum (p_h - p)^2 w), sqrt(sum_d sum (u_h,d - u_d)^2 w) at the volume points, and, per (element, face),
    0.5 / |F| sum (lambda_h - lambda)^2 w at the side points with |F| = sum w -- summed over all elements and all faces,
    so an interior face enters twice with half weight; then the square root."""
    nodes = np.asarray(mesh["nodes"], np.float64)
    E, _, dim = nodes.shape
    NU = 2 * dim
    sg = mesh["orient"][:, 1:].astype(np.float64)
    pts, wref = tensor_rule(dim, nq1, np.float64)
    x, J = geometry(nodes, pts)
    det, _ = det_cof(J)
    w = wref[None, :] * det
    phi, _ = rt0(pts, dim)
    pt, ut = true(x)
    ep = np.sum((state[:, 0, None] - pt) ** 2 * w)
    uh = np.zeros(x.shape)
    for f in range(NU):
        uh += (state[:, 1 + f] * sg[:, f])[:, None, None] * (phi[None, :, f] / det)[:, :, None] * J[:, :, :, f >> 1]
    eu = np.sum(np.sum((uh - ut) ** 2, axis=2) * w)
    ef = 0.0
    for k in range(NU):
        ck, _ = face_dir(k)
        fp, fw = face_rule(dim, k, nq1, np.float64)
        xf, Jf = geometry(nodes, fp)
        _, cof = det_cof(Jf)
        wf = np.sqrt(np.sum(cof[:, :, :, ck] ** 2, axis=2)) * fw[None, :]
        lt, _ = true(xf)
        lh = lam[mesh["trace_lids"][:, k]]
        ef += np.sum(0.5 / wf.sum(1) * np.sum((lh[:, None] - lt) ** 2 * wf, axis=1))
    return np.sqrt(ep), np.sqrt(eu), np.sqrt(ef)


def face_centroids(mesh):
    """Centroid of face k of every element [E][2 dim][dim], from the vertices alone."""
    nodes = np.asarray(mesh["nodes"], np.float64)
    dim = nodes.shape[2]
    sg = vertex_signs(dim)
    out = np.zeros((nodes.shape[0], 2 * dim, dim))
    for k in range(2 * dim):
        c, s = face_dir(k)
        out[:, k] = nodes[:, sg[:, c] == (1 if s else -1)].mean(axis=1)
    return out


# ---- input families of the tests --------------------------------------------------------------------------------------
def warp(mesh, amp=0.18, seed=5):
    """Interior vertices displaced by up to amp of the cell size (non-affine cells); boundary vertices stay."""
    nodes = np.array(mesh["nodes"], np.float64)
    dim = nodes.shape[2]
    flat = nodes.reshape(-1, dim)
    key = np.round(flat * 4096).astype(np.int64)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    rng = np.random.default_rng(seed)
    lo, hi = flat.min(0), flat.max(0)
    h = (nodes.max(1) - nodes.min(1)).min(0)
    disp = rng.uniform(-amp, amp, uniq.shape) * h[None, :]
    pos = uniq / 4096.0
    disp[np.any((np.abs(pos - lo) < 1e-9) | (np.abs(pos - hi) < 1e-9), axis=1)] = 0.0
    out = dict(mesh)
    out["nodes"] = (flat + disp[inv]).reshape(nodes.shape)
    return out


def random_state(mesh, seed):
    rng = np.random.default_rng(seed)
    E, dim = mesh["nelem"], mesh["dim"]
    return rng.uniform(-1, 1, (E, 1 + 2 * dim)), rng.uniform(-1, 1, mesh["ntrace"])


GEOMETRIES = ("2d 3x5 unit", "2d 3x5 warped", "2d 4x4 stretched", "3d 3x2x2 unit", "3d 3x2x2 warped", "3d 67x1x1")
COEFFICIENTS = ("constant", "element data", "deck strings")
KINV_CONSTANT, SOURCE_CONSTANT = (1.5, 0.75, 2.25), 0.7


def make_mesh(name, mesh_porous_hybrid):
    """The mesh of a geometry name, by the library's host-only generator (passed in: this module imports no library)."""
    dims = tuple(int(v) for v in name.split()[1].split("x"))
    if "stretched" in name:
        return mesh_porous_hybrid(dims, hi=(1.0, 1.0e-3))  # cells 1 : 1000
    m = mesh_porous_hybrid(dims)
    return warp(m) if "warped" in name else m


def coefficients(kind, mesh, seed=11):
    """-> (kinv(x), source(x), element data or None) of a coefficient family on a mesh."""
    if kind == "constant":
        return const_kinv(KINV_CONSTANT), (lambda x: np.full(x.shape[:2], SOURCE_CONSTANT, x.dtype)), None
    if kind == "element data":
        edata = 10.0 ** np.random.default_rng(seed).uniform(-3, 3, mesh["nelem"])  # permeabilities spanning 1e-3 .. 1e3
        return element_kinv(edata), (lambda x: np.full(x.shape[:2], SOURCE_CONSTANT, x.dtype)), edata
    assert kind == "deck strings"
    return deck_kinv, deck_source, None


def family(geometry, kind):
    """Input family of a case: the geometry class and the coefficient kind.  The row of 67 hexes has cells of 1/67 at
    coordinates up to 1: the cell Jacobian, a difference of vertex coordinates, carries 67 round-offs; it is a class of
    its own so that its constant does not loosen the others'."""
    return ("stretched" if "stretched" in geometry else "row of 67" if "67" in geometry else "regular", kind)


# K: the largest d of the float64 yardstick against the 80-bit one per input family, measured by
# tests/test_porous_hybrid.py and recorded as the next integer above 1.25 times the measurement (numpy's float64 sums
# follow the CPU's vector units); that test fails when a measurement exceeds its constant, or when a family's largest
# falls below a quarter of a constant above 1.  The device bound is max(8 K, 8).  "blocks": res and blocks of the plain
# kernel; "condensed": schur, gvec, du on the componentwise scale, which carries the conditioning (every measurement is
# below 0.5).  Measured values and the conditioning are tabulated in profiles/porous_hybrid.md.
K_YARDSTICK = {
    ("regular", "constant"): dict(blocks=3, condensed=1),
    ("regular", "element data"): dict(blocks=2, condensed=1),
    ("regular", "deck strings"): dict(blocks=2, condensed=1),
    ("row of 67", "constant"): dict(blocks=27, condensed=1),
    ("row of 67", "element data"): dict(blocks=19, condensed=1),
    ("row of 67", "deck strings"): dict(blocks=11, condensed=1),
    ("stretched", "constant"): dict(blocks=2, condensed=1),
    ("stretched", "element data"): dict(blocks=4, condensed=1),
    ("stretched", "deck strings"): dict(blocks=4, condensed=1),
}
# Conditioning guard, asserted on every compared case: cond_2 of the interior block A_uu.  Measured: 2.0e6 on the cells
# stretched 1 : 1000 (constant Kinv; 1.1e6 and 1.8e6 with element data and deck strings), 6.5e5 with permeabilities
# spanning 1e-3 .. 1e3 on the regular meshes, 6.7e3 on the row of 67, at most 11 elsewhere.
COND_GUARD = 1.0e7


def bound(fam, group):
    return max(8.0 * K_YARDSTICK[fam][group], 8.0)
