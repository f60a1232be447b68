"""The extended-precision yardstick of porousMixed (HVOL p, lowest-order HDIV u): element arrays, global CRS values,
residuals and the weak-Dirichlet side term in numpy's 80-bit longdouble, beside every entry the SCALE of its own sum.

TEST INFRASTRUCTURE, the sibling of tests/highprec_ref.py, from which it takes the mpmath tables, the multilinear geometry,
`seeded`, `assemble`, `matvec`, `diagonal` and `distance`.  Of oracle/ and mrhyde_amd/ it uses the mesh's integer maps and
the caller's `orient` signs only (and, for the KL cases, the roots of mrhyde_amd.kl_expansion as input data).

Reference basis: phihat_{2c} = (1 - xi_c)/2 e_c, phihat_{2c+1} = (1 + xi_c)/2 e_c, divhat = -/+ 1/2; HVOL
is the constant 1.  Physical basis: v_i = s_i J phihat_i / det J, div_i = s_i divhat_i / det J with s_i = orient verbatim.

  R_{u,i} = sum_q (Kinv u . v_i / mobility - p div_i) w        R_p = sum_q (source - div u) w      (porousMixed.cpp:236-337)
  side:     R_{u,i} += sum_q bsource w_side (v_i . n)                                               (porousMixed.cpp:400-418)

u is the stage value; the module has no time derivative, so the matrix carries alpha_u only.  local_res = -R and
local_J = +dR/du as in the ABI.  The module is linear in (u, p): the derivative is the bilinear form itself.

The scales.  On an axis-aligned box the off-diagonal of J is exactly zero, so the cross-direction entries A_ij of an exact
geometry have S = 0, while every double-precision evaluation leaves round-off residue of J's off-diagonal there (2e-12
beside 1.8e4).  The scale therefore carries the geometry's own terms at absolute value:

  Jabs_dc(q)  = sum_v |x_d(v)| |dN_v/dxi_c(q)|
  Vabs_i(q)_d = sum_c Jabs_dc |phihat_{i,c}(q)| / det(q)       Dabs_i(q) = 1 / (2 det(q))
  S_A_ij      = alpha_u sum_q sum_d Vabs_{i,d} |Kinv_d / mob| Vabs_{j,d} w
  S_B_i       = alpha_u sum_q Dabs_i w                          (both the (u_i, p) and the (p, u_i) entry)
  S_res_{u,i} = sum_q (sum_d Vabs_{i,d} |Kinv_d u_d / mob| + Dabs_i |p|) w
  S_res_p     = sum_q |source - div u| w
  side        = sum_q |bsource| w_side sum_d Vabs_{i,d} |n_d|

(det and all field values the yardstick's own.)  p-p entries and fixed rows have S == 0 and must be exactly 0.0.
"""
import mpmath
import numpy as np

import highprec_ref as H

LD = np.longdouble
MODULE, BOUNDARY = "porousMixed", "porousMixed boundary"

# K_oracle[(module, family)] as tests/test_highprec_hdiv.py measures it: the C oracle's rule of highprec_ref.K_ORACLE
# (next integer at least one half above the measurement; above 1000 the next multiple of ten).
K_ORACLE = {
    (MODULE,   "unit"):              33,      # measured 31.927
    (MODULE,   "stretched aligned"): 36,      # measured 35.384
    (MODULE,   "stretched sheared"): 405,     # measured 403.74
    (MODULE,   "stretched warped"):  27,      # measured 26.497
    (MODULE,   "units small"):       36,      # measured 34.560
    (MODULE,   "units large"):       14,      # measured 12.672
    (MODULE,   "unit deck source"):  33,      # measured 31.927
    (MODULE,   "unit element data"): 33,      # measured 31.927
    (MODULE,   "unit KL"):           33,      # measured 31.927
    (MODULE,   "database shifted"):  1650,    # measured 1646.5
    (MODULE,   "database scaled"):   194,     # measured 192.51
    (MODULE,   "database sheared"):  522,     # measured 520.96
    (BOUNDARY, "unit"):              6,       # measured 4.8089
    (BOUNDARY, "stretched warped"):  6,       # measured 4.7940
}
H.K_ORACLE.update(K_ORACLE)


# ---- reference cell ------------------------------------------------------------------------------------------------------
def _vertex_signs(dim):
    """The reference vertices (+-1 per direction) in the cell's vertex order."""
    perm = H._vertex_perm(dim)
    return np.array([[1 if (t >> d) & 1 else -1 for d in range(dim)] for t in perm], dtype=LD)


def volume_points(dim, qdeg):
    """Reference coordinates xi [q][dim] of the tensor Gauss points (x fastest) and their weights [q]."""
    npts = H.gauss_npts(qdeg)
    x1, w1, _, _ = H.line_tables(1, npts)
    idx = np.indices((npts,) * dim).reshape(dim, -1)[::-1]            # row d: the 1-D index of direction d, x fastest
    xi = np.stack([x1[idx[d]] for d in range(dim)], axis=1)
    w = np.prod(np.stack([w1[idx[d]] for d in range(dim)], axis=1), axis=1)
    return xi, w


# The sides in the mesh's numbering (bottom, right, top, left, back, front): (direction, sign of the outward reference
# normal) and the side's own tangents; side point = centre + s * du + t * dv in reference coordinates, s fastest.  The order
# of a side's points is part of the interface (per-point boundary data [k][point]): the Gauss points of a line are
# numbered from the largest to the smallest.  tests/test_highprec_hdiv.py checks the placement against the mesh.
_SIDE_2D = [((1, -1), ((1, 0),)), ((0, 1), ((0, 1),)), ((1, 1), ((-1, 0),)), ((0, -1), ((0, -1),))]
_SIDE_3D = [((1, -1), ((1, 0, 0), (0, 0, 1))), ((0, 1), ((0, 1, 0), (0, 0, 1))), ((1, 1), ((-1, 0, 0), (0, 0, 1))),
            ((0, -1), ((0, 0, 1), (0, 1, 0))), ((2, -1), ((0, 1, 0), (1, 0, 0))), ((2, 1), ((1, 0, 0), (0, 1, 0)))]


def side_points(dim, qdeg, side):
    """xi [qs][dim] and reference weights [qs] of the side's tensor Gauss points, and (direction, sign) of its normal."""
    (c, sign), tang = (_SIDE_2D if dim == 2 else _SIDE_3D)[side]
    npts = H.gauss_npts(qdeg)
    x1, w1, _, _ = H.line_tables(1, npts)
    x1, w1 = x1[::-1], w1[::-1]
    idx = np.indices((npts,) * (dim - 1)).reshape(dim - 1, -1)[::-1]
    xi = np.zeros((idx.shape[1], dim), LD)
    xi[:, c] = sign
    w = np.ones(idx.shape[1], LD)
    for k, t in enumerate(tang):
        xi += x1[idx[k]][:, None] * np.array(t, dtype=LD)[None, :]
        w = w * w1[idx[k]]
    return xi, w, c, sign


def vertex_functions(dim, xi):
    """Multilinear vertex functions at xi [q][dim]: NV [v][q], NG [v][q][dim]."""
    sg = _vertex_signs(dim)                                            # [v][dim]
    f = (1 + sg[:, None, :] * xi[None, :, :]) / 2                      # [v][q][dim]
    NV = np.prod(f, axis=2)
    NG = np.zeros(f.shape, LD)
    for c in range(dim):
        g = sg[:, None, c] / 2
        for d in range(dim):
            if d != c:
                g = g * f[:, :, d]
        NG[:, :, c] = g
    return NV, NG


def hdiv_reference(dim, xi):
    """phihat [2 dim][q] (the one non-zero component, direction i // 2) and divhat [2 dim]."""
    ph = np.zeros((2 * dim, xi.shape[0]), LD)
    dv = np.zeros(2 * dim, LD)
    for c in range(dim):
        ph[2 * c], ph[2 * c + 1] = (1 - xi[:, c]) / 2, (1 + xi[:, c]) / 2
        dv[2 * c], dv[2 * c + 1] = LD(-0.5), LD(0.5)
    return ph, dv


class PointTables:
    """Physical tables of the elements `nodes` [E][2^dim][dim] with signs s [E][2 dim] at reference points xi:
    x [E][q][dim], det [E][q], Jinv, V [E][i][q][dim], D [E][i][q] and the absolute tables Vabs, Dabs."""

    def __init__(self, nodes, s, xi):
        X = np.asarray(nodes).astype(LD)
        dim = X.shape[2]
        NV, NG = vertex_functions(dim, xi)
        self.x = np.einsum("evd,vq->eqd", X, NV)
        J = np.einsum("evd,vqc->eqdc", X, NG)
        Jabs = np.einsum("evd,vqc->eqdc", np.abs(X), np.abs(NG))
        self.det, self.Jinv = H.cofactor_inverse(J)
        assert np.all(self.det > 0)
        ph, dv = hdiv_reference(dim, xi)
        s = np.asarray(s).astype(LD)
        ci = np.arange(2 * dim) // 2
        Jc, Jac = np.transpose(J[:, :, :, ci], (0, 3, 1, 2)), np.transpose(Jabs[:, :, :, ci], (0, 3, 1, 2))   # [E][i][q][d]
        self.V = s[:, :, None, None] * Jc * ph[None, :, :, None] / self.det[:, None, :, None]
        self.Vabs = Jac * np.abs(ph)[None, :, :, None] / self.det[:, None, :, None]
        self.Vexact = np.abs(self.V)                                   # the exact-geometry scale, for the record only
        self.D = s[:, :, None] * dv[None, :, None] / self.det[:, None, :]
        self.Dabs = np.broadcast_to(1 / (2 * self.det[:, None, :]), self.D.shape)


class HdivBlock:
    """m: a mesh dict of tests/oracle_lib.py's mesh_multi layout with variables (HVOL 0, HDIV 1)."""

    def __init__(self, m, qdeg):
        self.nodes = np.asarray(m["nodes"], dtype=np.float64)
        self.lids = np.asarray(m["lids"])
        self.E, self.n = self.lids.shape
        self.dim = dim = self.nodes.shape[2]
        self.ndof, self.qdeg = int(m["ndof"]), qdeg
        off, vp = np.asarray(m["offsets"]), np.asarray(m["varptr"])
        assert self.n == 1 + 2 * dim and vp[1] - vp[0] == 1 and vp[2] - vp[1] == 2 * dim
        self.pp, self.up = int(off[vp[0]]), off[vp[1]:vp[2]]         # LID positions of p and of u_i
        self.s = np.asarray(m["orient"])[:, vp[1]:vp[2]].astype(np.int64)
        assert np.all(np.abs(self.s) == 1)
        self.xi, self.wref = volume_points(dim, qdeg)
        rt = H.ref_tables(dim, 1, qdeg)                                # the tables of the HGRAD yardstick: the same points
        NV, NG = vertex_functions(dim, self.xi)
        assert np.abs(NV - rt["NV"]).max() < 4e-19 and np.abs(NG - rt["NG"]).max() < 4e-19 and np.abs(self.wref - rt["w"]).max() < 4e-19
        self.pt = PointTables(self.nodes, self.s, self.xi)
        self.w = self.wref[None, :] * self.pt.det
        self.nq = self.w.shape[1]

    seeded = H.Block.seeded

    def side_tables(self, elems, side):
        """PointTables of the elements `elems` at the points of local side `side`, the unit normals n [k][qs][dim] and
        the side weights [k][qs]: n w_side = w_ref det J^-T nhat (the cofactor column), of the yardstick's own making."""
        xi, w, c, sign = side_points(self.dim, self.qdeg, side)
        pt = PointTables(self.nodes[elems], self.s[elems], xi)
        nvec = sign * pt.det[..., None] * pt.Jinv[:, :, c, :]         # det J^-T nhat
        area = np.sqrt((nvec * nvec).sum(axis=2))
        return pt, nvec / area[..., None], w[None, :] * area, (xi, w, c, sign)

    # -- its own checks -------------------------------------------------------------------------------------------------
    def check_fluxes(self):
        """(a) the flux of v_i through its own physical face is s_i (-/+ 1) 2^(dim-1), through every other face 0, and
        sum_q div_i w equals the sum of its face fluxes (the Piola map preserves flux); (b) on every interior face row
        the outward fluxes of the two incident elements cancel.  Returns the own-face fluxes [E][2 dim]."""
        dim, E = self.dim, self.E
        sides = _SIDE_2D if dim == 2 else _SIDE_3D
        flux = np.zeros((E, 2 * dim, 2 * dim), LD)                     # [e][i][face f = 2 c + (sign > 0)]
        for sd in range(2 * dim):
            pt, n, ws, (_, _, c, sign) = self.side_tables(np.arange(E), sd)
            assert sides[sd][0] == (c, sign)
            flux[:, :, 2 * c + (sign > 0)] = np.einsum("eiqd,eqd,eq->ei", pt.V, n, ws)
        full = LD(2) ** (dim - 1)
        want = np.zeros_like(flux)
        for i in range(2 * dim):
            want[:, i, i] = self.s[:, i] * (1 if i % 2 else -1) * full
        assert np.abs(flux - want).max() <= 1e-15 * float(full), "a basis function's face fluxes"
        div = np.einsum("eiq,eq->ei", self.pt.D, self.w)
        assert np.abs(div - flux.sum(axis=2)).max() <= 1e-15 * float(full), "divergence theorem of a basis function"
        own = np.einsum("eii->ei", flux)
        rows = self.lids[:, self.up]
        total, count = np.zeros(self.ndof, LD), np.zeros(self.ndof, np.int64)
        np.add.at(total, rows, own)
        np.add.at(count, rows, 1)
        assert count.max() <= 2 and np.all(count[np.unique(rows)] >= 1)
        assert (count == 2).any(), "no interior face"
        assert np.abs(total[count == 2]).max() <= 1e-15 * float(full), "outward fluxes of an interior face do not cancel"
        assert np.all(np.abs(total[count == 1]) > 0.5 * float(full))
        return own

    def check_constant_field(self, a=(0.7, -1.3, 0.45)):
        """(c) affine elements only: the interpolant of the constant vector a (dof_i = flux of a through face i over
        the flux of v_i) comes out of the tables as a at every point, with zero divergence.  Returns the two errors
        relative to |a|; the caller holds them to its tolerance."""
        dim, E = self.dim, self.E
        a = np.array(a, LD)[:dim]
        dof = np.zeros((E, 2 * dim), LD)
        for sd in range(2 * dim):
            pt, n, ws, (_, _, c, sign) = self.side_tables(np.arange(E), sd)
            i = 2 * c + (sign > 0)
            dof[:, i] = np.einsum("eqd,d,eq->e", n, a, ws) / np.einsum("eqd,eqd,eq->e", pt.V[:, i], n, ws)
        val = np.einsum("eiqd,ei->eqd", self.pt.V, dof)
        dv = np.einsum("eiq,ei->eq", self.pt.D, dof)
        size = (self.nodes.max(axis=1) - self.nodes.min(axis=1)).min()
        amax = float(np.abs(a).max())
        return float(np.abs(val - a).max()) / amax, float(np.abs(dv).max()) * float(size) / amax


# ---- functions of the deck --------------------------------------------------------------------------------------------------
def func_value(spec, x):
    """A number, ("sinprod", amp, freq), ("array", a [E][q]) or an array [E][q] at the points x [E][q][dim]."""
    if isinstance(spec, np.ndarray):
        return spec.astype(LD)
    if isinstance(spec, tuple) and spec[0] == "array":
        return np.asarray(spec[1]).astype(LD)
    return H.func_value(spec, x) + np.zeros(x.shape[:2], LD)


def kl_log_field(x, kl, roots, uq, stoch):
    """updateKLPerm (porousMixed.cpp:567-714) in longdouble at x [E][q][dim], with the 3-D terms as the deck's
    fix_KL_3d = 1 states them (every component the same product of three directions).  kl: per direction dict(N, L,
    sigma, eta); roots: per direction the roots omega (input data: the reference defines them by a 1e-10 Newton stop).
    Total-order multi-indices: by i + j + k, then k, then j, then i (KLindices)."""
    dim = x.shape[2]
    N = [k["N"] for k in kl] + [1] * (3 - dim)
    idx = [(i, j, k) for a in range(sum(N)) for k in range(N[2]) for j in range(N[1]) for i in range(N[0]) if i + j + k == a]
    assert len(idx) == N[0] * N[1] * N[2]
    om = [np.asarray(r).astype(LD) for r in roots]
    lam = [2 * LD(k["eta"]) * LD(k["sigma"]) ** 2 / (LD(k["eta"]) ** 2 * o * o + 1) for k, o in zip(kl, om)]

    def phi(d, i):
        w, eta, L = om[d][i], LD(kl[d]["eta"]), LD(kl[d]["L"])
        return (eta * w * np.cos(w * x[..., d]) + np.sin(w * x[..., d])) / np.sqrt((eta * eta * w * w + 1) * L / 2 + eta)

    coef = [None] * len(idx)
    prog = 0
    if uq is not None:
        for t in range(min(len(uq), len(idx))):
            coef[t] = LD(uq[t])
        prog = len(uq)
    if stoch is not None:
        for t in range(prog, min(len(idx), prog + len(stoch))):
            coef[t] = LD(stoch[t - prog])
    out = np.zeros(x.shape[:2], LD)
    for t, c in enumerate(coef):
        if c is None:
            continue
        ev, lm = LD(1), LD(1)
        for d in range(dim):
            ev, lm = ev * phi(d, idx[t][d]), lm * lam[d][idx[t][d]]
        out = out + c * np.sqrt(lm) * ev
    return out


def coefficients(blk, P):
    """Kinv [dim][E][q], mobility [E][q], source [E][q] of the case's parameters at the block's points."""
    x, dim = blk.pt.x, blk.dim
    kinv = [func_value(P["Kinv"][d], x) for d in range(dim)]
    if P.get("edata") is not None:                                       # updatePerm (:550-563): Kinv = 1 / element data
        kinv = [np.repeat(1 / np.asarray(P["edata"]).astype(LD)[:, None], blk.nq, axis=1) for _ in range(dim)]
    if P.get("kl") is not None:                                          # :198-216: Kinv / exp(KL)
        f = kl_log_field(x, P["kl"], P["kl_roots"], P.get("uq"), P.get("stoch"))
        kinv = [k / np.exp(f) for k in kinv]
    return kinv, func_value(P["mobility"], x), func_value(P["source"], x)


# ---- element arrays and their scales --------------------------------------------------------------------------------------
def element_arrays(blk, P, u, tr=None, exact_scale=False):
    """-> dict(local_res, local_J, S_res, S_J) in LID-position order.  exact_scale: the scales from |V| of the exact
    geometry instead of Vabs (printed for the record, never asserted)."""
    ue, _, alpha_u, _ = blk.seeded(u, tr)
    kinv, mob, src = coefficients(blk, P)
    E, n, dim, pt, w = blk.E, blk.n, blk.dim, blk.pt, blk.w
    uu, pe = ue[blk.lids[:, blk.up]], ue[blk.lids[:, blk.pp]]        # [E][2 dim], [E]
    Ki = np.stack(kinv, axis=-1) / mob[..., None]                         # [E][q][dim]
    uq = np.einsum("eiqd,ei->eqd", pt.V, uu)
    divu = np.einsum("eiq,ei->eq", pt.D, uu)
    Va = pt.Vexact if exact_scale else pt.Vabs
    Ru = np.einsum("eiqd,eqd,eq->ei", pt.V, Ki * uq, w) - np.einsum("eiq,eq->ei", pt.D, w) * pe[:, None]
    Rp = ((src - divu) * w).sum(axis=1)
    A = alpha_u * np.einsum("eiqd,eqd,ejqd,eq->eij", pt.V, Ki, pt.V, w)
    B = -alpha_u * np.einsum("eiq,eq->ei", pt.D, w)
    S_Ru = np.einsum("eiqd,eqd,eq->ei", Va, np.abs(Ki * uq), w) + np.einsum("eiq,eq->ei", pt.Dabs, w) * np.abs(pe)[:, None]
    S_Rp = (np.abs(src - divu) * w).sum(axis=1)
    S_A = alpha_u * np.einsum("eiqd,eqd,ejqd,eq->eij", Va, np.abs(Ki), Va, w)
    S_B = alpha_u * np.einsum("eiq,eq->ei", pt.Dabs, w)
    out = {k: np.zeros((E, n, n) if k.endswith("J") else (E, n), LD) for k in ("local_res", "local_J", "S_res", "S_J")}
    up, pp = blk.up, blk.pp
    out["local_res"][:, up], out["local_res"][:, pp] = -Ru, -Rp
    out["S_res"][:, up], out["S_res"][:, pp] = S_Ru, S_Rp
    for name, a, b in (("local_J", A, B), ("S_J", S_A, S_B)):
        out[name][:, up[:, None], up[None, :]] = a
        out[name][:, up, pp] = b
        out[name][:, pp, up] = b
    return out


def boundary_arrays(blk, groups, fixed=None):
    """The weak-Dirichlet term of the groups [(elems, sides, bsource spec)] -> global (res, S_res): res holds -R.  The
    term does not depend on the solution: its matrix is exactly zero."""
    res, S = np.zeros(blk.ndof, LD), np.zeros(blk.ndof, LD)
    free = np.ones(blk.ndof, bool) if fixed is None else ~np.asarray(fixed, bool)
    for elems, sides, spec in groups:
        elems, sides = np.asarray(elems), np.asarray(sides)
        assert len(set(sides.tolist())) == 1
        pt, n, ws, _ = blk.side_tables(elems, int(sides[0]))
        bs = func_value(spec, pt.x)
        r = np.einsum("kq,kq,kiqd,kqd->ki", bs, ws, pt.V, n)
        s = np.einsum("kq,kq,kiqd,kqd->ki", np.abs(bs), ws, pt.Vabs, np.abs(n))
        rows = blk.lids[elems][:, blk.up]
        np.add.at(res, rows[free[rows]], -r[free[rows]])
        np.add.at(S, rows[free[rows]], s[free[rows]])
    return res, S


# ---- (d) one element against mpmath alone ------------------------------------------------------------------------------------
def element_arrays_mp(nodes, s, qdeg, kinv, mob, src, ue, pe, dps=50):
    """A [i][j], B [i], Ru [i], Rp of ONE element in mpmath at `dps` digits with plain loops: Gauss points from the roots
    of P_n at that precision, the multilinear map, Piola values.  src = ("sinprod", amp, freq)."""
    mp = mpmath
    with mp.workdps(dps):
        dim = len(nodes[0])
        xs, ws = H.gauss_mp.__wrapped__(H.gauss_npts(qdeg))
        sg = [[int(v) for v in row] for row in _vertex_signs(dim)]
        X = [[mp.mpf(float(c)) for c in v] for v in nodes]
        nu = 2 * dim
        A = [[mp.mpf(0)] * nu for _ in range(nu)]
        B, Ru, Rp = [mp.mpf(0)] * nu, [mp.mpf(0)] * nu, mp.mpf(0)
        pts = [[]]
        for _ in range(dim):
            pts = [[k] + p for k in range(len(xs)) for p in pts]       # the x index runs fastest
        for p in pts:
            xi = [xs[k] for k in p]
            wq = mp.mpf(1)
            for k in p:
                wq *= ws[k]
            J = mp.zeros(dim, dim)
            x = [mp.mpf(0)] * dim
            for v in range(2 ** dim):
                f = [(1 + sg[v][d] * xi[d]) / 2 for d in range(dim)]
                N = mp.mpf(1)
                for d in range(dim):
                    N *= f[d]
                for d in range(dim):
                    x[d] += X[v][d] * N
                    for c in range(dim):
                        g = mp.mpf(sg[v][c]) / 2
                        for k in range(dim):
                            if k != c:
                                g *= f[k]
                        J[d, c] += X[v][d] * g
            det = mp.det(J)
            w = wq * det
            V, D = [], []
            for i in range(nu):
                c = i // 2
                ph = (1 + xi[c]) / 2 if i % 2 else (1 - xi[c]) / 2
                V.append([s[i] * J[d, c] * ph / det for d in range(dim)])
                D.append(s[i] * (mp.mpf(1) if i % 2 else mp.mpf(-1)) / 2 / det)
            f = mp.mpf(src[1])
            for d in range(dim):
                f *= mp.sin(mp.mpf(src[2][d]) * x[d])
            uq = [sum(V[i][d] * mp.mpf(float(ue[i])) for i in range(nu)) for d in range(dim)]
            divu = sum(D[i] * mp.mpf(float(ue[i])) for i in range(nu))
            Ki = [mp.mpf(kinv[d]) / mp.mpf(mob) for d in range(dim)]
            Rp += (f - divu) * w
            for i in range(nu):
                Ru[i] += (sum(Ki[d] * uq[d] * V[i][d] for d in range(dim)) - mp.mpf(float(pe)) * D[i]) * w
                B[i] += -D[i] * w
                for j in range(nu):
                    A[i][j] += sum(V[i][d] * Ki[d] * V[j][d] for d in range(dim)) * w
        ld = H._ld
        return (np.array([[ld(a) for a in row] for row in A]), np.array([ld(b) for b in B]), np.array([ld(r) for r in Ru]), ld(Rp))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
SHAPES = [("2-D 3x2", 2, (3, 2)), ("3-D 2x2x2", 3, (2, 2, 2)), ("3-D 3x2x1", 3, (3, 2, 1))]
GEOMETRY = H.FAMILIES                                                    # the six families of map_vertices
EXTRA = ["unit deck source", "unit element data", "unit KL"]
DATABASE = ["database shifted", "database scaled", "database sheared"]
DATABASE_SHAPES = [("3-D 64x2x4", 3, (64, 2, 4)), ("2-D 128x4", 2, (128, 4))]
BOUNDARY_FAMILIES = ["unit", "stretched warped"]
KL3 = [dict(N=3, L=1.0, sigma=1.0, eta=0.3), dict(N=4, L=1.2, sigma=1.0, eta=0.5), dict(N=2, L=0.9, sigma=1.0, eta=0.2)]
AFFINE = ("stretched aligned", "stretched sheared") + tuple(DATABASE)


def shapes(family):
    return DATABASE_SHAPES if family in DATABASE else SHAPES


def qdegs(family):
    """Quadrature 2 everywhere; quadrature 4 (27 points on a hex) on the unit and stretched-aligned families."""
    return (2, 4) if family in ("unit", "stretched aligned") else (2,)


def geometry_family(family):
    return "unit" if family in EXTRA else family


def database_vertices(v, family):
    """Exactly uniform meshes with dyadic coordinates (unit spacing from mesh_multi with hi = ncell), so that every
    element's vertex offsets are bit-identical."""
    dim = v.shape[1]
    assert np.array_equal(v, np.round(v))
    if family == "database shifted":
        return v + 3.0
    if family == "database scaled":
        return v * np.array([1.0, 2.0 ** -10, 1.0])[:dim]
    A = np.eye(dim) + 0.25 * np.array([[0, 3, -1], [-2, 1, 2], [1, -1, 0]])[:dim, :dim]   # multiples of 1/4: not axis-aligned
    return v @ A.T


def flip_orientations(m, rng, rate=0.3):
    """Consistent random flips per global face dof: the signs are the caller's, taken verbatim."""
    flip = rng.uniform(size=m["ndof"]) < rate
    u0 = m["varptr"][1]
    for e in range(m["nelem"]):
        for f in range(2 * m["dim"]):
            if flip[m["lids"][e, m["offsets"][u0 + f]]]:
                m["orient"][e, u0 + f] *= -1


_CASES = {}


def build_case(meshlib, family, shape, qdeg, transient, kl_roots=None):
    """One volume case, cached: mesh, data, the yardstick's element arrays `el` and global arrays `g` (H.assemble).
    kl_roots(N, L, sigma, eta) -> roots: needed by the KL family only."""
    key = (family, shape, qdeg, transient)
    if key in _CASES:
        return _CASES[key]
    name, dim, ncell = shape
    rng = np.random.default_rng(131)
    db = family in DATABASE
    m = meshlib.mesh_multi(dim, ncell, [meshlib.HVOL, meshlib.HDIV], [0, 1], hi=[float(c) for c in ncell] + [1.0] * (3 - dim) if db else None)
    if db:
        m["verts"] = database_vertices(m["verts"], family)               # uniform signs: no flips
        fixed = (rng.uniform(size=m["ndof"]) < 0.02).astype(np.uint8)
    else:
        m["verts"] = H.map_vertices(m["verts"], geometry_family(family))
        flip_orientations(m, rng)
        fixed = ((m["side_mask"] & 0b1100) != 0).astype(np.uint8)        # strong Dirichlet rows on two sides
    m["nodes"] = np.ascontiguousarray(m["verts"][m["cell2vert"]])
    L = {"units small": 1e-3, "units large": 1e3}.get(family, 1.0)
    coef = {"units small": 1e6, "units large": 1e-6}.get(family, 1.0)
    amp = 1e3 if family.startswith("units") else 1.0
    u = amp * rng.uniform(-1, 1, m["ndof"])
    tr = None
    if transient:
        tr = dict(H.TABLEAU, dt=0.05, u_prev=amp * rng.uniform(-1, 1, (m["ndof"], 2)), u_stage=amp * rng.uniform(-1, 1, (m["ndof"], 2)))
    fr = [f / L for f in ((0.11, 0.7, 1.9) if db else (1.3, 0.7, 2.1))[:dim]]
    P = dict(Kinv=[k * coef for k in (1.3, 0.7, 2.1)], mobility=1.9, source=("sinprod", 2.0 * amp / L, fr))
    if family == "unit element data":
        P["edata"] = rng.uniform(0.2, 5.0, m["nelem"])
    if family == "unit KL":
        P["kl"] = KL3[:dim]
        P["kl_roots"] = [kl_roots(k["N"], k["L"], k["sigma"], k["eta"]) for k in P["kl"]]
        P["uq"], P["stoch"] = rng.normal(0, 1, 5), rng.normal(0, 1, int(np.prod([k["N"] for k in P["kl"]])))
    blk = HdivBlock(m, qdeg)
    el = element_arrays(blk, P, u, tr)
    c = dict(module=MODULE, family=family, shape=shape, m=m, dim=dim, qdeg=qdeg, u=u, tr=tr, P=P, fixed=fixed, blk=blk, el=el,
             g=H.assemble(blk, el, fixed))
    _CASES[key] = c
    return c


def build_boundary_case(meshlib, family, shape):
    """All 2 dim sides as weak-Dirichlet groups, alternating sinprod and per-point arrays; cached."""
    key = ("boundary", family, shape)
    if key in _CASES:
        return _CASES[key]
    name, dim, ncell = shape
    rng = np.random.default_rng(137)
    m = meshlib.mesh_multi(dim, ncell, [meshlib.HVOL, meshlib.HDIV], [0, 1])
    m["verts"] = H.map_vertices(m["verts"], family)
    flip_orientations(m, rng)
    m["nodes"] = np.ascontiguousarray(m["verts"][m["cell2vert"]])
    blk = HdivBlock(m, 2)
    nqs = 2 ** (dim - 1)
    groups = []
    for i, side in enumerate(["left", "right", "bottom", "top"] + (["back", "front"] if dim == 3 else [])):
        be, bs = meshlib.boundary_sides(dim, ncell, side)
        data = ("array", rng.uniform(-2, 2, (len(be), nqs))) if i % 2 else ("sinprod", 1.7, [1.0, 2.0, 0.5][:dim])
        groups.append((side, be, bs, data))
    res, S = boundary_arrays(blk, [(be, bs, d) for _, be, bs, d in groups])
    rowptr, colind = H.build_graph(m["ndof"], m["lids"])
    c = dict(module=BOUNDARY, family=family, shape=shape, m=m, dim=dim, qdeg=2, u=rng.uniform(-1, 1, m["ndof"]), blk=blk,
             groups=groups, res=res, S_res=S, rowptr=rowptr, colind=colind)
    _CASES[key] = c
    return c
