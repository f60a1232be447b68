"""The extended-precision yardstick of shallowwaterHybridized: the side point functions with their derivatives, the HDG
element's augmented system [A_uu A_ul | r_u ; A_lu A_ll | r_l] (12 interior + 24 HFACE trace unknowns), the volume term and
the statically condensed S, g, du in numpy's 80-bit longdouble / clongdouble, beside every entry the SCALE of its own sum.

TEST INFRASTRUCTURE, the sibling of tests/highprec_hdiv_ref.py.  From tests/highprec_ref.py it takes the mpmath Gauss and
Lagrange tables, the multilinear geometry, `seeded`, `assemble`, `matvec`, `diagonal` and `distance`; the side points and
the multilinear vertex functions at them are those of tests/highprec_hdiv_ref.py (mpmath tables again).  Of oracle/ and
mrhyde_amd/ it uses the mesh's integer maps only.

Reference lines restated here (src/physics/shallowwaterHybridized.cpp): computeFluxVector :409-480,
eigendecompFluxJacobian :765-823, computeStabilizationTerm :487-588, computeBoundaryTerm :595-758, computeFlux :270-368,
volumeResidual :113-184, boundaryResidual :190-263.  R w(Lambda) L x is written once, as the three matrix products of the
reference (characteristic_product); nothing here follows the device's swh_characteristic_apply.

Values and derivatives.  Every point function runs on `Mag` numbers: a clongdouble value whose imaginary part carries the
derivative (complex step h = 1e-30, as highprec_ref.point_derivative: no derivative is written by hand), and beside it the
magnitudes m, dm of the sums that formed its real and imaginary parts.  abs and max decide on the real part; what they do
at an exact tie (Re == 0, equal real parts) is the parameter `tie` = (abs_plus, max_second).  TIE_DEVICE = (True, True)
is the convention of the device and of the oracle (`a < 0 ? -a : a`, `a > b ? a : b`).  The AD library that decides this
in the reference is not available to read here; the other choices are measured in tests/test_highprec_swhdg.py, not guessed.

The scales.  The HGRAD rule (highprec_ref's header), |F| and |dF/dS| taken component by component:

  S_res_r = sum_p |T_r| |F| w        S_J_rc = sum_p |T_r| |C| |T_c| w        S_y = sum S_J |x|

For the volume term |F| and |C| are the absolute values of the point function and of its complex-step derivative, verbatim
(highprec_ref.element_arrays).  For the side terms they are the magnitudes m, dm instead: R w(Lambda) L x is itself a sum
whose terms cancel (the (H, H) entry of R Lambda L is 0 in exact arithmetic, and any evaluation, this one included, leaves
residue of the size eps |R| |Lambda| |L| there), so the absolute value of the result would judge round-off by the size of
round-off.  m and dm follow the sums as they are formed: |a| + |b| for a + b, m_a m_b and dm_a m_b + m_a dm_b for a b.  A
weight that is exactly zero (A- where every lambda > 0, A+ where every lambda < 0) gives m = dm = 0: there S == 0, and the
entry has to be exactly 0.0.

Condensed outputs: S = A_ll - A_lu X, g = r_l - A_lu x_r, [X | x_r] = A_uu^-1 [A_ul | r_u] by Gauss-Jordan with partial
pivoting in longdouble (condense_longdouble); their scale is the sum as formed, S_S_ab = S_All_ab + sum_i |A_lu|_ai |X|_ib
(likewise g; du: sum_j |A_uu^-1|_ij S_ru_j), and their bound carries the conditioning: it is measured on the CPU oracle.
"""
import numpy as np

import highprec_hdiv_ref as HD
import highprec_ref as H

LD, CLD = np.longdouble, np.clongdouble
MODULE, BOUNDARY, CONDENSED = "shallowwaterHybridized", "shallowwaterHybridized boundary", "shallowwaterHybridized condensed"
CONDENSED_CW = "shallowwaterHybridized condensed, componentwise scale"
INTERFACE, FARFIELD, SLIP = 0, 1, 2
TIE_DEVICE = (True, True)
GRAVITY = 9.81

# K_oracle[(group, family)] as tests/test_highprec_swhdg.py measures it (the measurement and the entry that gives it stand
# beside each constant; the table is in profiles/extended_precision_yardstick.md).  Per family:
#   * MODULE: the uncondensed arrays of the C oracle -- orc_swh_* at the side points, orc_swh_hdg_element, the volume term
#     of assemble_block(want_local) on every sub-mesh.  The rule of highprec_ref.K_ORACLE for the C oracle: the next
#     integer at least one half above the measurement, above 1000 the next multiple of ten.
#   * BOUNDARY: the boundary-group assembly, a key of its own as in highprec_hdiv_ref: the oracle takes d flux / d S there
#     as the difference f(S + e_j) - f(S) of two point-function values (the flux is affine in S), which leaves
#     eps |f| in a derivative of size |A|: d up to 1.8e5 on the metric family (g H^2 / 2 beside a).  Folded into MODULE it
#     would have let an error of 2^-40 in one term of the element kernels pass; the same rule.
#   * CONDENSED: S, g, du of numpy.linalg.solve on the oracle's blocks, m = 1..4.  LAPACK and matmul sum in the order of
#     the CPU's vector units: highprec_ref's rule for such figures, the measurement times 1.25 rounded up to two digits.
#   * CONDENSED_CW: the same S, g, du by the componentwise scale of `condensed` (the conditioning in the scale, not in
#     the constant): an addition to the criterion above, which alone lets an error of 2^-40 in one term of the fused
#     kernels pass (their only outputs are S, g, du).  The same rule as CONDENSED.
K_ORACLE = {
    (MODULE,    "unit"):             42,        # measured 40.764 (m=4 Roe steady volume local_J)
    (BOUNDARY,  "unit"):             437,       # measured 435.97 (m=2 Roe steady boundary vals)
    (CONDENSED, "unit"):             4100,      # measured 3227.9 (m=2 maxEV stage 1 schur)
    (MODULE,    "near-critical"):    101,       # measured 99.627 (m=4 Roe stage 1 volume local_J)
    (BOUNDARY,  "near-critical"):    1010,      # measured 1000.8 (m=2 maxEV stage 1 boundary vals)
    (CONDENSED, "near-critical"):    3900,      # measured 3074 (m=3 Roe stage 1 schur)
    (MODULE,    "supercritical"):    51,        # measured 50.197 (m=4 Roe stage 1 volume local_J)
    (BOUNDARY,  "supercritical"):    634,       # measured 632.75 (m=1 Roe steady boundary vals)
    (CONDENSED, "supercritical"):    9300,      # measured 7390.2 (m=2 maxEV stage 1 schur)
    (MODULE,    "shallow"):          42,        # measured 40.933 (m=4 Roe steady volume local_J)
    (BOUNDARY,  "shallow"):          8,         # measured 7.4217 (m=2 Roe stage 1 boundary vals)
    (CONDENSED, "shallow"):          4700000,   # measured 3.69e+06 (m=2 Roe steady schur)
    (MODULE,    "metric"):           56,        # measured 55.204 (m=4 Roe stage 1 volume local_res)
    (BOUNDARY,  "metric"):           180190,    # measured 1.8018e+05 (m=1 maxEV stage 1 boundary vals)
    (CONDENSED, "metric"):           3600000,   # measured 2.8535e+06 (m=4 Roe stage 1 schur)
    (MODULE,    "rest"):             47,        # measured 45.859 (m=3 Roe stage 1 volume local_res)
    (BOUNDARY,  "rest"):             1150,      # measured 1146.4 (m=2 maxEV stage 1 boundary vals)
    (CONDENSED, "rest"):             30000,     # measured 23769 (m=1 Roe steady schur)
    (MODULE,    "rest consistent"):  47,        # measured 45.859 (m=3 Roe stage 1 volume local_res)
    (BOUNDARY,  "rest consistent"):  1150,      # measured 1146.4 (m=2 maxEV stage 1 boundary vals)
    (CONDENSED, "rest consistent"):  13000,     # measured 9636.3 (m=1 maxEV stage 1 schur)
    (MODULE,    "stretched sheared"): 3850,      # measured 3849.2 (m=4 Roe stage 1 volume local_J)
    (BOUNDARY,  "stretched sheared"): 70,        # measured 68.754 (m=2 maxEV steady boundary vals)
    (CONDENSED, "stretched sheared"): 880000,    # measured 6.9919e+05 (m=3 maxEV steady schur)
    (CONDENSED_CW, "unit"):              5.2,    # measured 4.1521 (m=4 maxEV stage 1 schur)
    (CONDENSED_CW, "near-critical"):     5.3,    # measured 4.1679 (m=1 maxEV stage 1 schur)
    (CONDENSED_CW, "supercritical"):     35,     # measured 27.957 (m=2 maxEV stage 1 schur)
    (CONDENSED_CW, "shallow"):           210,    # measured 167.63 (m=1 Roe steady schur)
    (CONDENSED_CW, "metric"):            4600,   # measured 3621.1 (m=4 maxEV stage 1 schur)
    (CONDENSED_CW, "rest"):              5.3,    # measured 4.1637 (m=4 Roe stage 1 schur)
    (CONDENSED_CW, "rest consistent"):   6.4,    # measured 5.0694 (m=2 maxEV stage 1 schur)
    (CONDENSED_CW, "stretched sheared"): 22,     # measured 17.589 (m=2 maxEV stage 1 schur)
}
H.K_ORACLE.update(K_ORACLE)


# ---- numbers that carry the magnitude of their own sum --------------------------------------------------------------------
class Mag:
    """v: clongdouble array (Im / h = the derivative in the seeded direction); m, dm: longdouble arrays, the magnitude of
    the sums behind Re v and behind Im v / h."""
    __slots__ = ("v", "m", "dm")
    __array_ufunc__ = None                                      # ndarray op Mag -> Mag's reflected operator

    def __init__(self, v, m, dm):
        self.v, self.m, self.dm = v, m, dm

    @staticmethod
    def lift(a):
        if isinstance(a, Mag):
            return a
        a = np.asarray(a, dtype=LD)
        return Mag(a.astype(CLD), np.abs(a), np.zeros_like(a))

    def __add__(self, o):
        o = Mag.lift(o)
        return Mag(self.v + o.v, self.m + o.m, self.dm + o.dm)

    __radd__ = __add__

    def __neg__(self):
        return Mag(-self.v, self.m, self.dm)

    def __sub__(self, o):
        return self + (-Mag.lift(o))

    def __rsub__(self, o):
        return Mag.lift(o) + (-self)

    def __mul__(self, o):
        o = Mag.lift(o)
        return Mag(self.v * o.v, self.m * o.m, self.dm * o.m + self.m * o.dm)

    __rmul__ = __mul__

    def recip(self):
        a2 = np.real(self.v) ** 2
        return Mag(1 / self.v, self.m / a2, self.dm / a2)

    def __truediv__(self, o):
        return self * Mag.lift(o).recip()

    def __rtruediv__(self, o):
        return Mag.lift(o) * self.recip()

    def sqrt(self):
        r = np.sqrt(self.v)
        a = np.abs(np.real(r))
        return Mag(r, a * self.m / np.abs(np.real(self.v)), self.dm / (2 * a))


def m_abs(a, tie):
    re = np.real(a.v)
    neg = re < 0 if tie[0] else re <= 0
    return Mag(np.where(neg, -a.v, a.v), a.m, a.dm)


def m_split(a, tie):
    """((a + |a|) / 2, (a - |a|) / 2).  In binary arithmetic both are exact: a + |a| is 2 a or exactly 0, so one weight
    is a itself and the other is 0 with nothing behind it (m = dm = 0); at Re a == 0 the tie rule of abs decides which."""
    re = np.real(a.v)
    pos = re >= 0 if tie[0] else re > 0
    z = np.zeros_like(a.m)
    return (Mag(np.where(pos, a.v, 0), np.where(pos, a.m, z), np.where(pos, a.dm, z)),
            Mag(np.where(pos, 0, a.v), np.where(pos, z, a.m), np.where(pos, z, a.dm)))


def m_where(sel, a, b):
    return Mag(np.where(sel, a.v, b.v), np.where(sel, a.m, b.m), np.where(sel, a.dm, b.dm))


def m_max(a, b, tie):
    first = np.real(a.v) > np.real(b.v) if tie[1] else np.real(a.v) >= np.real(b.v)
    return Mag(np.where(first, a.v, b.v), np.where(first, a.m, b.m), np.where(first, a.dm, b.dm))


# ---- the point functions ----------------------------------------------------------------------------------------------------
def flux_vector(S, g):
    """computeFluxVector :446-478 -> F[eqn][dir]."""
    Hh, Hux, Huy = S
    p = 0.5 * Hh * Hh * g
    return [[Hux, Huy], [Hux * Hux / Hh + p, Hux * Huy / Hh], [Hux * Huy / Hh, Huy * Huy / Hh + p]]


def eigendecomp(Sh, nx, ny, g):
    """eigendecompFluxJacobian :792-823 -> L[3][3], lam[3], R[3][3]."""
    Hh, Hux, Huy = Sh
    vn = Hux / Hh * nx + Huy / Hh * ny
    a = (Hh * g).sqrt()
    one, zero = Mag.lift(np.ones_like(nx)), Mag.lift(np.zeros_like(nx))
    R = [[one, zero, one],
         [Hux / Hh + a * nx, -(a * ny), Hux / Hh - a * nx],
         [Huy / Hh + a * ny, a * nx, Huy / Hh - a * ny]]
    L = [[0.5 - vn / (2. * a), nx / (2. * a), ny / (2. * a)],
         [(ny * Hux / Hh - nx * Huy / Hh) / a, -ny / a, nx / a],
         [0.5 + vn / (2. * a), -nx / (2. * a), -ny / (2. * a)]]
    return L, [vn + a, vn, vn - a], R


def matvec3(A, x):
    """matVec: y_i = sum_j A_ij x_j."""
    return [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(3)]


def characteristic_product(L, w, R, x):
    """R diag(w) L x, the three products of :565-571 / :703-709."""
    t = matvec3(L, x)
    return matvec3(R, [t[i] * w[i] for i in range(3)])


def stab_term(S, Sh, nx, ny, g, roe, tie):
    """computeStabilizationTerm :541-586."""
    dS = [S[i] - Sh[i] for i in range(3)]
    if roe:
        L, lam, R = eigendecomp(Sh, nx, ny, g)
        return characteristic_product(L, [m_abs(l, tie) for l in lam], R, dS)
    vn = nx * Sh[1] / Sh[0]
    a = (Sh[0] * g).sqrt()
    vn = vn + ny * Sh[2] / Sh[0]
    lmax = m_max(m_abs(vn + a, tie), m_abs(vn - a, tie), tie)
    return [dS[i] * lmax for i in range(3)]


def boundary_term(side_type, S, Sh, Sinf, nx, ny, g, tie):
    """computeBoundaryTerm :675-756: Far-field A+ (S - Sh) - A- (Sinf - Sh), Slip."""
    if side_type == FARFIELD:
        L, lam, R = eigendecomp(Sh, nx, ny, g)
        dS = [S[i] - Sh[i] for i in range(3)]
        w = [m_split(l, tie) for l in lam]                          # (Lambda + |Lambda|) / 2, (Lambda - |Lambda|) / 2
        out = characteristic_product(L, [p for p, _ in w], R, dS)
        dS = [Sinf[i] - Sh[i] for i in range(3)]
        neg = characteristic_product(L, [q for _, q in w], R, dS)
        return [out[i] - neg[i] for i in range(3)]
    vn = nx * S[1] / S[0]
    vn = vn + ny * S[2] / S[0]
    return [S[0] - Sh[0], (S[1] / S[0] - vn * nx) - Sh[1] / Sh[0], (S[2] / S[0] - vn * ny) - Sh[2] / Sh[0]]


def interface_flux(side_type, S, Sh, Sinf, nx, ny, g, roe, tie):
    """computeFlux :297-362 (and the integrand of boundaryResidual :254-256 on an interface side)."""
    if side_type != INTERFACE:
        return boundary_term(side_type, S, Sh, Sinf, nx, ny, g, tie)
    F = flux_vector(Sh, g)
    st = stab_term(S, Sh, nx, ny, g, roe, tie)
    return [F[i][0] * nx + F[i][1] * ny + st[i] for i in range(3)]


def _seed(S, mS, k0, k):
    h = H.H_STEP
    out = []
    for i in range(3):
        on = k == k0 + i
        out.append(Mag(S[..., i].astype(CLD) + (1j * h if on else 0), mS[..., i], np.full(S.shape[:-1], 1.0 if on else 0.0, LD)))
    return out


def _vals(xs):
    return np.stack([np.real(x.v).astype(LD) for x in xs], -1), np.stack([x.m for x in xs], -1)


def _ders(xs):
    return np.stack([np.imag(x.v).astype(LD) / H.H_STEP for x in xs], -1), np.stack([x.dm for x in xs], -1)


def side_point_eval(side_type, roe, g, S, Sh, n, Sinf, tie=TIE_DEVICE, mS=None, mSh=None):
    """Everything mha_swhdg_side_terms and mha_swhdg_eigendecomp give, at the points of S, Sh, Sinf [..., 3], n [..., 2]
    (taken as exact): name -> (value, scale), longdouble.  side_type and roe may be arrays over the points.  mS, mSh:
    the magnitudes of the sums that formed S and Sh (default: |S|, |Sh|, exact inputs)."""
    S, Sh, Sinf, n = (np.asarray(a).astype(LD) for a in (S, Sh, Sinf, n))
    shp = S.shape[:-1]
    Sinf = np.broadcast_to(Sinf, S.shape)
    mS = np.abs(S) if mS is None else mS
    mSh = np.abs(Sh) if mSh is None else mSh
    nx, ny = n[..., 0], n[..., 1]
    st_arr = np.broadcast_to(np.asarray(side_type), shp)
    Sf = [Mag.lift(Sinf[..., i]) for i in range(3)]
    roe = bool(roe)

    def run(k):
        a, b = _seed(S, mS, 0, k), _seed(Sh, mSh, 3, k)
        flux = term = None
        for t in np.unique(st_arr):
            fl = interface_flux(int(t), a, b, Sf, nx, ny, g, roe, tie)
            tm = stab_term(a, b, nx, ny, g, roe, tie) if t == INTERFACE else fl
            sel = st_arr == t
            flux = fl if flux is None else [m_where(sel, x, y) for x, y in zip(fl, flux)]
            term = tm if term is None else [m_where(sel, x, y) for x, y in zip(tm, term)]
        return flux, term

    out = {}
    cols, scols = [], []
    for k in range(6):
        flux, term = run(k)
        if k == 0:
            out["iflux"], out["term"] = _vals(flux), _vals(term)
        d, s = _ders(flux)
        cols.append(d)
        scols.append(s)
    out["d_dS"] = (np.stack(cols[:3], -1), np.stack(scols[:3], -1))          # [..., eqn, state]
    out["d_dShat"] = (np.stack(cols[3:], -1), np.stack(scols[3:], -1))
    b = _seed(Sh, mSh, 3, -1)
    F = flux_vector(b, g)
    out["fluxvec"] = tuple(np.stack(a, -2) for a in zip(*[_vals(row) for row in F]))      # [..., eqn, dir]
    L, lam, R = eigendecomp(b, nx, ny, g)
    out["L"] = tuple(np.stack(a, -2) for a in zip(*[_vals(row) for row in L]))
    out["R"] = tuple(np.stack(a, -2) for a in zip(*[_vals(row) for row in R]))
    out["lam"] = _vals(lam)
    return out


def eigenvalues(Sh, n, g):
    """lam [..., 3] and a [...] at the trace states (longdouble), for the guards."""
    Sh, n = np.asarray(Sh).astype(LD), np.asarray(n).astype(LD)
    vn = (Sh[..., 1] * n[..., 0] + Sh[..., 2] * n[..., 1]) / Sh[..., 0]
    a = np.sqrt(Sh[..., 0] * LD(g))
    return np.stack([vn + a, vn, vn - a], -1), a


# ---- side geometry of the HDG (macro) element ---------------------------------------------------------------------------------
# A macro element is an m x m sub-mesh of Q1 elements (m = 1: the HDG element itself), elements [k m^2, (k + 1) m^2) row by
# row with x fastest.  Interior unknowns of a macro element: (variable, node) = v (m + 1)^2 + ay (m + 1) + ax; the Q1
# functions of a sub-element in tensor order (xi fastest).  The mesh's sides: bottom, right, top, left
# (highprec_hdiv_ref._SIDE_2D); the HFACE trace basis sits on the macro edges left, bottom, right, top (swhdg_element.hip),
# two linear functions per edge in the edge's coordinate t (eta on left and right, xi on bottom and top):
# mu_0 = (1 - t) / 2, mu_1 = (1 + t) / 2, and on sub-side j of m the edge coordinate is t = -1 + (2 j + (t_local + 1)) / m
# (tests/swhdg_subgrid_ref.py).  Traces: n_int + 8 v + 2 edge + k.  Only the 4 m sub-sides on the macro boundary carry side
# terms.
HFACE_EDGE = [1, 2, 3, 0]
NT = 24


def n_int(m):
    return 3 * (m + 1) ** 2


def interior_index(m, ex, ey):
    """[3][4]: macro-interior index of (variable, Q1 function) of sub-element (ex, ey)."""
    npn = (m + 1) ** 2
    return np.array([[v * npn + (ey + (aa >> 1)) * (m + 1) + ex + (aa & 1) for aa in range(4)] for v in range(3)])


def side_geometry(nodes, qdeg, s):
    """Side s of the elements nodes [k][4][2] -> dict: x [k][qs][2], n [k][qs][2] (unit, outward), w [k][qs] (side weights:
    n w = w_ref det J^-T nhat), phi [qs][4] (Q1 functions), t [qs] (the side's local edge coordinate)."""
    X = np.asarray(nodes).astype(LD)
    xi, wref, c, sign = HD.side_points(2, qdeg, s)
    NV, NG = HD.vertex_functions(2, xi)
    x = np.einsum("evd,vq->eqd", X, NV)
    J = np.einsum("evd,vqc->eqdc", X, NG)
    det, Jinv = H.cofactor_inverse(J)
    assert np.all(det > 0)
    nvec = sign * det[..., None] * Jinv[:, :, c, :]
    area = np.sqrt((nvec * nvec).sum(axis=2))
    fx = np.stack([(1 - xi[:, 0]) / 2, (1 + xi[:, 0]) / 2], -1)            # [q][a]
    fy = np.stack([(1 - xi[:, 1]) / 2, (1 + xi[:, 1]) / 2], -1)
    phi = np.einsum("qb,qa->qba", fy, fx).reshape(len(xi), 4)                # f = a + 2 b
    t = xi[:, 1] if HFACE_EDGE[s] in (0, 2) else xi[:, 0]
    return dict(x=x, n=nvec / area[..., None], w=wref[None, :] * area, phi=phi, t=t, xi=xi)


def boundary_subsides(m):
    """(side s, sub-side j, ex, ey) of the 4 m sub-sides on the macro boundary."""
    for s in range(4):
        for j in range(m):
            yield s, j, (m - 1 if s == 1 else (0 if s == 3 else j)), (0 if s == 0 else (m - 1 if s == 2 else j))


def side_blocks(nodes, m, qdeg, ue, alpha_u, lam, st, ff, g, roe, tie=TIE_DEVICE):
    """The side part of the HDG macro elements: nodes [Em m^2][4][2], ue [Em][n_int] the (seeded) interior values, lam
    [Em][24], st [Em][4] side types, ff [3] the far-field state.  -> dict(res [Em][N] = -R, blocks [Em][N][N] =
    dR/d(u, lambda), S_res, S_blocks; N = n_int + 24) and the point data pts = [(s, j, geometry, S, Sh, point values)]."""
    ni = n_int(m)
    N = ni + NT
    ue, lm = np.asarray(ue).astype(LD), np.asarray(lam).astype(LD)
    Em = ue.shape[0]
    lm = lm.reshape(Em, 3, 4, 2)
    st = np.asarray(st)
    out = dict(res=np.zeros((Em, N), LD), S_res=np.zeros((Em, N), LD), blocks=np.zeros((Em, N, N), LD),
               S_blocks=np.zeros((Em, N, N), LD), pts=[])
    for s, j, ex, ey in boundary_subsides(m):
        edge = HFACE_EDGE[s]
        el = np.arange(Em) * m * m + ey * m + ex
        geo = side_geometry(np.asarray(nodes)[el], qdeg, s)
        qs = len(geo["t"])
        tc = -1 + (2 * j + (geo["t"] + 1)) / LD(m)
        mu = np.stack([(1 - tc) / 2, (1 + tc) / 2], -1)                        # [q][2]
        gi = interior_index(m, ex, ey)                                        # [3][4]
        ul = ue[:, gi]                                                        # [Em][3][4]
        S, mS = np.einsum("qf,evf->eqv", geo["phi"], ul), np.einsum("qf,evf->eqv", geo["phi"], np.abs(ul))
        le = lm[:, :, edge, :]                                                # [Em][3][2]
        Sh, mSh = np.einsum("qk,evk->eqv", mu, le), np.einsum("qk,evk->eqv", mu, np.abs(le))
        st_pt = np.broadcast_to(st[:, s, None], (Em, qs))
        pe = side_point_eval(st_pt, roe, g, S, Sh, geo["n"], ff, tie, mS, mSh)
        out["pts"].append((s, j, geo, S, Sh, pe))
        # the test functions of this sub-side [q][6] and their unknowns: 4 interior + 2 trace per variable
        T = np.concatenate([geo["phi"], mu], axis=1)
        dT = np.concatenate([LD(alpha_u) * geo["phi"], mu], axis=1)            # d (S | Sh) / d unknown
        idx = np.array([np.concatenate([gi[v], ni + 8 * v + 2 * edge + np.arange(2)]) for v in range(3)])    # [3][6]
        isS = np.arange(6) < 4
        for tag, k in (("", 0), ("S_", 1)):
            F, CS, CSh = pe["iflux"][k], pe["d_dS"][k], pe["d_dShat"][k]       # [Em][q][3], [Em][q][3][3]
            R = np.einsum("eq,qa,eqi->eia", geo["w"], T, F)                    # [Em][eqn][6]
            C = np.where(isS[None, None, None, None, :], CS[..., None], CSh[..., None])        # [Em][q][i][jvar][6]
            B = np.einsum("eq,qa,eqijb,qb->eiajb", geo["w"], T, C, dT)         # [Em][i][a][jvar][b]
            for i in range(3):
                out[tag + "res"][:, idx[i]] += -R[:, i] if k == 0 else R[:, i]
                for jv in range(3):
                    out[tag + "blocks"][:, idx[i][:, None], idx[jv][None, :]] += B[:, i, :, jv, :]
    return out


# ---- the volume term -------------------------------------------------------------------------------------------------------------
def volume_point(U, Ud, x, P):
    """volumeResidual :164-180: (v_i, dS_i/dt) - (grad v_i, F_i) - (v_i, source_i); slots [value, d/dx, d/dy] per variable."""
    g = LD(P["g"])
    Hh, Hux, Huy = U[0], U[3], U[6]
    p = .5 * Hh * Hh * g
    Fl = [[Hux, Huy], [Hux * Hux / Hh + p, Hux * Huy / Hh], [Hux * Huy / Hh, Huy * Huy / Hh + p]]
    F = [None] * 9
    for v, name in enumerate(("source H", "source Hux", "source Huy")):
        F[3 * v] = Ud[3 * v] - H.func_value(P[name], x)
        F[3 * v + 1], F[3 * v + 2] = -Fl[v][0], -Fl[v][1]
    return F


H.POINT[MODULE] = volume_point


# ---- condensation -------------------------------------------------------------------------------------------------------------------
def condense_longdouble(blocks, res, ni, nt):
    """Gauss-Jordan on [A_uu | A_ul | r_u] with partial pivoting in 80-bit arithmetic -> (S, g, du) as float64 and the
    smallest number of row exchanges over the elements (the form tests/test_swhdg_gpu.py uses)."""
    Sg, X, nswap = _condense(blocks, res, ni)
    return (Sg[:, :, :nt].astype(np.float64), Sg[:, :, nt].astype(np.float64), X[:, :, nt].astype(np.float64), int(nswap.min()))


def _gauss_jordan(M, ni):
    """M [E][ni][ni + k] = [A | B] -> (A^-1 B, row exchanges per element), partial pivoting, in M's precision."""
    E = M.shape[0]
    ar = np.arange(E)
    nswap = np.zeros(E, dtype=int)
    for k in range(ni):
        piv = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        nswap += piv != k
        rk, rp = M[ar, k].copy(), M[ar, piv].copy()
        M[ar, piv], M[ar, k] = rk, rp
        M[:, k] = M[:, k] / M[:, k, k:k + 1]
        f = M[:, :, k].copy()
        f[:, k] = 0
        M = M - f[:, :, None] * M[:, k:k + 1, :]
    return M[:, :, ni:], nswap


def _condense(blocks, res, ni):
    X, nswap = _gauss_jordan(np.concatenate([blocks[:, :ni, :], res[:, :ni, None]], axis=2).astype(LD), ni)   # [X_ul | x_r]
    low = np.concatenate([blocks[:, ni:, :], res[:, ni:, None]], axis=2).astype(LD)
    Sg = low[:, :, ni:] - np.einsum("eai,eib->eab", low[:, :, :ni], X)
    return Sg, X, nswap


def condensed(blocks, res, S_blocks, S_res, ni):
    """-> dict(schur, gvec, du, S_schur, S_gvec, S_du) in longdouble, the scales the sums as formed."""
    nt = res.shape[1] - ni
    E = res.shape[0]
    Sg, X, _ = _condense(blocks, res, ni)
    Ainv, _ = _gauss_jordan(np.concatenate([blocks[:, :ni, :ni], np.broadcast_to(np.eye(ni, dtype=LD), (E, ni, ni))], axis=2).astype(LD), ni)
    Alu = np.abs(blocks[:, ni:, :ni].astype(LD))
    low = np.concatenate([S_blocks[:, ni:, ni:], S_res[:, ni:, None]], axis=2)
    SSg = low + np.einsum("eai,eib->eab", Alu, np.abs(X))
    # the second, sharper scale (key CONDENSED_CW): the first-order componentwise bound of the same sums under entrywise
    # perturbations of the blocks by their own scales, |dX| <= |A_uu^-1| (S_[A_ul | r_u] + S_A_uu |X|), so that the
    # conditioning sits in the scale and not in K_oracle
    up = np.concatenate([S_blocks[:, :ni, ni:], S_res[:, :ni, None]], axis=2)
    SX = np.einsum("eij,ejb->eib", np.abs(Ainv), up + np.einsum("eij,ejb->eib", S_blocks[:, :ni, :ni], np.abs(X)))
    CSg = low + np.einsum("eai,eib->eab", S_blocks[:, ni:, :ni], np.abs(X)) + np.einsum("eai,eib->eab", Alu, SX)
    return dict(schur=Sg[:, :, :nt], gvec=Sg[:, :, nt], du=X[:, :, nt], S_schur=SSg[:, :, :nt], S_gvec=SSg[:, :, nt],
                S_du=np.einsum("eij,ej->ei", np.abs(Ainv), S_res[:, :ni]),
                C_schur=CSg[:, :, :nt], C_gvec=CSg[:, :, nt], C_du=SX[:, :, nt])


def cond2(A):
    """2-norm condition numbers of A [E][n][n] (double precision is enough for a guard at 1e7)."""
    sv = np.linalg.svd(np.asarray(A, dtype=np.float64), compute_uv=False)
    return sv[:, 0] / sv[:, -1]


# ---- the input families -----------------------------------------------------------------------------------------------------------------
FAMILIES = ["unit", "near-critical", "supercritical", "shallow", "metric", "rest", "rest consistent", "stretched sheared"]
REST = ("rest", "rest consistent")
# (H range, Froude range, direction range in rad about +x or None = any, far-field state or ("froude", H, Fr, direction))
_SPEC = {
    "unit":              ((1.0, 2.0), (0.0, 0.3), None, (1.4, -0.3, 0.5)),
    "near-critical":     ((1.0, 2.0), (0.9, 1.1), (0.2, 0.5), ("froude", 1.5, 1.0, 0.35)),
    "supercritical":     ((1.0, 2.0), (1.5, 2.5), (0.2, 0.5), ("froude", 1.5, 2.0, 0.35)),
    "shallow":           ((1e-3, 2e-3), (0.0, 0.3), None, ("froude", 1.4e-3, 0.2, 2.1)),
    "metric":            ((50.0, 100.0), (0.0, 0.05), None, ("froude", 70.0, 0.03, 2.1)),
    "rest":              ((1.0, 2.0), (0.0, 0.0), None, (1.4, 0.0, 0.0)),
    "rest consistent":   ((1.0, 2.0), (0.0, 0.0), None, (1.4, 0.0, 0.0)),
    "stretched sheared": ((1.0, 2.0), (0.0, 0.3), None, (1.4, -0.3, 0.5)),
}
BRANCH_GUARD, COND_GUARD = 1e-3, 1e7
QDEG = 2
NCELL = {1: (3, 2), 2: (2, 2), 3: (2, 2), 4: (2, 2)}                    # macro elements per m
# The seed of each (family, m): the first from 300 on at which the family's guards hold on every case of that m (both
# stabilisations, steady and stage 1), as find_seed finds it; tests/test_highprec_swhdg.py asserts the guards on each.
SEED = {(f, m): 300 for f in FAMILIES for m in (1, 2, 3, 4)}
SEED.update({("unit", 1): 301, ("near-critical", 1): 302, ("shallow", 1): 301, ("metric", 1): 330,
             ("unit", 2): 301, ("shallow", 2): 301, ("metric", 2): 328, ("stretched sheared", 2): 302,
             ("unit", 3): 301, ("shallow", 3): 301, ("metric", 3): 458, ("stretched sheared", 3): 302,
             ("unit", 4): 301, ("shallow", 4): 301, ("metric", 4): 338, ("stretched sheared", 4): 301})


def _states(rng, family, shape):
    """Random states [shape + (3,)] of the family: H, then speed = Fr sqrt(g H) in the family's directions."""
    (h0, h1), (f0, f1), dirs, _ = _SPEC[family]
    Hh = rng.uniform(h0, h1, shape)
    fr = rng.uniform(f0, f1, shape)
    sgn = rng.choice([-1.0, 1.0], shape)
    th = rng.uniform(0, 2 * np.pi, shape) if dirs is None else sgn * rng.uniform(dirs[0], dirs[1], shape)
    sp = fr * np.sqrt(GRAVITY * Hh)
    if family in REST:
        return np.stack([Hh, np.zeros(shape), np.zeros(shape)], -1)
    return np.stack([Hh, Hh * sp * np.cos(th), Hh * sp * np.sin(th)], -1)


def farfield_state(family):
    ff = _SPEC[family][3]
    if ff[0] == "froude":
        _, Hh, fr, th = ff
        sp = fr * np.sqrt(GRAVITY * Hh)
        return np.array([Hh, Hh * sp * np.cos(th), Hh * sp * np.sin(th)])
    return np.array(ff, dtype=np.float64)


def macro_vertices(family):
    """The warp of tests/test_oracle_swhdg.py's hdg_case on the macro vertices; the 1 : 1e-3 sheared box of
    highprec_ref.map_vertices."""
    def warp(c):
        if family == "stretched sheared":
            return H.map_vertices(np.asarray(c, dtype=np.float64), family)
        w = c.copy()
        w[:, 0] += 0.07 * np.sin(2.0 * c[:, 1])
        w[:, 1] += 0.05 * c[:, 0] ** 2
        return w
    return warp


_CASES = {}


def build_case(family, m, roe, transient, seed=None):
    """One case, cached: NCELL[m] macro elements of m x m Q1 sub-elements (the mesh and its integer maps from
    tests/swhdg_subgrid_ref.subgrid_mesh: interior unknowns local to a macro element), mixed side types, the yardstick's
    side blocks `sd`, volume arrays `el` (per sub-element, LID-position order), global volume arrays `g`, the full system
    `blocks`, `res` with `S_blocks`, `S_res`, and the condensed outputs `cd`."""
    import swhdg_subgrid_ref as R
    key = (family, m, bool(roe), bool(transient), seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(SEED[(family, m)] if seed is None else seed)
    sm = R.subgrid_mesh(NCELL[m], m, warp=macro_vertices(family))
    Em, ni, npn = sm["nmacro"], sm["n_int"], (m + 1) ** 2
    sm.update(orders=np.array([1, 1, 1], np.int32), varptr=np.array([0, 4, 8, 12], np.int32), types=np.array([0, 0, 0], np.int32),
              orient=np.ones((sm["nelem"], 12), np.int8), n_tot=12)
    rows = R.interior_rows(sm)                                                 # [Em][n_int] global row of (variable, node)
    assert np.array_equal(np.sort(rows.ravel()), np.arange(sm["ndof"]))

    def field():                                                               # a global vector of the family's states
        a = np.zeros(sm["ndof"])
        a[rows] = np.transpose(_states(rng, family, (Em, npn)), (0, 2, 1)).reshape(Em, ni)
        return a
    lam = np.transpose(_states(rng, family, (Em, 4, 2)), (0, 3, 1, 2))          # [Em][v][edge][k]  (the first draw: find_seed)
    st = rng.integers(0, 3, (Em, 4)).astype(np.uint8)
    u = field()
    if family == "rest consistent":                                            # the trace of the interior state
        uv = u[rows].reshape(Em, 3, m + 1, m + 1)                              # [..][ay][ax]
        ends = {0: ((0, 0), (m, 0)), 1: ((0, 0), (0, m)), 2: ((0, m), (m, m)), 3: ((m, 0), (m, m))}   # edge -> (ay, ax) of t = -1, +1
        for ed, pts in ends.items():
            for k, (ay, ax) in enumerate(pts):
                lam[:, :, ed, k] = uv[:, :, ay, ax]
    tr = None
    if transient:
        size = np.linalg.norm(sm["nodes"][:, 2] - sm["nodes"][:, 0], axis=1).min()
        tr = dict(H.TABLEAU, dt=float(0.1 * size / np.sqrt(GRAVITY * _SPEC[family][0][1])),
                  u_prev=np.stack([field(), field()], 1), u_stage=np.stack([field(), field()], 1))
    P = {"g": GRAVITY, "source H": 0.2, "source Hux": ("sinprod", 1.0, [1.0, 2.0]), "source Huy": -0.4}
    if family in ("shallow", "metric"):                                       # sources of the size of the flux divergence
        sc = _SPEC[family][0][1] ** 1.5
        P.update({"source H": 0.2 * sc, "source Hux": ("sinprod", sc, [1.0, 2.0]), "source Huy": -0.4 * sc})
    if family in REST:
        P.update({"source H": 0.0, "source Hux": 0.0, "source Huy": 0.0})
    ff = farfield_state(family)
    blk = H.Block(sm, QDEG)
    el = H.element_arrays(blk, MODULE, P, u, tr)
    us, _, alpha_u, _ = blk.seeded(u, tr)
    sd = side_blocks(sm["nodes"], m, QDEG, us[rows], alpha_u, lam.reshape(Em, 24), st, ff, GRAVITY, roe)
    full = {k: sd[k].copy() for k in ("res", "blocks", "S_res", "S_blocks")}
    off = np.asarray(sm["offsets"])
    for ey in range(m):
        for ex in range(m):
            gi = interior_index(m, ex, ey).ravel()
            e = np.arange(Em) * m * m + ey * m + ex
            for name, vol in (("blocks", "local_J"), ("S_blocks", "S_J")):
                full[name][:, gi[:, None], gi[None, :]] += el[vol][e][:, off][:, :, off]
            for name, vol in (("res", "local_res"), ("S_res", "S_res")):
                full[name][:, gi] += el[vol][e][:, off]
    c = dict(module=MODULE, family=family, mm=m, roe=bool(roe), m=sm, rows=rows, dim=2, qdeg=QDEG, u=u, lam=lam.reshape(Em, 24),
             st=st, ff=ff, tr=tr, P=P, blk=blk, el=el, g=H.assemble(blk, el), sd=sd, n_int=ni, **full)
    # the conditioning guard decides whether the condensed outputs of this case are compared at all
    c["cond"] = float(cond2(full["blocks"][:, :ni, :ni]).max())
    c["cd"] = condensed(full["blocks"], full["res"], full["S_blocks"], full["S_res"], ni) if c["cond"] <= COND_GUARD else None
    _CASES[key] = c
    return c


def check_guards(c):
    """The branch, regime and conditioning guards of one case (assertions on the yardstick) -> largest cond_2(A_uu)."""
    fam, ni = c["family"], c["n_int"]
    Sh = np.stack([p[4] for p in c["sd"]["pts"]], 1)                           # [Em][4 m][qs][3]
    S = np.stack([p[3] for p in c["sd"]["pts"]], 1)
    nrm = np.stack([p[2]["n"] for p in c["sd"]["pts"]], 1)
    side = np.array([p[0] for p in c["sd"]["pts"]])
    lam, a = eigenvalues(Sh, nrm, GRAVITY)
    if fam not in REST:
        assert np.all(np.abs(lam).min(axis=-1) >= BRANCH_GUARD * a), "branch guard: an eigenvalue within 1e-3 a of 0"
    else:
        assert np.all(lam[..., 1] == 0) and np.all(S[..., 1:] == 0) and np.all(Sh[..., 1:] == 0)
    far = np.asarray(c["st"])[:, side] == FARFIELD                             # [Em][4 m]
    if fam == "supercritical":
        allpos, allneg = np.all(lam > 0, axis=(-1, -2)), np.all(lam < 0, axis=(-1, -2))
        assert (far & allpos).any() and (far & allneg).any(), "regime guard: no far-field side with every lambda > 0 / < 0"
    if fam == "near-critical":
        assert (lam[..., 2] > 0).any() and (lam[..., 2] < 0).any(), "regime guard: lam2 keeps one sign"
    # cond_2(A_uu) <= 1e7 wherever S, g, du are compared: every one-element case, and every subgrid case at stage 1.  A
    # steady subgrid case may exceed it (at rest the steady A_uu of m >= 3 is singular to working precision): its
    # condensed outputs are then not compared (c["cd"] is None), its uncondensed blocks are.
    if c["mm"] == 1 or c["tr"] is not None:
        assert c["cond"] <= COND_GUARD, ("conditioning guard", c["cond"])
    return c["cond"]


def _trace_guards(family, m, seed):
    """The branch and regime guards from the traces alone (the first draws of build_case): a quick screen for find_seed."""
    import swhdg_subgrid_ref as R
    rng = np.random.default_rng(seed)
    sm = R.subgrid_mesh(NCELL[m], m, warp=macro_vertices(family))
    Em = sm["nmacro"]
    lm = np.transpose(_states(rng, family, (Em, 4, 2)), (0, 3, 1, 2)).astype(LD)
    st = rng.integers(0, 3, (Em, 4))
    lams, far = [], []
    for s, j, ex, ey in boundary_subsides(m):
        geo = side_geometry(sm["nodes"][np.arange(Em) * m * m + ey * m + ex], QDEG, s)
        tc = -1 + (2 * j + (geo["t"] + 1)) / LD(m)
        mu = np.stack([(1 - tc) / 2, (1 + tc) / 2], -1)
        lam, a = eigenvalues(np.einsum("qk,evk->eqv", mu, lm[:, :, HFACE_EDGE[s], :]), geo["n"], GRAVITY)
        if family not in REST and not np.all(np.abs(lam).min(axis=-1) >= BRANCH_GUARD * a):
            return False
        lams.append(lam)
        far.append(st[:, s] == FARFIELD)
    lams, far = np.stack(lams, 1), np.stack(far, 1)
    if family == "supercritical":
        return bool((far & np.all(lams > 0, axis=(-1, -2))).any() and (far & np.all(lams < 0, axis=(-1, -2))).any())
    if family == "near-critical":
        return bool((lams[..., 2] > 0).any() and (lams[..., 2] < 0).any())
    return True


def find_seed(family, m, start=300, tries=20000):
    """The first seed at which every case of (family, m) passes check_guards (how SEED was filled)."""
    for seed in range(start, start + tries):
        if not _trace_guards(family, m, seed):
            continue
        try:
            for roe in (True, False):
                for transient in (False, True):
                    check_guards(build_case(family, m, roe, transient, seed=seed))
            return seed
        except AssertionError:
            continue
    raise AssertionError("no seed in range")


# ---- boundary groups (boundaryResidual through the block's boundary-group interface) ----------------------------------------
# BOUNDARY_SEED[(family, m)]: the first seed from 0 on at which the groups' per-point trace states of the m-case pass the
# branch guard (find_boundary_seed).  The states are drawn per (element, side, point), so every m has draws of its own;
# boundary_guard asserts the guard on each (family, m) whose groups are built (m = 1 and 2).
BOUNDARY_MS = (1, 2)
BOUNDARY_SEED = {(f, m): 0 for f in FAMILIES for m in BOUNDARY_MS}
BOUNDARY_SEED.update({("unit", 1): 4, ("unit", 2): 5, ("near-critical", 2): 1, ("shallow", 1): 4, ("shallow", 2): 5,
                      ("metric", 1): 4, ("metric", 2): 7257, ("stretched sheared", 2): 7})


def boundary_guard(c, groups):
    """The branch guard at every per-point trace state of the groups (the rest families sit on the tie by construction)."""
    if c["family"] in REST:
        return all(np.all(aux[..., 1:] == 0) for _, _, _, _, aux, _ in groups)
    sm, ok = c["m"], True
    for name, bc, be, bs, aux, ffp in groups:
        for s in range(4):
            sel = bs == s
            geo = side_geometry(sm["nodes"][be[sel]], c["qdeg"], s)
            lam, a = eigenvalues(aux[sel], geo["n"], GRAVITY)
            ok = ok and bool(np.all(np.abs(lam).min(axis=-1) >= BRANCH_GUARD * a))
    return ok


def find_boundary_seed(family, m, tries=20000):
    c = build_case(family, m, True, False)
    for seed in range(tries):
        if boundary_guard(c, boundary_groups(c, seed)):
            return seed
    raise AssertionError("no seed in range")


def boundary_groups(c, seed=None):
    """Three groups over ALL (element, side) pairs of the case's mesh, one per side type (interface 10, far-field 11, slip
    12), each with per-point trace and far-field states of the family [nb][qs][3]: -> [(name, bc, belem, bside, aux, ff)]."""
    rng = np.random.default_rng(1000 + (BOUNDARY_SEED[(c["family"], c["mm"])] if seed is None else seed))
    E = c["m"]["nelem"]
    be, bs = np.repeat(np.arange(E, dtype=np.int32), 4), np.tile(np.arange(4, dtype=np.int32), E)
    kind = (be + bs) % 3
    qs = H.gauss_npts(c["qdeg"])
    out = []
    for t, name in enumerate(("interface", "farfield", "slip")):
        sel = kind == t
        nb = int(sel.sum())
        out.append((name, 10 + t, be[sel], bs[sel], _states(rng, c["family"], (nb, qs)), _states(rng, c["family"], (nb, qs))))
    return out


def boundary_arrays(c, groups, tie=TIE_DEVICE):
    """The groups' contribution to the global residual and CRS values on the graph of c["g"] (interior rows only: the trace
    state is data) -> dict(res, crs_vals, S_res, S_vals, lam, a); lam, a: the eigenvalues at every point, for the guards."""
    sm, blk, g = c["m"], c["blk"], c["g"]
    nd = sm["ndof"]
    off = np.asarray(sm["offsets"]).reshape(3, 4)
    us, _, alpha_u, _ = blk.seeded(c["u"], c["tr"])
    rows_of = np.repeat(np.arange(nd), np.diff(g["rowptr"]))
    key = rows_of.astype(np.int64) * nd + g["colind"]
    out = dict(res=np.zeros(nd, LD), S_res=np.zeros(nd, LD), crs_vals=np.zeros(len(key), LD), S_vals=np.zeros(len(key), LD),
               lam=[], a=[])
    for name, bc, be, bs, aux, ffp in groups:
        for s in range(4):
            sel = bs == s
            if not sel.any():
                continue
            el = be[sel]
            geo = side_geometry(sm["nodes"][el], c["qdeg"], s)
            lid = sm["lids"][el][:, off]                                        # [k][3][4] global rows of (variable, function)
            ul = us[lid]
            S, mS = np.einsum("qf,evf->eqv", geo["phi"], ul), np.einsum("qf,evf->eqv", geo["phi"], np.abs(ul))
            pe = side_point_eval(bc - 10, c["roe"], GRAVITY, S, aux[sel], geo["n"], ffp[sel], tie, mS, None)
            lam, a = eigenvalues(aux[sel], geo["n"], GRAVITY)
            out["lam"].append(lam.reshape(-1, 3))
            out["a"].append(a.ravel())
            idx = np.searchsorted(key, lid.reshape(len(el), 12, 1).astype(np.int64) * nd + lid.reshape(len(el), 1, 12))
            for tag, k in (("", 0), ("S_", 1)):
                R = np.einsum("eq,qa,eqi->eia", geo["w"], geo["phi"], pe["iflux"][k])
                B = LD(alpha_u) * np.einsum("eq,qa,eqij,qb->eiajb", geo["w"], geo["phi"], pe["d_dS"][k], geo["phi"])
                np.add.at(out[tag + "res"], lid, -R if k == 0 else R)
                np.add.at(out[tag + ("crs_vals" if k == 0 else "vals")], idx, B.reshape(len(el), 12, 12))
    out["lam"], out["a"] = np.concatenate(out["lam"]), np.concatenate(out["a"])
    return out


def point_inputs(family, m=1):
    """The side points of the family's m-case as DOUBLES (what a point-level call takes): S, Sh [P][3], n [P][2], and the
    far-field state."""
    c = build_case(family, m, True, False)
    S = np.concatenate([p[3].reshape(-1, 3) for p in c["sd"]["pts"]]).astype(np.float64)
    Sh = np.concatenate([p[4].reshape(-1, 3) for p in c["sd"]["pts"]]).astype(np.float64)
    n = np.concatenate([p[2]["n"].reshape(-1, 2) for p in c["sd"]["pts"]]).astype(np.float64)
    return S, Sh, n, c["ff"]
