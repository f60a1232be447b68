"""The extended-precision yardstick of the HGRAD modules (thermal, navierstokes, linearelasticity, cdr, helmholtz, stokes,
shallowwater and the coupled blocks navierstokes+thermal, linearelasticity+thermal, navierstokes+cdr): element arrays,
global CRS values and residuals in numpy's 80-bit longdouble / clongdouble (eps 1.08e-19) from 1-D ingredients that mpmath
computes at 40 digits, and beside every entry the SCALE of its own sum, so that an entry is judged by its own condition.

TEST INFRASTRUCTURE (the checker), imported by tests/test_highprec.py, tests/test_highprec_gpu.py and the HVOL/HDIV sibling
tests/highprec_hdiv_ref.py only.  It shares no
code, tables or derivative rules with oracle/ or mrhyde_amd/: quadrature and Lagrange tables come from mpmath, the
geometry from the multilinear map of the element's vertices, the modules are restated as point functions from the
reference's loop nests, and their derivatives are complex steps (no hand-written derivative, no AD rules).

  res_i = -sum_q T(i,q) . F(q) w(q)                            S_res_i = sum_q sum_k |T_k(i,q)| |F_k(q)| w(q)
  J_ij  =  sum_q T(i,q)^T [alpha_u dF/dU + alpha_t dF/dUdot] T(j,q) w(q)
                                                               S_J_ij  = sum_q sum_kl |T_k(i,q)| |C_kl(q)| |T_l(j,q)| w(q)
  y = A x:  S_y_i = sum_j S_J_ij |x_j|

with T the slot values of a basis function at a point (value and gradient components of its variable, zero elsewhere),
F the module's point function and C its derivative.  The criterion (distance): d = |got - yardstick| / (2^-53 S), and
got == 0.0 exactly where S == 0.

Reference lines restated here:
  * thermal::volumeResidual                  src/physics/thermal.cpp:125-163
  * navierstokes::volumeResidual, computeTau src/physics/navierstokes.cpp:82-849, :1054-1079 (uz through uy's offsets: :688)
  * linearelasticity::volumeResidual, computeStress  src/physics/linearelasticity.cpp:92-238, :985-1073
  * stokes::volumeResidual                   src/physics/stokes.cpp:178-438 (PSPG tau h / (2 nu) in 2-D :256, h^2 / (2 nu) in
                                             3-D :402; LSIC tested with the sum of the derivatives of q :283, :432)
  * shallowwater::volumeResidual             src/physics/shallowwater.cpp:118-153 (gravity 9.8: :32)
  * helmholtz::volumeResidual                src/physics/helmholtz.cpp:134-194 (vr and vi: :156-157, the two rows :175-193)
  * cdr::volumeResidual                      src/physics/cdr.cpp:62-142
  * navierstokes with have_energy            src/physics/navierstokes.cpp:134-141, :168-176, :471-483, :824-838 (the PSPG
                                             buoyancy part is not divided by the density)
  * thermal with have_nsvel, have_advection  src/physics/thermal.cpp:139-160
  * computeStress with e_num >= 0            src/physics/linearelasticity.cpp:1001-1011, :1024-1034, :1074-1084
  * Workset::computeSolnTransientSeeded      src/tools/workset.cpp:589-623
  * Workset::getElementSize                  src/tools/workset.cpp:2666-2679
  * the scatter (-res.val(), +res.dx(col), fixed rows skipped)  src/managers/assemblyManager.cpp:4031-4145
"""
import functools

import mpmath
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS64 = 2.0 ** -53
H_STEP = LD("1e-30")
_DPS = 40


# ---- measured constants -----------------------------------------------------------------------------------------------
# K_oracle[(module, family)]: the CPU oracle's largest distance d from this yardstick over every entry (element arrays,
# CRS values, residual) of every shape of the family, steady and transient, as tests/test_highprec.py measures and prints
# it (the measurement stands beside each constant; the table is in profiles/extended_precision_yardstick.md).
#   * thermal and navierstokes (the C oracle: plain loops, -ffp-contract=off, the same figure on every run): the next
#     integer that is at least one half above the measurement (above 1000: the next multiple of ten);
#   * linearelasticity and thermal's nonlinear diffusion (Python restatements on numpy's einsum, whose summation order
#     follows the vector units of the CPU it runs on): the measurement times 1.25, rounded up to two digits.
# The CPU test fails when the oracle exceeds its constant or falls below two thirds of it.  The device's bound is
# max(8 K_oracle, 8).
K_ORACLE = {
    ("thermal",          "unit"):              23,      # measured 22.10
    ("thermal",          "stretched aligned"): 23,      # measured 21.74
    ("thermal",          "stretched sheared"): 1120,    # measured 1119
    ("thermal",          "stretched warped"):  28,      # measured 26.94
    ("thermal",          "units small"):       22,      # measured 21.13
    ("thermal",          "units large"):       23,      # measured 21.99
    ("thermal",          "unit advection"):    23,      # measured 22.31
    ("thermal",          "unit nonlinear"):    25,      # measured 19.82 (Python restatement)
    ("navierstokes",     "unit"):              23,      # measured 22.23
    ("navierstokes",     "stretched aligned"): 45,      # measured 43.90
    ("navierstokes",     "stretched sheared"): 1020,    # measured 1018
    ("navierstokes",     "stretched warped"):  69,      # measured 67.98
    ("navierstokes",     "units small"):       41,      # measured 40.41
    ("navierstokes",     "units large"):       26,      # measured 24.96
    ("navierstokes",     "rest"):              63,      # measured 62.36
    ("linearelasticity", "unit"):              23,      # measured 18.28
    ("linearelasticity", "stretched aligned"): 25,      # measured 19.83
    ("linearelasticity", "stretched sheared"): 1300,    # measured 1029
    ("linearelasticity", "stretched warped"):  26,      # measured 20.08
    ("linearelasticity", "units small"):       25,      # measured 19.28
    ("linearelasticity", "units large"):       23,      # measured 18.38
    ("linearelasticity", "unit plane stress"): 23,      # measured 18.28
    # the later point-engine modules: Python restatements on einsum, every one (the measurement times 1.25)
    ("cdr",                      "unit"):               18,      # measured 14.1
    ("cdr",                      "stretched aligned"):  26,      # measured 20.18
    ("cdr",                      "stretched sheared"):  1400,    # measured 1045
    ("cdr",                      "stretched warped"):   27,      # measured 21.06
    ("cdr",                      "units small"):        19,      # measured 14.95
    ("cdr",                      "units large"):        16,      # measured 12.66
    ("cdr",                      "unit fields"):        21,      # measured 16.07
    ("cdr",                      "unit arrays"):        19,      # measured 14.52
    ("helmholtz",                "unit"):               19,      # measured 14.49
    ("helmholtz",                "stretched aligned"):  23,      # measured 18.11
    ("helmholtz",                "stretched sheared"):  1400,    # measured 1048
    ("helmholtz",                "stretched warped"):   25,      # measured 19.66
    ("helmholtz",                "units small"):        22,      # measured 16.88
    ("helmholtz",                "units large"):        22,      # measured 17.51
    ("helmholtz",                "unit all functions"): 15,      # measured 11.36
    ("stokes",                   "unit"):               24,      # measured 18.79 (the worst of the four PSPG / LSIC settings)
    ("stokes",                   "stretched aligned"):  27,      # measured 21.49
    ("stokes",                   "stretched sheared"):  1800,    # measured 1372
    ("stokes",                   "stretched warped"):   47,      # measured 36.93
    ("stokes",                   "units small"):        34,      # measured 26.85
    ("stokes",                   "units large"):        34,      # measured 26.69
    ("shallowwater",             "unit"):               44,      # measured 35.06 (the stage-1 residual: the seeded xi_t cancels)
    ("shallowwater",             "stretched aligned"):  65,      # measured 51.79
    ("shallowwater",             "stretched sheared"):  1800,    # measured 1383
    ("shallowwater",             "stretched warped"):   44,      # measured 34.69
    ("shallowwater",             "units small"):        44,      # measured 34.67
    ("shallowwater",             "units large"):        47,      # measured 37.2
    ("shallowwater",             "small elevation"):    73,      # measured 57.92 (D D - b b cancels: its own round-off)
    ("navierstokes+thermal",     "unit"):               43,      # measured 34.28
    ("navierstokes+thermal",     "stretched aligned"):  96,      # measured 76.46
    ("navierstokes+thermal",     "stretched sheared"):  1300,    # measured 1022
    ("navierstokes+thermal",     "stretched warped"):   45,      # measured 35.93
    ("navierstokes+thermal",     "units small"):        49,      # measured 38.61
    ("navierstokes+thermal",     "units large"):        56,      # measured 44.3
    ("navierstokes+thermal",     "unit plain"):         43,      # measured 34.28
    ("navierstokes+thermal",     "rest"):               44,      # measured 34.84
    ("linearelasticity+thermal", "unit"):               31,      # measured 24.16
    ("linearelasticity+thermal", "stretched aligned"):  24,      # measured 18.75
    ("linearelasticity+thermal", "stretched sheared"):  1800,    # measured 1394
    ("linearelasticity+thermal", "stretched warped"):   34,      # measured 26.64
    ("linearelasticity+thermal", "units small"):        27,      # measured 21.15
    ("linearelasticity+thermal", "units large"):        28,      # measured 22
    ("linearelasticity+thermal", "unit plane stress"):  30,      # measured 23.69
    ("navierstokes+cdr",         "unit"):               24,      # measured 18.97
    ("navierstokes+cdr",         "stretched aligned"):  36,      # measured 28.71
    ("navierstokes+cdr",         "stretched sheared"):  1200,    # measured 889.3
    ("navierstokes+cdr",         "stretched warped"):   42,      # measured 33.1
    ("navierstokes+cdr",         "units small"):        34,      # measured 26.78
    ("navierstokes+cdr",         "units large"):        57,      # measured 45.22
    ("navierstokes+cdr",         "unit fields"):        27,      # measured 20.91
}


def device_bound(module, family):
    return max(8.0 * K_ORACLE[(module, family)], 8.0)


# ---- 1-D ingredients: mpmath at 40 digits, rounded once ---------------------------------------------------------------
def _ld(x):
    return LD(mpmath.nstr(x, 30, strip_zeros=False))


@functools.lru_cache(maxsize=None)
def gauss_mp(n):
    """Gauss-Legendre points and weights on [-1, 1] as mpf: the roots of P_n, w = 2 / ((1 - x^2) P_n'(x)^2)."""
    with mpmath.workdps(max(_DPS, mpmath.mp.dps)):
        P = lambda x: mpmath.legendre(n, x)
        xs = [mpmath.findroot(P, mpmath.cos(mpmath.pi * (4 * k + 3) / (4 * n + 2))) for k in range(n)]
        xs = sorted(xs)
        for a, b in zip(xs, xs[1:]):
            assert b - a > mpmath.mpf(10) ** -10, "a root found twice"
        ws = []
        for x in xs:
            dP = n * (x * mpmath.legendre(n, x) - mpmath.legendre(n - 1, x)) / (x * x - 1)
            ws.append(2 / ((1 - x * x) * dP * dP))
        return tuple(xs), tuple(ws)


def gauss_npts(degree):
    return degree // 2 + 1


def lagrange_mp(order, x):
    """Values and derivatives at x (mpf) of the Lagrange polynomials on the order + 1 equispaced nodes of [-1, 1]."""
    with mpmath.workdps(max(_DPS, mpmath.mp.dps)):
        nd = [mpmath.mpf(-1) + mpmath.mpf(2 * k) / order for k in range(order + 1)]
        val, der = [], []
        for k in range(order + 1):
            v = mpmath.mpf(1)
            for m in range(order + 1):
                if m != k:
                    v *= (x - nd[m]) / (nd[k] - nd[m])
            d = mpmath.mpf(0)
            for l in range(order + 1):
                if l == k:
                    continue
                t = 1 / (nd[k] - nd[l])
                for m in range(order + 1):
                    if m != k and m != l:
                        t *= (x - nd[m]) / (nd[k] - nd[m])
                d += t
            val.append(v)
            der.append(d)
        return val, der


@functools.lru_cache(maxsize=None)
def line_tables(order, npts):
    """(points [q], weights [q], values [order + 1][q], derivatives [order + 1][q]) as longdouble."""
    xs, ws = gauss_mp(npts)
    V, D = np.zeros((order + 1, npts), LD), np.zeros((order + 1, npts), LD)
    for q, x in enumerate(xs):
        v, d = lagrange_mp(order, x)
        for k in range(order + 1):
            V[k, q], D[k, q] = _ld(v[k]), _ld(d[k])
    return np.array([_ld(x) for x in xs]), np.array([_ld(w) for w in ws]), V, D


@functools.lru_cache(maxsize=None)
def node_tables(order, at_order):
    """Lagrange values of `order` at the equispaced nodes of `at_order`: [order + 1][at_order + 1] (longdouble)."""
    with mpmath.workdps(max(_DPS, mpmath.mp.dps)):
        V = np.zeros((order + 1, at_order + 1), LD)
        for j in range(at_order + 1):
            v, _ = lagrange_mp(order, mpmath.mpf(-1) + mpmath.mpf(2 * j) / at_order)
            for k in range(order + 1):
                V[k, j] = _ld(v[k])
        return V


# ---- tensor products ----------------------------------------------------------------------------------------------------
def _tensor(dim, V, D):
    """Tensor product of 1-D tables V, D [f][q]: B [f^dim][q^dim], G [..][..][dim]; the x index runs fastest."""
    if dim == 2:
        B = np.einsum("bj,ai->baji", V, V)
        G = np.stack([np.einsum("bj,ai->baji", V, D), np.einsum("bj,ai->baji", D, V)], axis=-1)
    else:
        B = np.einsum("ck,bj,ai->cbakji", V, V, V)
        G = np.stack([np.einsum("ck,bj,ai->cbakji", V, V, D), np.einsum("ck,bj,ai->cbakji", V, D, V),
                      np.einsum("ck,bj,ai->cbakji", D, V, V)], axis=-1)
    nf, nq = V.shape[0] ** dim, V.shape[1] ** dim
    return B.reshape(nf, nq), G.reshape(nf, nq, dim)


def _vertex_perm(dim):
    """Tensor index (x fastest) of the vertices in the cell's vertex order: counter-clockwise bottom, then top."""
    sg = [(0, 0), (1, 0), (1, 1), (0, 1)]
    if dim == 2:
        return [a + 2 * b for a, b in sg]
    return [a + 2 * b + 4 * c for c in (0, 1) for a, b in sg]


def ref_tables(dim, order, qdeg):
    """Reference-cell tables: B [f][q], G [f][q][dim] of the order-`order` basis, NV / NG of the multilinear vertex
    functions (cell vertex order), w [q]."""
    npts = gauss_npts(qdeg)
    _, w1, V, D = line_tables(order, npts)
    _, _, V1, D1 = line_tables(1, npts)
    B, G = _tensor(dim, V, D)
    NV, NG = _tensor(dim, V1, D1)
    perm = _vertex_perm(dim)
    w = w1
    for _ in range(dim - 1):
        w = np.multiply.outer(w1, w).reshape(-1)
    return dict(B=B, G=G, NV=NV[perm], NG=NG[perm], w=w)


# ---- geometry -----------------------------------------------------------------------------------------------------------
def cofactor_inverse(J):
    """det [..] and inverse [..][d][d] of J [..][d][d] by cofactors (numpy.linalg has no longdouble)."""
    d = J.shape[-1]
    if d == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        adj = np.stack([np.stack([J[..., 1, 1], -J[..., 0, 1]], -1), np.stack([-J[..., 1, 0], J[..., 0, 0]], -1)], -2)
    else:
        c = lambda i, j, k, l: J[..., i, j] * J[..., k, l] - J[..., i, l] * J[..., k, j]
        adj = np.stack([np.stack([c(1, 1, 2, 2), -c(0, 1, 2, 2), c(0, 1, 1, 2)], -1),
                        np.stack([-c(1, 0, 2, 2), c(0, 0, 2, 2), -c(0, 0, 1, 2)], -1),
                        np.stack([c(1, 0, 2, 1), -c(0, 0, 2, 1), c(0, 0, 1, 1)], -1)], -2)
        det = J[..., 0, 0] * adj[..., 0, 0] + J[..., 0, 1] * adj[..., 1, 0] + J[..., 0, 2] * adj[..., 2, 0]
    return det, adj / det[..., None, None]


def geometry(nodes, rt):
    """x [E][q][dim], Jinv [E][q][dim][dim], wts [E][q] of the multilinear map of nodes [E][2^dim][dim]."""
    X = np.asarray(nodes).astype(LD)
    x = np.einsum("evi,vq->eqi", X, rt["NV"])
    J = np.einsum("evi,vqj->eqij", X, rt["NG"])        # J_ij = d x_i / d xi_j
    det, Jinv = cofactor_inverse(J)
    assert np.all(det > 0)
    return x, Jinv, rt["w"][None, :] * det


# ---- the block: slot tables T, seeding ----------------------------------------------------------------------------------
class Block:
    """m: a mesh dict of tests/oracle_lib.py's layout (nodes, lids, offsets, ndof and, for several variables, orders and
    varptr; a single-variable mesh gives `order`).  Slots: variable v -> [value, d/dx, d/dy(, d/dz)] at v (1 + dim)."""

    def __init__(self, m, qdeg, order=None, test_var=None, test_slots=None):
        self.nodes = np.asarray(m["nodes"], dtype=np.float64)
        self.lids = np.asarray(m["lids"])
        self.E, self.n = self.lids.shape
        self.dim = dim = self.nodes.shape[2]
        self.ndof = int(m["ndof"])
        off = np.asarray(m["offsets"])
        if order is not None:
            self.orders, self.offs = [int(order)], [off]
        else:
            self.orders = [int(o) for o in m["orders"]]
            self.offs = [off[m["varptr"][v]:m["varptr"][v + 1]] for v in range(len(self.orders))]
        self.nv, self.S = len(self.orders), 1 + dim
        K = self.nv * self.S
        rt0 = ref_tables(dim, 1, qdeg)
        self.x, Jinv, self.w = geometry(self.nodes, rt0)
        self.nq = self.w.shape[1]
        self.h = (self.w.sum(axis=1) ** (LD(1) / dim))[:, None]        # getElementSize
        T = np.zeros((self.E, self.n, self.nq, K), LD)
        for v, (o, of) in enumerate(zip(self.orders, self.offs)):
            rt = ref_tables(dim, o, qdeg)
            assert len(of) == rt["B"].shape[0]
            T[:, of, :, v * self.S:v * self.S + 1] = rt["B"][None, :, :, None]
            T[:, of, :, v * self.S + 1:(v + 1) * self.S] = np.einsum("eqji,fqj->efqi", Jinv, rt["G"])   # J^-T grad
        self.T = T
        # rows: test_var[v] = the variable through whose offsets the rows of v's equation are scattered
        self.Ttest = T
        if test_var is not None and list(test_var) != list(range(self.nv)):
            self.Ttest = np.zeros_like(T)
            for v, tv in enumerate(test_var):
                assert self.orders[v] == self.orders[tv]
                self.Ttest[:, self.offs[tv], :, v * self.S:(v + 1) * self.S] += T[:, self.offs[v], :, v * self.S:(v + 1) * self.S]
        # test_slots[g] = (rv, bv): the point function gives len(test_slots) groups of 1 + dim outputs; group g multiplies
        # basis function i of variable bv (value, gradient) and goes to row i of variable rv (helmholtz: vr and vi apart)
        if test_slots is not None:
            assert test_var is None
            self.Ttest = np.zeros((self.E, self.n, self.nq, len(test_slots) * self.S), LD)
            for g, (rv, bv) in enumerate(test_slots):
                assert self.orders[rv] == self.orders[bv]
                self.Ttest[:, self.offs[rv], :, g * self.S:(g + 1) * self.S] += T[:, self.offs[bv], :, bv * self.S:(bv + 1) * self.S]

    # -- its own check of the dof ordering -------------------------------------------------------------------------------
    def check_ordering(self):
        """(1) every global row sits at one physical point in all elements that share it; (2) the nodal field a . x(node)
        comes out of the tables as a . x(q) with gradient a.  Returns the node coordinates [ndof][dim]."""
        dim = self.dim
        X = self.nodes.astype(LD)
        size = (X.max(axis=1) - X.min(axis=1)).max(axis=1)                         # [E]
        xn = np.full((self.ndof, dim), np.nan, LD)
        perm = _vertex_perm(dim)
        for v, (o, of) in enumerate(zip(self.orders, self.offs)):
            V1 = node_tables(1, o)
            NVn, _ = _tensor(dim, V1, np.zeros_like(V1))
            pts = np.einsum("evi,vf->efi", X, NVn[perm])                          # node of basis function f
            rows = self.lids[:, of]
            for e in range(self.E):
                for f in range(len(of)):
                    r = rows[e, f]
                    if np.isnan(xn[r, 0]):
                        xn[r] = pts[e, f]
                    assert np.abs(xn[r] - pts[e, f]).max() <= 1e-12 * size[e], ("row placed at two points", v, e, f)
        assert not np.isnan(xn).any(), "a row that no element reaches"
        a = np.array([0.7, -1.3, 0.45], LD)[:dim]
        U = self.fields((xn * a).sum(axis=1)[self.lids])
        tol = 1e-15 * max(float(np.abs(xn).max()), float(size.max()))
        for v in range(self.nv):
            assert np.abs(U[v * self.S] - (self.x * a).sum(axis=2)).max() <= tol, ("a . x(node) != a . x(q)", v)
            for d in range(dim):
                assert np.abs(U[v * self.S + 1 + d] - a[d]).max() <= 1e-15 * float(size.max() / size.min() * 1e3), v
        return xn

    # -- fields and seeding ----------------------------------------------------------------------------------------------
    def fields(self, ue):
        """ue [E][n] (LID-position order) -> slot values [K][E][q]."""
        return np.einsum("epqk,ep->keq", self.T, ue)

    def seeded(self, u, tr):
        """Stage value and time derivative of every row, and (alpha_u, alpha_t): workset.cpp:589-623."""
        cu = np.asarray(u).astype(LD)
        if tr is None:
            return cu, np.zeros_like(cu), LD(1), LD(0)
        A, b, bdf = (np.asarray(tr[k]).astype(LD) for k in ("butcher_A", "butcher_b", "bdf"))
        st, dt = tr["stage"], LD(tr["dt"])
        up, us = np.asarray(tr["u_prev"]).astype(LD), np.asarray(tr["u_stage"]).astype(LD)
        alpha_u = A[st, st] / b[st]
        timewt = LD(1) / dt / b[st]
        alpha_t = bdf[0] * timewt
        beta_u = (LD(1) - alpha_u) * up[:, 0]
        for s in range(st):
            beta_u = beta_u + A[st, s] / b[s] * (us[:, s] - up[:, 0])
        beta_t = np.zeros_like(cu)
        for s in range(1, len(bdf)):
            beta_t = beta_t + bdf[s] * up[:, s - 1]
        beta_t = beta_t * timewt
        return alpha_u * cu + beta_u, alpha_t * cu + beta_t, alpha_u, alpha_t


# ---- the modules as point functions F(U, Udot, x, params) ----------------------------------------------------------------
def func_value(spec, x, env=None):
    """A function of the deck at the points x [E][q][dim]: a number, ("sinprod", amp, freq), ("array", a) -- per-point
    data [E][q], as the device takes it from a tensor -- or (callable, deck text): the device and the float64 oracle get
    the text, the yardstick calls the callable with env(), the slot values by their deck names ("c", "c_t",
    "grad(c)[x]", "ux", "x", ...), so that a string that reads the fields is differentiated by the complex step."""
    if isinstance(spec, (int, float)):
        return LD(spec)
    if isinstance(spec, mpmath.mpf):                            # the point functions on mpf (tests/test_highprec.py)
        return spec
    if callable(spec[0]):
        return spec[0](env())
    if spec[0] == "array":
        return np.asarray(spec[1]).astype(LD)
    assert spec[0] == "sinprod"
    v = LD(spec[1])
    for d in range(x.shape[2]):
        v = v * np.sin(LD(spec[2][d]) * x[..., d])
    return v


def deck_function(spec):
    """What the device and the float64 oracle are given for a function: the text of a (callable, text) pair, else spec."""
    return spec[1] if isinstance(spec, tuple) and callable(spec[0]) else spec


def slot_env(names, U, Ud, x):
    """The slot values by the names a deck string reads them under (Workset::getSolutionField) and the coordinates."""
    dim = x.shape[2]
    S = 1 + dim

    def env():
        f = {c: x[..., d] for d, c in enumerate("xyz"[:dim])}
        for v, nm in enumerate(names):
            f[nm], f[nm + "_t"] = U[v * S], Ud[v * S]
            for d, c in enumerate("xyz"[:dim]):
                f["grad(%s)[%s]" % (nm, c)] = U[v * S + 1 + d]
        return f
    return env


def thermal_point(U, Ud, x, P):
    """thermal.cpp:125-163.  params: source, diffusion (a number, sinprod, or a callable of e: "1+e*e"), rho, cp, and
    adv = (bx, by[, bz]) or None ('include advection')."""
    dim = x.shape[2]
    kap = P["diffusion"](U[0]) if callable(P["diffusion"]) else func_value(P["diffusion"], x)
    F = [None] * (1 + dim)
    F[0] = LD(P["rho"]) * LD(P["cp"]) * Ud[0] - func_value(P["source"], x)
    for d in range(dim):
        F[1 + d] = kap * U[1 + d]
    if P.get("adv") is not None:
        for d in range(dim):
            F[0] = F[0] + func_value(P["adv"][d], x) * U[1 + d]
    return F


def _num(v):
    """A number of the deck as longdouble; an mpf stays (the point functions on mpf, tests/test_highprec.py)."""
    return v if isinstance(v, mpmath.mpf) else LD(v)


def compute_tau(visc, vel, h, dt, transient):
    """navierstokes.cpp:1054-1079; the branch nvel > 1e-12 is taken on the real part."""
    C1, C2, C3 = LD(4), LD(2), LD(2) if transient else LD(0)
    nvel = vel[0] * vel[0]
    for v in vel[1:]:
        nvel = nvel + v * v
    if isinstance(nvel, mpmath.mpf):                            # on mpf: the same branch and formula, one point
        nvel = mpmath.sqrt(nvel) if nvel > 1e-12 else nvel
        tau = (4 * visc / h / h) * (4 * visc / h / h) + (2 * nvel / h) * (2 * nvel / h) + (int(C3) / dt) * (int(C3) / dt)
        return 1 / mpmath.sqrt(tau)
    nvel = np.where(np.real(nvel) > 1e-12, np.sqrt(np.where(np.real(nvel) > 1e-12, nvel, 1)), nvel)
    tau = (C1 * visc / h / h) * (C1 * visc / h / h) + (C2 * nvel / h) * (C2 * nvel / h) + (C3 / dt) * (C3 / dt)
    return 1 / np.sqrt(tau)


def navierstokes_point(U, Ud, x, P):
    """navierstokes.cpp:82-849, variables ux, pr, uy[, uz]; params: source ux / uy / uz, density, viscosity, useSUPG,
    usePSPG, h [E][1], dt, transient.  (The uz rows go through uy's offsets unless fix_uz_offsets: Block(test_var=...).)"""
    dim = x.shape[2]
    S = 1 + dim
    vn, pn = [0, 2, 3][:dim], 1
    dens, visc = func_value(P["density"], x), func_value(P["viscosity"], x)
    src = [func_value(P["source u" + c], x) for c in "xyz"[:dim]]
    vel = [U[v * S] for v in vn]
    pr = U[pn * S]
    supg, pspg = bool(P.get("useSUPG")), bool(P.get("usePSPG"))
    tau = compute_tau(visc, vel, P["h"], _num(P["dt"]), bool(P["transient"])) if supg or pspg else None
    F = [None] * ((dim + 1) * S)
    divu = 0
    strong = []
    # have_energy (the coupled block navierstokes+thermal): P["energy"] = (the variable number of e, beta, T_ambient)
    buoy = None
    if P.get("energy") is not None:
        ev, beta, T0 = P["energy"]
        buoy = [dens * _num(beta) * (U[ev * S] - _num(T0)) * src[i] for i in range(dim)]   # :141, :176, :480
    for i, v in enumerate(vn):
        b = v * S
        conv = sum(vel[d] * U[b + 1 + d] for d in range(dim))
        F[b] = (Ud[b] + conv - src[i]) * dens                                  # F of :520-521
        for d in range(dim):
            F[b + 1 + d] = visc * U[b + 1 + d] - (pr if d == i else 0)           # Fx, Fy, Fz of :514-519
        divu = divu + U[b + 1 + i]
        # stabres of :554 (= Sx / (tau wts / dens) of :813)
        strong.append(dens * Ud[b] + dens * conv + U[pn * S + 1 + i] - dens * src[i])
        if supg:
            for d in range(dim):
                F[b + 1 + d] = F[b + 1 + d] + tau * strong[i] * vel[d]          # :555-559
        if buoy is not None:
            F[b] = F[b] + buoy[i]                                                # :134-147
            if supg:
                for d in range(dim):
                    F[b + 1 + d] = F[b + 1 + d] + tau * buoy[i] * vel[d]        # :168-185
    F[pn * S] = divu                                                            # :782-784
    for d in range(dim):
        F[pn * S + 1 + d] = strong[d] * tau / dens if pspg else 0 * pr          # :813-820
        if pspg and buoy is not None:
            F[pn * S + 1 + d] = F[pn * S + 1 + d] + buoy[d] * tau                # :471-488, :824-845: not over the density
    return F


def linearelasticity_point(U, Ud, x, P):
    """linearelasticity.cpp:92-238 with computeStress :985-1073; variables dx, dy[, dz]; params: lambda, mu, source dx /
    dy / dz, incplanestress."""
    dim = x.shape[2]
    S = 1 + dim
    lam, mu = func_value(P["lambda"], x), func_value(P["mu"], x)
    g = lambda i, j: U[i * S + 1 + j]                                            # grad(d_i)[j]
    F = [None] * (dim * S)
    for i in range(dim):
        F[i * S] = -func_value(P["source d" + "xyz"[i]], x) + 0 * U[0]
        for j in range(dim):
            if i != j:
                sig = mu * (g(i, j) + g(j, i))
            elif dim == 2 and P.get("incplanestress"):
                sig = 4 * mu * g(i, i) + 2 * mu * g(1 - i, 1 - i)                 # :995, :998
            else:
                sig = (2 * mu + lam) * g(i, i) + lam * sum(g(k, k) for k in range(dim) if k != i)
            F[i * S + 1 + j] = sig
    return F


def stokes_point(U, Ud, x, P):
    """stokes.cpp:178-438, variables ux, pr, uy[, uz]; params: source ux / uy / uz, viscosity, usePSPG, useLSIC, h.  No
    time term; "source pr" is read by no term; the uz rows go through their own offsets."""
    dim = x.shape[2]
    S = 1 + dim
    vn, pn = [0, 2, 3][:dim], 1
    visc = func_value(P["viscosity"], x)
    src = [func_value(P["source u" + c], x) for c in "xyz"[:dim]]
    pr, h = U[pn * S], P["h"]
    F = [None] * ((dim + 1) * S)
    divu = 0
    for i, v in enumerate(vn):
        b = v * S
        F[b] = -src[i] + 0 * pr                                                  # g of :197, :218, :364
        for d in range(dim):
            F[b + 1 + d] = visc * U[b + 1 + d] - (pr if d == i else 0)           # Fx, Fy, Fz of :193-195, :312-316
        divu = divu + U[b + 1 + i]
    F[pn * S] = divu                                                            # :236, :382
    for d in range(dim):
        F[pn * S + 1 + d] = 0 * pr
    if P.get("usePSPG"):
        tau = (h if dim == 2 else h * h) / (2.0 * visc)                          # :256 and :402
        for d in range(dim):
            F[pn * S + 1 + d] = F[pn * S + 1 + d] + (U[pn * S + 1 + d] + src[d]) * tau      # :257-262, :403-410
    if P.get("useLSIC"):
        tau = h * h / (2.0 * visc)                                               # :279, :428
        for d in range(dim):
            F[pn * S + 1 + d] = F[pn * S + 1 + d] + tau * divu                   # S (q_x + q_y [+ q_z]) of :283, :432
    return F


def shallowwater_point(U, Ud, x, P):
    """shallowwater.cpp:118-153, variables H (holding the surface elevation xi), Hu, Hv; params: bathymetry, bathymetry_x,
    bathymetry_y, source H / Hu / Hv, gravity."""
    S = 3
    fv = lambda k: func_value(P[k], x)
    bath, g = fv("bathymetry"), P.get("gravity", 9.8)                            # :32
    xi, Hu, Hv = U[0], U[S], U[2 * S]
    F = [None] * (3 * S)
    F[0], F[1], F[2] = Ud[0] - fv("source H"), -Hu, -Hv                          # :124-126
    D = xi + bath                                                                # :131
    uHu, uHv, vHv = Hu * Hu / D, Hu * Hv / D, Hv * Hv / D                        # :132-134
    pres = 0.5 * g * (D * D - bath * bath)                                       # :137, :145
    F[S] = Ud[S] - g * xi * fv("bathymetry_x") - fv("source Hu")                 # :136
    F[S + 1], F[S + 2] = -(uHu + pres), -uHv                                     # :137-138
    F[2 * S] = Ud[2 * S] - g * xi * fv("bathymetry_y") - fv("source Hv")         # :143
    F[2 * S + 1], F[2 * S + 2] = -uHv, -(vHv + pres)                             # :144-145
    return F


HELMHOLTZ_TEST_SLOTS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (the variable whose rows, the variable whose basis)


def helmholtz_point(U, Ud, x, P):
    """helmholtz.cpp:134-194, the non-fractional branch, variables ureal, uimag, with vr = ureal's basis function i and
    vi = uimag's basis function i kept apart: four groups of test slots (Block(test_slots=HELMHOLTZ_TEST_SLOTS)) -- what
    multiplies (vr, grad vr) and (vi, grad vi) in the ureal row :175-182, then the same of the uimag row :186-193.
    params: c2r_x .. c2i_z, omega2r, omega2i, source_r, source_i.  No time term."""
    dim = x.shape[2]
    S = 1 + dim
    fv = lambda k: func_value(P[k], x)
    o2r, o2i, sr, si = fv("omega2r"), fv("omega2i"), fv("source_r"), fv("source_i")
    ur, ui = U[0], U[S]
    F = [None] * (4 * S)
    F[0] = -o2r * ur + o2i * ui - sr                                             # the ureal row, vr
    F[S] = -o2r * ui - o2i * ur - si                                             # the ureal row, vi
    F[2 * S] = -o2r * ui - o2i * ur - si                                         # the uimag row, vr
    F[3 * S] = o2r * ur - o2i * ui + sr                                          # the uimag row, vi
    for d, c in enumerate("xyz"[:dim]):
        c2r, c2i = fv("c2r_" + c), fv("c2i_" + c)
        dur, dui = U[1 + d], U[S + 1 + d]
        F[1 + d] = c2r * dur - c2i * dui
        F[S + 1 + d] = c2r * dui + c2i * dur
        F[2 * S + 1 + d] = c2r * dui + c2i * dur
        F[3 * S + 1 + d] = -c2r * dur + c2i * dui
    return F


def cdr_row(U, Ud, x, P, names):
    """cdr.cpp:112-140 on c, the LAST variable of names: [f, Fx, Fy(, Fz)].  params: source, diffusion, specific heat,
    density, reaction, xvel, yvel, zvel; each may read the fields ((callable, text), func_value)."""
    dim = x.shape[2]
    S = 1 + dim
    b = (len(names) - 1) * S
    env = slot_env(names, U, Ud, x)
    fv = lambda k: func_value(P[k], x, env)
    f = Ud[b] + fv("reaction") - fv("source")                                    # no rho cp on the time derivative
    for d, c in enumerate("xyz"[:dim]):
        f = f + fv(c + "vel") * U[b + 1 + d]
    kd = 1.0 / (fv("density") * fv("specific heat")) * fv("diffusion")
    return [f] + [kd * U[b + 1 + d] for d in range(dim)]


def cdr_point(U, Ud, x, P):
    return cdr_row(U, Ud, x, P, ["c"])


def navierstokes_cdr_point(U, Ud, x, P):
    """navierstokes' rows as navierstokes_point gives them, then cdr's on c; "density" is one function for both."""
    dim = x.shape[2]
    return navierstokes_point(U, Ud, x, P) + cdr_row(U, Ud, x, P, ["ux", "pr", "uy", "uz"][:dim + 1] + ["c"])


def navierstokes_thermal_point(U, Ud, x, P):
    """navierstokes with have_energy, then thermal.cpp:125-163 with have_nsvel on e, the last variable; params besides
    navierstokes': thermal source, thermal diffusion, specific heat, beta, T_ambient, include advection with bx, by, bz."""
    dim = x.shape[2]
    S = 1 + dim
    vn, b = [0, 2, 3][:dim], (dim + 1) * S
    fv = lambda k: func_value(P[k], x)
    F = navierstokes_point(U, Ud, x, dict(P, energy=(dim + 1, P["beta"], P["T_ambient"])))
    f = fv("density") * fv("specific heat") * Ud[b] - fv("thermal source")       # :131
    for d in range(dim):
        f = f + U[vn[d] * S] * U[b + 1 + d]                                       # :139-149
        if P.get("include advection"):
            f = f + fv("b" + "xyz"[d]) * U[b + 1 + d]                             # :150-160
    return F + [f] + [fv("thermal diffusion") * U[b + 1 + d] for d in range(dim)]


def linearelasticity_thermal_point(U, Ud, x, P):
    """linearelasticity with e_num >= 0: every normal stress gets -alpha_T (e - T_ambient) c, c = 3 lambda + 2 mu, or 5 mu
    under incplanestress in 2-D (linearelasticity.cpp:1007-1008, :1030-1031, :1080-1082); then thermal.cpp:125-163 without
    have_nsvel on e, the last variable."""
    dim = x.shape[2]
    S = 1 + dim
    b = dim * S
    fv = lambda k: func_value(P[k], x)
    lam, mu = fv("lambda"), fv("mu")
    F = linearelasticity_point(U, Ud, x, P)
    c = 5 * mu if dim == 2 and P.get("incplanestress") else 3 * lam + 2 * mu
    th = _num(P["alpha_T"]) * (U[b] - _num(P["T_ambient"])) * c
    for i in range(dim):
        F[i * S + 1 + i] = F[i * S + 1 + i] - th
    f = fv("density") * fv("specific heat") * Ud[b] - fv("thermal source")
    if P.get("include advection"):
        for d in range(dim):
            f = f + fv("b" + "xyz"[d]) * U[b + 1 + d]
    return F + [f] + [fv("thermal diffusion") * U[b + 1 + d] for d in range(dim)]


POINT = {"thermal": thermal_point, "navierstokes": navierstokes_point, "linearelasticity": linearelasticity_point,
         "stokes": stokes_point, "shallowwater": shallowwater_point, "helmholtz": helmholtz_point, "cdr": cdr_point,
         "navierstokes+cdr": navierstokes_cdr_point, "navierstokes+thermal": navierstokes_thermal_point,
         "linearelasticity+thermal": linearelasticity_thermal_point}


def _stack(F, like):
    return np.stack([np.broadcast_to(np.asarray(f, dtype=like.dtype), like.shape[1:]) for f in F])


def point_derivative(point, U, Ud, x, P):
    """F [K out][E][q], dF/dU and dF/dUdot [K out][K in][E][q] by the complex step Im F(U + i h e_k) / h, h = 1e-30."""
    K = U.shape[0]
    Uc, Udc = U.astype(CLD), Ud.astype(CLD)
    F = np.real(_stack(point(Uc, Udc, x, P), Uc)).astype(LD)
    CU, CT = np.zeros((F.shape[0], K) + U.shape[1:], LD), np.zeros((F.shape[0], K) + U.shape[1:], LD)
    S = 1 + x.shape[2]
    for k in range(K):
        Up = Uc.copy()
        Up[k] += 1j * H_STEP
        CU[:, k] = np.imag(_stack(point(Up, Udc, x, P), Uc)) / H_STEP
        if k % S == 0:                               # only the value slots have a time derivative
            Up = Udc.copy()
            Up[k] += 1j * H_STEP
            CT[:, k] = np.imag(_stack(point(Uc, Up, x, P), Uc)) / H_STEP
    return F, CU, CT


# ---- element arrays and their scales --------------------------------------------------------------------------------------
def element_arrays(blk, module, P, u, tr=None):
    """-> dict(local_res, local_J, S_res, S_J) in LID-position order [E][n], [E][n][n] (longdouble); local_res holds -R
    and local_J +dR/du, the sign conventions of the ABI."""
    ue, ud, alpha_u, alpha_t = blk.seeded(u, tr)
    U, Ud = blk.fields(ue[blk.lids]), blk.fields(ud[blk.lids])
    P = dict(P, h=blk.h, transient=tr is not None, dt=tr["dt"] if tr is not None else 1.0)
    F, CU, CT = point_derivative(POINT[module], U, Ud, blk.x, P)
    C = alpha_u * CU + alpha_t * CT
    E, n, nq, K = blk.T.shape
    Tt, Tr, w = blk.Ttest, blk.T, blk.w
    Fw = np.transpose(F, (1, 2, 0)) * w[..., None]                       # [E][q][K]
    Cw = np.transpose(C, (2, 3, 0, 1)) * w[..., None, None]              # [E][q][K out][K in]
    out = {}
    for tag, (a, f, c, b) in (("", (Tt, Fw, Cw, Tr)), ("S_", (np.abs(Tt), np.abs(Fw), np.abs(Cw), np.abs(Tr)))):
        r = np.einsum("eiqk,eqk->ei", a, f)
        Pm = np.einsum("eiqk,eqkl->eiql", a, c).reshape(E, n, nq * K)    # P = T C
        Jm = np.matmul(Pm, np.transpose(b.reshape(E, n, nq * K), (0, 2, 1)))   # then P T
        out[tag + "res"], out[tag + "J"] = r, Jm
    return dict(local_res=-out["res"], local_J=out["J"], S_res=out["S_res"], S_J=out["S_J"])


# ---- assembly -------------------------------------------------------------------------------------------------------------
def build_graph(ndof, lids):
    """CRS graph of the element connectivity: every row's columns ascending."""
    cols = [set() for _ in range(ndof)]
    for e in range(lids.shape[0]):
        s = set(int(c) for c in lids[e])
        for r in s:
            cols[r] |= s
    rowptr = np.zeros(ndof + 1, np.int32)
    rowptr[1:] = np.cumsum([len(c) for c in cols])
    colind = np.array([c for cs in cols for c in sorted(cs)], np.int32)
    return rowptr, colind


def assemble(blk, el, fixed=None):
    """Element arrays -> dict(rowptr, colind, crs_vals, res, S_vals, S_res [global]); fixed rows are zero rows (what
    assemble_jacres(..., overwrite=True) leaves).  The scales assemble as the values do: sums of the element scales."""
    lids, nd = blk.lids, blk.ndof
    rowptr, colind = build_graph(nd, lids)
    rows = np.repeat(np.arange(nd), np.diff(rowptr))
    key = rows.astype(np.int64) * nd + colind
    ek = lids[:, :, None].astype(np.int64) * nd + lids[:, None, :]
    idx = np.searchsorted(key, ek)
    assert np.array_equal(key[idx], ek)
    free = np.ones(nd, bool) if fixed is None else ~np.asarray(fixed, bool)
    mr, mj = free[lids], np.broadcast_to(free[lids][:, :, None], ek.shape)
    out = dict(rowptr=rowptr, colind=colind)
    for name, loc, glob, size in (("res", "local_res", lids, nd), ("S_res", "S_res", lids, nd)):
        a = np.zeros(size, LD)
        np.add.at(a, glob[mr], el[loc][mr])
        out[name] = a
    for name, loc in (("crs_vals", "local_J"), ("S_vals", "S_J")):
        a = np.zeros(len(colind), LD)
        np.add.at(a, idx[mj], el[loc][mj])
        out[name] = a
    return out


def matvec(g, X, transpose=False):
    """(A X[k], S of it) for the rows of X [K][ndof] with the assembled matrix of g (longdouble)."""
    X = np.atleast_2d(np.asarray(X)).astype(LD)
    nd = len(g["rowptr"]) - 1
    rows = np.repeat(np.arange(nd), np.diff(g["rowptr"]))
    r, c = (g["colind"], rows) if transpose else (rows, g["colind"])
    Y, SY = np.zeros(X.shape, LD), np.zeros(X.shape, LD)
    for k in range(X.shape[0]):
        np.add.at(Y[k], r, g["crs_vals"] * X[k, c])
        np.add.at(SY[k], r, g["S_vals"] * np.abs(X[k, c]))
    return Y, SY


def diagonal(g):
    nd = len(g["rowptr"]) - 1
    rows = np.repeat(np.arange(nd), np.diff(g["rowptr"]))
    on = rows == g["colind"]
    d, s = np.zeros(nd, LD), np.zeros(nd, LD)
    d[rows[on]], s[rows[on]] = g["crs_vals"][on], g["S_vals"][on]
    return d, s


# ---- the criterion ----------------------------------------------------------------------------------------------------------
def distance(got, ref, S):
    """max over ALL entries of |got - ref| / (2^-53 S); inf if an entry with S == 0 is not exactly 0.0, and inf if any
    entry of got is not finite (a NaN must not pass for want of an ordering)."""
    got, ref, S = np.asarray(got), np.asarray(ref), np.asarray(S)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(S)), "the yardstick itself is not finite"
    if not np.all(np.isfinite(got)):
        return float("inf")
    zero = S == 0
    if np.any(got[zero] != 0.0) or np.any(ref[zero] != 0):
        return float("inf")
    if zero.all():
        return 0.0
    d = np.abs(got[~zero].astype(LD) - ref[~zero]) / (LD(EPS64) * S[~zero])
    d = float(d.max())
    return d if d == d else float("inf")


# ---- the cases: shapes, input families, data ---------------------------------------------------------------------------------
TABLEAU = dict(butcher_A=np.array([[0.5, 0.0], [0.3, 0.7]]), butcher_b=np.array([0.4, 0.6]),
               bdf=np.array([1.5, -2.0, 0.5]), stage=1)        # the two-stage tableau of tests/test_multi_gpu.py

SHAPES = {  # module -> (name, dim, ncell, orders)
    "thermal": [("Q1 quad", 2, (3, 2), (1,)), ("Q2 quad", 2, (3, 2), (2,)), ("Q3 quad", 2, (2, 2), (3,)),
                ("Q4 quad", 2, (2, 2), (4,)), ("Q1 hex", 3, (2, 2, 2), (1,)), ("Q2 hex", 3, (2, 2, 2), (2,))],
    "navierstokes": [("2-D Q2/Q1", 2, (3, 2), (2, 1, 2)), ("3-D Q1/Q1", 3, (2, 2, 2), (1, 1, 1, 1)),
                     ("3-D Q2/Q1", 3, (2, 1, 1), (2, 1, 2, 2))],
    "linearelasticity": [("2-D Q1", 2, (3, 2), (1, 1)), ("2-D Q2", 2, (3, 2), (2, 2)), ("3-D Q1", 3, (2, 2, 2), (1, 1, 1)),
                         ("3-D Q2", 3, (2, 1, 1), (2, 2, 2))],
    # the later point-engine modules: the shapes of their own GPU tests, the smallest that reach every instantiation family
    "cdr": [("2-D Q1", 2, (3, 2), (1,)), ("2-D Q2", 2, (3, 2), (2,)), ("3-D Q1", 3, (2, 3, 2), (1,)), ("3-D Q2", 3, (2, 2, 2), (2,))],
    "helmholtz": [("2-D Q1", 2, (3, 3), (1, 1)), ("2-D Q2", 2, (2, 2), (2, 2)), ("3-D Q1", 3, (2, 2, 2), (1, 1)),
                  ("3-D Q2", 3, (2, 2, 1), (2, 2))],
    "stokes": [("2-D Q1/Q1", 2, (3, 3), (1, 1, 1)), ("2-D Q2/Q1", 2, (3, 3), (2, 1, 2)), ("3-D Q1/Q1", 3, (2, 2, 2), (1, 1, 1, 1)),
               ("3-D Q2/Q1", 3, (2, 2, 2), (2, 1, 2, 2))],
    "shallowwater": [("2-D Q1", 2, (3, 3), (1, 1, 1)), ("2-D Q2", 2, (3, 3), (2, 2, 2))],
    "navierstokes+thermal": [("2-D Q2/Q1/Q2", 2, (3, 2), (2, 1, 2, 2)), ("3-D Q1", 3, (2, 2, 2), (1, 1, 1, 1, 1))],
    "linearelasticity+thermal": [("2-D Q1/Q1", 2, (4, 3), (1, 1, 1)), ("2-D Q2/Q1", 2, (4, 3), (2, 2, 1)),
                                 ("3-D Q2/Q1", 3, (2, 2, 2), (2, 2, 2, 1))],
    "navierstokes+cdr": [("2-D Q1", 2, (3, 2), (1, 1, 1, 1)), ("2-D Q2/Q1/Q2", 2, (3, 2), (2, 1, 2, 2)),
                         ("3-D Q1", 3, (2, 2, 2), (1, 1, 1, 1, 1))],
}
FAMILIES = ["unit", "stretched aligned", "stretched sheared", "stretched warped", "units small", "units large"]
# the terms of thermal that only the point engine has, on the unit family's inputs: (b . grad e, v) and kappa = 1 + e*e
THERMAL_ONLY = ["unit advection", "unit nonlinear"]
# the branches that only one of the later modules has, on the unit family's geometry
MODULE_ONLY = {
    "thermal": THERMAL_ONLY, "navierstokes": ["rest"], "linearelasticity": ["unit plane stress"],
    "cdr": ["unit fields", "unit arrays"],                 # deck strings that read c, c_t, grad(c); every function per point
    "navierstokes+cdr": ["unit fields"],                   # ... and ux
    "helmholtz": ["unit all functions"],                   # the ten volume functions non-zero, different in every direction
    "navierstokes+thermal": ["unit plain", "rest"],        # no stabilisation, b . grad e; computeTau at |u| = 0
    "linearelasticity+thermal": ["unit plane stress"],
    "shallowwater": ["small elevation"],                   # |xi| ~ 1e-3 b: D D - b b cancels
}
# stokes: the four (usePSPG, useLSIC) settings under ONE family key (the worst d over the four)
VARIANTS = {"stokes": [dict(usePSPG=0, useLSIC=0), dict(usePSPG=1, useLSIC=0), dict(usePSPG=0, useLSIC=1), dict(usePSPG=1, useLSIC=1)]}
# the deck's names per module: the functions the yardstick reads, the physics parameters
NS_FUNCS = ["source ux", "source uy", "source uz", "viscosity", "density"]
LE_FUNCS = ["lambda", "mu", "source dx", "source dy", "source dz"]
MODULE_FUNCS = {
    "navierstokes": NS_FUNCS, "linearelasticity": LE_FUNCS,
    "stokes": ["source ux", "source uy", "source uz", "viscosity"],
    "shallowwater": ["bathymetry", "bathymetry_x", "bathymetry_y", "source H", "source Hu", "source Hv"],
    "helmholtz": ["c2r_x", "c2i_x", "c2r_y", "c2i_y", "c2r_z", "c2i_z", "omega2r", "omega2i", "source_r", "source_i"],
    "cdr": ["source", "diffusion", "specific heat", "density", "reaction", "xvel", "yvel", "zvel"],
    "navierstokes+cdr": NS_FUNCS + ["source", "diffusion", "specific heat", "reaction", "xvel", "yvel", "zvel"],
    "navierstokes+thermal": NS_FUNCS + ["thermal source", "thermal diffusion", "specific heat", "bx", "by", "bz"],
    "linearelasticity+thermal": LE_FUNCS + ["thermal source", "thermal diffusion", "specific heat", "density", "bx", "by", "bz"],
}
MODULE_PARAMS = {
    "navierstokes": ["useSUPG", "usePSPG", "fix_uz_offsets"], "linearelasticity": ["incplanestress"],
    "stokes": ["usePSPG", "useLSIC"], "shallowwater": [], "helmholtz": [], "cdr": [],
    "navierstokes+cdr": ["useSUPG", "usePSPG", "fix_uz_offsets"],
    "navierstokes+thermal": ["useSUPG", "usePSPG", "fix_uz_offsets", "beta", "T_ambient", "include advection"],
    "linearelasticity+thermal": ["incplanestress", "alpha_T", "T_ambient", "include advection"],
}


def families(module):
    return FAMILIES + MODULE_ONLY.get(module, [])


def transients(module, family):
    """steady and stage 1; the nonlinear diffusion's oracle (oracle_lib.assemble_thermal_fields) is steady only."""
    return (False,) if family == "unit nonlinear" else (False, True)


def case_list(module, family):
    """(shape, transient, variant) of every case of a (module, family) key."""
    return [(shape, tr, v) for shape in SHAPES[module] for tr in transients(module, family)
            for v in range(len(VARIANTS.get(module, [None])))]


def deck(c):
    """(functions, physics parameters) of a case as the device and the float64 restatements are given them: names of the
    third direction left out in 2-D, deck text for (callable, text), the named helper strings, and the functions that the
    reference registers and no term reads."""
    P, z = c["P"], c["dim"] == 2
    funcs = {k: deck_function(P[k]) for k in MODULE_FUNCS[c["module"]]
             if k in P and not (z and (k.endswith("z") or k == "zvel"))}
    funcs.update(P.get("unread", {}))
    funcs.update(P.get("helpers", {}))
    return funcs, {k: P[k] for k in MODULE_PARAMS[c["module"]] if k in P}


def sinprod_text(spec, dim):
    """("sinprod", amp, freq) as a deck string."""
    return "*".join([repr(float(spec[1]))] + ["sin(%r*%s)" % (float(spec[2][d]), "xyz"[d]) for d in range(dim)])


def map_vertices(v, family):
    """The family's geometry from the unit-box vertices v [nv][dim] (doubles; the yardstick takes them as exact)."""
    dim = v.shape[1]
    v = v.copy()
    warp = v.copy()
    warp[:, 0] += 0.06 * np.sin(1.3 * v[:, 1] + 0.4) + (0.04 * v[:, 2] ** 2 if dim == 3 else 0.0)
    warp[:, 1] += 0.05 * np.cos(1.1 * v[:, 0]) * (1 + 0.5 * v[:, 1])
    if dim == 3:
        warp[:, 2] += 0.05 * v[:, 0] * v[:, 1] + 0.03 * np.sin(2.0 * v[:, 2])
    stretch = np.array([1.0, 1e-3, 1.0])[:dim]                  # 1 : 1000 boxes
    if family in ("unit", "rest", "unit plane stress") + tuple(THERMAL_ONLY):
        return warp
    if family == "stretched aligned":
        return v * stretch
    if family == "stretched sheared":
        A = np.eye(dim) + 0.25 * np.array([[0.3, 0.8, -0.4], [-0.5, 0.2, 0.6], [0.7, -0.3, 0.1]])[:dim, :dim]
        return (v * stretch) @ A.T + 0.3
    if family == "stretched warped":
        return warp * stretch
    if family == "units small":
        return warp * 1e-3
    if family == "units large":
        return warp * 1e3
    raise ValueError(family)


def case_data(module, family, dim, ndof, dof_var, transient, seed=97):
    """-> (u, tr, params): the state, the transient dict (or None) and the module's functions / parameters."""
    rng = np.random.default_rng(seed)
    # "units small": lengths 1e-3 with coefficients 1e+6; "units large": lengths 1e+3 with coefficients 1e-6
    L = {"units small": 1e-3, "units large": 1e3}.get(family, 1.0)          # length scale
    coef = {"units small": 1e6, "units large": 1e-6}.get(family, 1.0)
    amp = 1e3 if family.startswith("units") else 1.0
    u = amp * rng.uniform(-1, 1, ndof)
    tr = None
    if transient:
        # dt scaled to match: the diffusive time L^2 / kappa (thermal), the advective time L / |u| (navierstokes)
        dt = 0.05 * {"thermal": L * L / coef, "navierstokes": L / amp, "linearelasticity": 1.0}[module]
        tr = dict(TABLEAU, dt=dt, u_prev=amp * rng.uniform(-1, 1, (ndof, 2)), u_stage=amp * rng.uniform(-1, 1, (ndof, 2)))
    fr = [f / L for f in (1.3, 0.7, 2.1)[:dim]]
    if module == "thermal":
        P = dict(source=("sinprod", 3.0 * amp * coef / (L * L), fr), diffusion=1.7 * coef, rho=1.3, cp=0.7, adv=None)
        if family == "unit advection":
            P["adv"] = (0.8, -0.5, 0.3)[:dim]
        if family == "unit nonlinear":
            P["diffusion"], P["diffusion_text"] = (lambda e: 1 + e * e), "1+e*e"
    elif module == "navierstokes":
        P = {"source ux": 0.3, "source uy": ("sinprod", 1.0, fr), "source uz": -0.2, "viscosity": 0.05 * coef,
             "density": 1.3, "useSUPG": 1, "usePSPG": 1, "fix_uz_offsets": 0}
        if family == "rest":                                    # the other side of nvel > 1e-12: every velocity dof 0
            P["fix_uz_offsets"] = 1                             # ... and the uz rows through their own offsets
            for a in (u,) + ((tr["u_prev"], tr["u_stage"]) if tr else ()):
                a[np.asarray(dof_var) != 1] = 0.0
    else:
        P = {"lambda": 1.1 * coef, "mu": 0.6 * coef, "source dx": 0.3, "source dy": ("sinprod", 1.0, fr), "source dz": -0.2,
             "incplanestress": 1 if family == "unit plane stress" else 0}   # 2-D: lambda = 2 mu (:990-1000); 3-D ignores it
    return u, tr, P


LATER = ("cdr", "helmholtz", "stokes", "shallowwater", "navierstokes+thermal", "linearelasticity+thermal", "navierstokes+cdr")


def later_case_data(module, family, dim, ndof, dof_var, transient, variant, nelem, nq, seed=131):
    """case_data of the later point-engine modules.  Every coefficient, source and dt follows the units: with lengths L,
    coefficients coef and amplitudes amp the terms of each equation keep their unit-family balance, so no term drops
    below the others' round-off."""
    rng = np.random.default_rng(seed)
    L = {"units small": 1e-3, "units large": 1e3}.get(family, 1.0)
    coef = {"units small": 1e6, "units large": 1e-6}.get(family, 1.0)
    amp = 1e3 if family.startswith("units") else 1.0
    dof_var = np.asarray(dof_var)
    u = amp * rng.uniform(-1, 1, ndof)
    # the time scales: diffusive L^2 / kappa, advective L / |u|, the gravity wave's L (shallowwater; g is not scaled)
    diffusive, advective = L * L / coef, L / amp
    dt = 0.05 * {"cdr": diffusive, "linearelasticity+thermal": diffusive, "shallowwater": L, "helmholtz": L}.get(module, advective)
    tr = None
    if transient:
        tr = dict(TABLEAU, dt=dt, u_prev=amp * rng.uniform(-1, 1, (ndof, 2)), u_stage=amp * rng.uniform(-1, 1, (ndof, 2)))
    fr = [f / L for f in (1.3, 0.7, 2.1)[:dim]]
    fr2 = [f / L for f in (0.9, 1.6, 1.1)[:dim]]
    per_point = lambda lo, hi: ("array", rng.uniform(lo, hi, (nelem, nq)))
    ns = lambda: {"source ux": 0.3 * amp * amp / L, "source uy": ("sinprod", 1.0 * amp * amp / L, fr), "source uz": -0.2 * amp * amp / L,
                  "viscosity": 0.05 * coef, "density": 1.3, "useSUPG": 1, "usePSPG": 1, "fix_uz_offsets": 0,
                  "unread": {"source pr": 5.0}}

    def at_rest():                                              # the other side of nvel > 1e-12: every velocity dof 0
        for a in (u,) + ((tr["u_prev"], tr["u_stage"]) if tr else ()):
            a[(dof_var != 1) & (dof_var != dim + 1)] = 0.0

    if module == "stokes":
        f = coef * amp / (L * L)                                # the viscous force nu u / L^2
        P = {"source ux": 0.3 * f, "source uy": ("sinprod", 1.0 * f, fr), "source uz": -0.2 * f, "viscosity": 0.7 * coef,
             "unread": {"source pr": 5.0}}
        P.update(VARIANTS["stokes"][variant])
    elif module == "shallowwater":
        xi = dof_var == 0
        small = 1e-3 if family == "small elevation" else 1.0    # |xi| ~ 1e-3 b, of both signs; else xi in [0.5, 1.5] amp
        sign = rng.choice([-1.0, 1.0], int(xi.sum())) if family == "small elevation" else 1.0
        u[xi] = small * amp * sign * rng.uniform(0.5, 1.5, int(xi.sum()))
        if tr is not None:                                      # every xi array the same draw plus a small one of its own:
            for k in ("u_prev", "u_stage"):                     # the seeded depth stays positive
                tr[k][xi] = u[xi][:, None] + small * amp * rng.uniform(-0.05, 0.05, tr[k][xi].shape)
        # (slopes of the order of b / L: g xi b_x keeps a share of its entries beside the pressure flux that the bound sees)
        P = {"bathymetry": ("array", amp * rng.uniform(0.5, 1.5, (nelem, nq))), "bathymetry_x": 0.5 * amp / L,
             "bathymetry_y": ("sinprod", -0.8 * amp / L, fr), "source H": 0.2 * amp / L, "source Hu": ("sinprod", 0.4 * amp * amp / L, fr2),
             "source Hv": -0.1 * amp * amp / L, "unread": {"viscosity": 3.0, "Coriolis": 2.0}}
    elif module == "helmholtz":
        k2, s = coef / (L * L), amp * coef / (L * L)
        P = {"omega2r": 2.1 * k2, "omega2i": 0.3 * k2, "source_r": ("sinprod", 2.0 * s, fr), "source_i": 0.4 * s}
        P.update({"c2r_" + c: 1.3 * coef for c in "xyz"}, **{"c2i_" + c: 0.4 * coef for c in "xyz"})
        if family == "unit all functions":
            P.update({"c2r_x": 1.3, "c2r_y": 0.8, "c2r_z": 1.9, "c2i_x": 0.4, "c2i_y": -0.6, "c2i_z": 0.25,
                      "omega2r": ("sinprod", 2.1, fr2), "omega2i": per_point(0.2, 0.5), "source_i": ("sinprod", -1.5, fr2)})
    elif module == "cdr":
        k2 = coef / (L * L)
        P = {"source": ("sinprod", 2.0 * amp * k2, fr), "diffusion": 0.9 * coef, "specific heat": 1.4, "density": 1.3,
             "reaction": 0.6 * amp * k2, "xvel": 0.7 * coef / L, "yvel": -1.1 * coef / L, "zvel": 0.4 * coef / L,
             "unread": {"SUPG tau": 3.0}}
        if family == "unit arrays":
            P.update({"source": per_point(-2, 2), "diffusion": per_point(0.5, 1.5), "specific heat": per_point(1, 2),
                      "density": per_point(1, 2), "reaction": per_point(-1, 1), "xvel": per_point(-1, 1),
                      "yvel": per_point(-1, 1), "zvel": per_point(-1, 1)})
    elif module == "navierstokes+cdr":
        P = ns()
        P.update({"source": ("sinprod", 2.0 * amp * amp / L, fr2), "diffusion": 0.9 * coef, "specific heat": 1.4,
                  "reaction": 0.6 * amp * amp / L, "xvel": 0.7 * amp, "yvel": -1.1 * amp, "zvel": 0.4 * amp})
    elif module == "navierstokes+thermal":
        P = ns()
        P.update({"thermal source": ("sinprod", 3.0 * amp * amp / L, fr2), "thermal diffusion": 1.7 * coef, "specific heat": 1.4,
                  "beta": 0.7 / amp, "T_ambient": 0.3 * amp, "include advection": 0})
        if family == "unit plain":
            P.update({"useSUPG": 0, "usePSPG": 0, "include advection": 1, "bx": 0.8, "by": -0.5, "bz": 0.3})
        if family == "rest":
            P["fix_uz_offsets"] = 1
            at_rest()
    else:
        assert module == "linearelasticity+thermal"
        f, k2 = coef * amp / (L * L), amp * coef / (L * L)
        P = {"lambda": 1.1 * coef, "mu": 0.6 * coef, "source dx": 0.3 * f, "source dy": ("sinprod", 1.0 * f, fr), "source dz": -0.2 * f,
             "thermal source": ("sinprod", 3.0 * k2, fr2), "thermal diffusion": 1.7 * coef, "specific heat": 1.4, "density": 1.3,
             "incplanestress": 1 if family == "unit plane stress" else 0, "alpha_T": 0.35 / L, "T_ambient": 0.3 * amp,
             "include advection": 0}
    if family == "unit fields":
        # deck strings that read the fields, each with its callable twin on the slot values; powers written as products
        P["helpers"] = {"kappa0": "1+0.1*x"}
        P["reaction"] = (lambda f: 0.5 * f["c"] * f["c"] + 0.1 * f["grad(c)[x]"] * f["grad(c)[x]"], "0.5*c*c + 0.1*grad(c)[x]^2")
        P["diffusion"] = (lambda f: (1 + 0.1 * f["x"]) + f["c"] * f["c"], "kappa0+c*c")
        P["xvel"] = (lambda f: f["ux"], "ux") if module == "navierstokes+cdr" else (lambda f: f["c"], "c")
        if transient:
            P["yvel"] = (lambda f: 0.3 * f["c_t"], "0.3*c_t")
    return u, tr, P


def fixed_rows(module, m):
    """The strong rows, 10 - 30 % of all: the left side without its top edge (a whole side of a mesh two cells wide is a
    third of a Q1 variable's rows), never the pressure; shallowwater after its drop test: Hu on the left and right sides, Hv
    on the bottom."""
    side, var = m["side_mask"], m["dof_var"]
    if module == "shallowwater":
        return (((var == 1) & ((side & 0b0011) != 0)) | ((var == 2) & ((side & 0b0100) != 0))).astype(np.uint8)
    pinned = (side & 0b1001) == 0b0001
    if module in ("stokes", "navierstokes+thermal", "navierstokes+cdr"):
        pinned = pinned & (var != 1)
    return pinned.astype(np.uint8)


def in_point_order(meshlib, blk, qdeg, P):
    """P with every ("array", a) taken from the ABI's order of the integration points (meshlib's) to the yardstick's:
    an integer map, found by matching the points of the first element."""
    if not any(isinstance(v, tuple) and v[0] == "array" for v in P.values()):
        return P
    ip = meshlib.physical_basis_var(blk.dim, 0, 1, qdeg, blk.nodes[:1])["ip"][0]
    x = blk.x[0].astype(np.float64)
    dist = np.abs(x[:, None, :] - ip[None, :, :]).max(axis=2)
    perm = dist.argmin(axis=1)
    size = np.ptp(blk.nodes[0], axis=0).max()
    assert sorted(perm) == list(range(blk.nq)) and dist[np.arange(blk.nq), perm].max() < 1e-12 * size
    return {k: ("array", np.asarray(v[1])[:, perm]) if isinstance(v, tuple) and v[0] == "array" else v for k, v in P.items()}


_CASES = {}


def build_case(meshlib, module, shape, family, transient, variant=0):
    """One case, cached: mesh (meshlib: tests/oracle_lib.py, used for the structured mesh and its integer maps only),
    data, the yardstick's element arrays `el` and global arrays `g`."""
    key = (module, shape, family, transient, variant)
    if key in _CASES:
        return _CASES[key]
    name, dim, ncell, orders = shape
    if module == "thermal":
        m = meshlib.mesh_structured(dim, orders[0], ncell)
        m["dof_var"] = np.zeros(m["ndof"], np.int32)
        fixed = m["boundary"].copy()
    else:
        m = meshlib.mesh_multi(dim, ncell, [0] * len(orders), list(orders))
        pinned = (m["side_mask"] & 0b1100) != 0                               # strong Dirichlet rows on two sides
        fixed = (pinned & (m["dof_var"] != 1) if module == "navierstokes" else pinned).astype(np.uint8)
        if module in LATER:
            fixed = fixed_rows(module, m)
    m["verts"] = map_vertices(m["verts"], family if family in FAMILIES or module not in LATER else "unit")
    m["nodes"] = np.ascontiguousarray(m["verts"][m["cell2vert"]])
    qdeg = 2 * orders[0]
    if module in LATER:
        u, tr, P = later_case_data(module, family, dim, m["ndof"], m["dof_var"], transient, variant, m["nelem"],
                                   gauss_npts(qdeg) ** dim)
    else:
        u, tr, P = case_data(module, family, dim, m["ndof"], m["dof_var"], transient)
    # the uz rows through uy's offsets (navierstokes.cpp:688), in the coupled blocks too
    quirk = module.startswith("navierstokes") and dim == 3 and not P["fix_uz_offsets"]
    blk = Block(m, qdeg, order=orders[0] if module == "thermal" else None,
                test_var=([0, 1, 2, 2] + list(range(4, len(orders)))) if quirk else None,
                test_slots=HELMHOLTZ_TEST_SLOTS if module == "helmholtz" else None)
    blk.check_ordering()
    el = element_arrays(blk, module, in_point_order(meshlib, blk, qdeg, P), u, tr)
    c = dict(module=module, shape=shape, family=family, m=m, dim=dim, orders=orders, qdeg=qdeg, u=u, tr=tr, P=P, fixed=fixed,
             blk=blk, el=el, g=assemble(blk, el, fixed), variant=variant,
             tag="%s %s" % (name, "stage 1" if transient else "steady") +
                 ("" if module not in VARIANTS else " " + " ".join("%s=%d" % kv for kv in VARIANTS[module][variant].items())))
    _CASES[key] = c
    return c
