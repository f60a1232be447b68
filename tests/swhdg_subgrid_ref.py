"""The yardstick of the HDG subgrids of m x m sub-elements per macro element (mha_swhdg_set_subgrids,
mha_swhdg_condensed_subgrid, mha_swhdg_subgrid_blocks): a numpy restatement that assembles the dense (n_int + 24)^2 system
of every macro element from the unchanged oracle and condenses it with numpy.linalg.solve.

TEST INFRASTRUCTURE (the checker), imported by tests/test_swhdg_subgrids.py and tests/test_swhdg_subgrids_gpu.py only.

  * volume terms (shallowwaterHybridized::volumeResidual, src/physics/shallowwaterHybridized.cpp:113-184): the oracle's
    block assembly (orc_assemble_block, want_local) on the sub-mesh, summed into the interior rows through the sub-mesh
    LIDs (SubGridDtN_Solver::assembleJacobianResidual, src/subgrid/subgridDtN_solver.cpp:774-808);
  * side terms (boundaryResidual :190-263) on the 4m sub-sides of the macro boundary only, and the trace rows (computeFlux
    :270-368 against the macro trace basis, updateFlux subgridDtN_solver.cpp:1542-1616): the flux VALUE at every sub-side
    point is the oracle's point function orc_swh_interface_flux; its derivatives with respect to the interior and the
    trace state come from the same formulas run on the numpy forward-AD class of tests/oracle_lib.py, whose values are
    asserted against the oracle's at every point (the oracle exposes no point derivatives).  To be plain about it:
    _interface_flux_ad below RESTATES the side physics in test code; it is not taken from the oracle.  Only its values
    are checked against orc_swh_interface_flux directly; its derivatives are pinned indirectly, by the m = 1 comparison
    with orc_swh_hdg_element (whose blocks are the oracle's own AD) and by the central finite difference of the
    restatement's residual, both in tests/test_swhdg_subgrids.py;
  * the trace state at a sub-side point is the macro edge's HFACE basis there (src/subgrid/subgridDtN.cpp:746-870): on
    macro edge k sub-side j of m covers the edge coordinate [-1 + 2j/m, -1 + 2(j+1)/m];
  * seeding: Workset::computeSolnTransientSeeded (src/tools/workset.cpp:589-623).

Orders: sub-elements of macro element k are elements [k m^2, (k+1) m^2), row-major with x fastest; interior unknowns of a
macro element are flattened (variable, node), node = ay (m+1) + ax; traces (variable, HFACE edge left/bottom/right/top,
function); rows / columns of a block = n_int interior then 24 traces; res = -res.val(), blocks = res(r).dx(c)."""
import numpy as np

HFACE_EDGE = (1, 2, 3, 0)          # shards side (bottom, right, top, left) -> HFACE edge
SHV = (0, 1, 3, 2)                 # dof (x fastest) -> shards vertex


def subgrid_mesh(ncell, m, lo=(0.0, 0.0), hi=(1.0, 1.0), warp=None):
    """ncell macro quads, each an m x m sub-mesh.  warp(xy [.., 2]) -> xy moves the MACRO vertices; the sub-mesh is the
    bilinear image of the uniform subdivision of each (warped) macro quad, as the layout requires.
    -> dict(nodes [E][4][2], lids [E][12], offsets [12], trace_lids [Em][24], nelem, nmacro, ndof, ntrace, n_int, m)."""
    nx, ny = ncell
    Em, npn = nx * ny, (m + 1) ** 2
    E = Em * m * m
    nodes, lids = np.zeros((E, 4, 2)), np.zeros((E, 12), np.int32)
    offsets = np.array([SHV[d] * 3 + v for v in range(3) for d in range(4)], np.int32)
    hx, hy = (hi[0] - lo[0]) / nx, (hi[1] - lo[1]) / ny
    vx, vy = (0, 1, 1, 0), (0, 0, 1, 1)
    nvert = (nx + 1) * ny
    trace = np.zeros((Em, 24), np.int32)
    for J in range(ny):
        for I in range(nx):
            k = J * nx + I
            c = np.array([[lo[0] + hx * (I + vx[s]), lo[1] + hy * (J + vy[s])] for s in range(4)])
            if warp is not None:
                c = warp(c)
            for ey in range(m):
                for ex in range(m):
                    e = k * m * m + ey * m + ex
                    for sv in range(4):
                        ax, ay = ex + vx[sv], ey + vy[sv]
                        s, t = ax / m, ay / m
                        if warp is None:   # the mesh helper's own arithmetic, bit for bit
                            nodes[e, sv] = (lo[0] + hx * (I + ax / m), lo[1] + hy * (J + ay / m))
                        else:
                            nodes[e, sv] = (1 - s) * (1 - t) * c[0] + s * (1 - t) * c[1] + s * t * c[2] + (1 - s) * t * c[3]
                        lids[e, sv * 3:sv * 3 + 3] = (k * npn + ay * (m + 1) + ax) * 3 + np.arange(3)
            edges = (J * (nx + 1) + I, nvert + J * nx + I, J * (nx + 1) + I + 1, nvert + (J + 1) * nx + I)
            for v in range(3):
                for ed in range(4):
                    for f in range(2):
                        trace[k, (v * 4 + ed) * 2 + f] = (edges[ed] * 3 + v) * 2 + f
    return dict(nodes=nodes, lids=lids, offsets=offsets, trace_lids=trace, nelem=E, nmacro=Em, ndof=Em * 3 * npn,
                ntrace=6 * ((nx + 1) * ny + nx * (ny + 1)), n_int=3 * npn, m=m, dim=2)


def macro_warp(c):
    """A smooth warp of macro vertices: non-affine macro quads, hence non-constant sub-element Jacobians."""
    w = c.copy()
    w[..., 0] += 0.07 * np.sin(2.0 * c[..., 1]) * (1.0 + 0.3 * c[..., 0])
    w[..., 1] += 0.05 * c[..., 0] ** 2 + 0.03 * np.cos(1.7 * c[..., 0] + c[..., 1])
    return w


def select_macros(sm, ks):
    """The sub-mesh of the macro elements ks alone (rows renumbered macro by macro) -> (mesh, rows of the full vector)."""
    m, ni = sm["m"], sm["n_int"]
    ks = np.asarray(ks)
    el = (ks[:, None] * m * m + np.arange(m * m)[None]).ravel()
    lids = sm["lids"][el]
    rows = np.unique(lids)
    new = np.full(sm["ndof"], -1, np.int64)
    new[rows] = np.arange(len(rows))
    out = dict(sm, nodes=sm["nodes"][el].copy(), lids=new[lids].astype(np.int32), trace_lids=sm["trace_lids"][ks].copy(),
               nelem=len(el), nmacro=len(ks), ndof=len(rows))
    return out, rows


def oracle_mesh(oracle, sm):
    H = oracle.HGRAD
    return dict(dim=2, types=np.array([H] * 3, np.int32), orders=np.array([1] * 3, np.int32), nodes=sm["nodes"],
                lids=sm["lids"], offsets=sm["offsets"], orient=np.ones((sm["nelem"], 12), np.int8), ndof=sm["ndof"],
                nelem=sm["nelem"], n_tot=12)


def interior_rows(sm):
    """rows [Em][n_int]: global row of interior unknown (variable, node) of every macro element."""
    m, Em, ni = sm["m"], sm["nmacro"], sm["n_int"]
    npn = (m + 1) ** 2
    rows = np.full((Em, ni), -1, np.int64)
    L = sm["lids"].reshape(Em, m, m, 12)
    off = sm["offsets"]
    for ey in range(m):
        for ex in range(m):
            for v in range(3):
                for aa in range(4):
                    node = (ey + (aa >> 1)) * (m + 1) + ex + (aa & 1)
                    rows[:, v * npn + node] = L[:, ey, ex, off[v * 4 + aa]]
    return rows


def time_coeffs(tr):
    """alpha_u, alpha_t and the stage value / time derivative of every row (computeSolnTransientSeeded, seedwhat 1)."""
    if tr is None:
        return 1.0, 0.0, None, None
    st, A, b, bdf = tr["stage"], tr["butcher_A"], tr["butcher_b"], tr["bdf"]
    alpha_u, timewt = A[st, st] / b[st], 1.0 / tr["dt"] / b[st]
    alpha_t = bdf[0] * timewt
    up, us = tr["u_prev"], tr["u_stage"]
    beta_u = (1.0 - alpha_u) * up[:, 0]
    for s in range(st):
        beta_u = beta_u + A[st, s] / b[s] * (us[:, s] - up[:, 0])
    beta_t = np.zeros(len(up))
    for s in range(1, up.shape[1] + 1):
        beta_t = beta_t + bdf[s] * up[:, s - 1]
    return alpha_u, alpha_t, beta_u, beta_t * timewt


def _interface_flux_ad(oracle, stype, roe, S, Sh, Sinf, nx, ny, g):
    """computeFlux (:270-368) with computeFluxVector, computeStabilizationTerm (:487-588), computeBoundaryTerm (:595-758) and
    eigendecompFluxJacobian (:793-823) on AD views; S, Sh: lists of three ADView over the points of ONE side type."""
    AD = oracle.ADView
    nx, ny = AD(nx, W=6), AD(ny, W=6)  # (constants, lifted here: a bare array on the left of an operator would spread over the view)
    sqrt = lambda a: AD(np.sqrt(a.val), (0.5 / np.sqrt(a.val))[..., None] * a.dx)
    absv = lambda a: AD(np.abs(a.val), np.sign(a.val)[..., None] * a.dx)

    def pick(c, a, b):  # c ? a : b on values
        return AD(np.where(c, a.val, b.val), np.where(c[..., None], a.dx, b.dx))

    def eig(Sh):
        ux, uy = Sh[1] / Sh[0], Sh[2] / Sh[0]
        vn, a = ux * nx + uy * ny, sqrt(Sh[0] * g)
        one, zero = ux * 0.0 + 1.0, ux * 0.0
        R = [[one, zero, one], [ux + a * nx, -(a * ny), ux - a * nx], [uy + a * ny, a * nx, uy - a * ny]]
        two_a = a * 2.0
        L = [[0.5 - vn / two_a, nx / two_a, ny / two_a], [(ux * ny - uy * nx) / a, -(ny / a), nx / a],
             [0.5 + vn / two_a, -(nx / two_a), -(ny / two_a)]]
        return L, [vn + a, vn, vn - a], R

    mv = lambda A, x: [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(3)]
    if stype == 0:
        hh = Sh[0] * Sh[0] * (0.5 * g)
        F = [[Sh[1], Sh[2]], [Sh[1] * Sh[1] / Sh[0] + hh, Sh[1] * Sh[2] / Sh[0]], [Sh[1] * Sh[2] / Sh[0], Sh[2] * Sh[2] / Sh[0] + hh]]
        dS = [S[i] - Sh[i] for i in range(3)]
        if roe:
            L, lam, R = eig(Sh)
            t = mv(L, dS)
            stab = mv(R, [t[i] * absv(lam[i]) for i in range(3)])
        else:
            vn, a = Sh[1] / Sh[0] * nx + Sh[2] / Sh[0] * ny, sqrt(Sh[0] * g)
            p, q = absv(vn + a), absv(vn - a)
            lmax = pick(p.val > q.val, p, q)
            stab = [dS[i] * lmax for i in range(3)]
        return [F[i][0] * nx + F[i][1] * ny + stab[i] for i in range(3)]
    if stype == 1:
        L, lam, R = eig(Sh)
        t = mv(L, [S[i] - Sh[i] for i in range(3)])
        out = mv(R, [t[i] * ((lam[i] + absv(lam[i])) * 0.5) for i in range(3)])
        t = mv(L, [Sinf[i] - Sh[i] for i in range(3)])
        neg = mv(R, [t[i] * ((lam[i] - absv(lam[i])) * 0.5) for i in range(3)])
        return [out[i] - neg[i] for i in range(3)]
    vn = S[1] / S[0] * nx + S[2] / S[0] * ny
    return [S[0] - Sh[0], (S[1] / S[0] - vn * nx) - Sh[1] / Sh[0], (S[2] / S[0] - vn * ny) - Sh[2] / Sh[0]]


def point_fluxes(oracle, stypes, roe, S, Sh, ff, nrm, g):
    """S, Sh [P][3], nrm [P][2], stypes [P] -> flux [P][3] (the oracle's point function), dS, dSh [P][3][3] (AD restatement,
    values asserted against the oracle's)."""
    P = len(S)
    flux, dS, dSh = np.zeros((P, 3)), np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
    for p in range(P):
        flux[p] = oracle.swh_interface_flux(2, int(stypes[p]), roe, S[p], Sh[p], ff, nrm[p], g)
    for t in range(3):
        sel = np.flatnonzero(stypes == t)
        if len(sel) == 0:
            continue
        seed = lambda vals, base: [oracle.ADView(vals[sel, i], np.eye(6)[base + i][None].repeat(len(sel), 0)) for i in range(3)]
        f = _interface_flux_ad(oracle, t, roe, seed(S, 0), seed(Sh, 3), ff, nrm[sel, 0], nrm[sel, 1], g)
        for i in range(3):
            assert np.abs(f[i].val - flux[sel, i]).max() <= 1e-13 * max(1.0, np.abs(flux[sel]).max()), (t, i)
            dS[sel, i], dSh[sel, i] = f[i].dx[:, :3], f[i].dx[:, 3:]
    return flux, dS, dSh


def assemble(oracle, sm, qdeg, u, lam, side_types, ff, g=9.81, roe=True, transient=None, funcs=None):
    """The uncondensed system of every macro element -> res [Em][n_int+24], blocks [Em][n_int+24][n_int+24]."""
    m, Em, ni = sm["m"], sm["nmacro"], sm["n_int"]
    npn, N = (m + 1) ** 2, sm["n_int"] + 24
    u = np.asarray(u, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64).reshape(Em, 3, 4, 2)
    res, blocks = np.zeros((Em, N)), np.zeros((Em, N, N))
    om = oracle_mesh(oracle, sm)
    off = sm["offsets"]
    # ---- volume: the oracle's element blocks on the sub-mesh, summed through the sub-mesh LIDs ----
    vol = oracle.assemble_block(om, oracle.PHYS_SHALLOWWATER_HYBRIDIZED, qdeg, u, params=[g], transient=transient,
                                want_local=True, funcs=funcs)
    lJ = vol["local_J"][:, off][:, :, off].reshape(Em, m, m, 12, 12)
    lr = vol["local_res"][:, off].reshape(Em, m, m, 12)
    loc = lambda ex, ey: np.array([v * npn + (ey + (aa >> 1)) * (m + 1) + ex + (aa & 1) for v in range(3) for aa in range(4)])
    for ey in range(m):
        for ex in range(m):
            gidx = loc(ex, ey)
            blocks[:, gidx[:, None], gidx[None, :]] += lJ[:, ey, ex]
            res[:, gidx] += lr[:, ey, ex]
    # ---- sides: the 4m sub-sides on the macro boundary ----
    alpha_u, _, beta_u, _ = time_coeffs(transient)
    ue = u if transient is None else alpha_u * u + beta_u
    rows = interior_rows(sm)
    tab = oracle.side_tables(2, 1, qdeg)
    sip, sb = tab["sip"], tab["sbasis"]                     # [4][nqs][2], [4][4][nqs]
    nqs = sip.shape[1]
    for s in range(4):
        edge = HFACE_EDGE[s]
        for j in range(m):
            ex = m - 1 if s == 1 else (0 if s == 3 else j)
            ey = 0 if s == 0 else (m - 1 if s == 2 else j)
            el = (np.arange(Em) * m * m + ey * m + ex).astype(np.int32)
            geo = oracle.physical_side_basis(2, 1, qdeg, sm["nodes"], el, np.full(Em, s, np.int32))
            gidx = loc(ex, ey).reshape(3, 4)                # interior index of (variable, dof)
            uloc = ue[rows[:, gidx]]                        # [Em][3][4]
            for q in range(nqs):
                tl = sip[s, q, 1] if edge in (0, 2) else sip[s, q, 0]
                tc = -1.0 + (2.0 * j + (tl + 1.0)) / m
                mu = np.array([0.5 * (1.0 - tc), 0.5 * (1.0 + tc)])
                Nb = sb[s, :, q]
                S = uloc @ Nb                               # [Em][3]
                Sh = lam[:, :, edge, :] @ mu
                flux, dS, dSh = point_fluxes(oracle, side_types[:, s], roe, S, Sh, ff, geo["normals"][:, q], g)
                w = geo["wts"][:, q]
                # test functions of this point: interior (i, dof) and trace (i, edge, f)
                for i in range(3):
                    ridx = np.concatenate([gidx[i], ni + i * 8 + edge * 2 + np.arange(2)])
                    T = np.concatenate([Nb, mu])                                          # [6]
                    res[:, ridx] -= (flux[:, i] * w)[:, None] * T[None]
                    for k in range(3):
                        cidx = np.concatenate([gidx[k], ni + k * 8 + edge * 2 + np.arange(2)])
                        dcol = np.concatenate([alpha_u * dS[:, i, k, None] * Nb[None], dSh[:, i, k, None] * mu[None]], axis=1)  # [Em][6]
                        blocks[:, ridx[:, None], cidx[None, :]] += (w[:, None, None] * T[None, :, None]) * dcol[:, None, :]
    return res, blocks


def condense(res, blocks, ni, solve=None):
    """S = A_ll - A_lu A_uu^-1 A_ul, g = r_l - A_lu A_uu^-1 r_u, du = A_uu^-1 r_u (mha_batched_condense) with numpy.linalg.solve
    (or `solve`, e.g. gauss_jordan_solve)."""
    solve = solve or np.linalg.solve
    nt = blocks.shape[1] - ni
    X = solve(blocks[:, :ni, :ni], np.concatenate([blocks[:, :ni, ni:], res[:, :ni, None]], axis=2))
    S = blocks[:, ni:, ni:] - blocks[:, ni:, :ni] @ X[:, :, :nt]
    gv = res[:, ni:] - (blocks[:, ni:, :ni] @ X[:, :, nt:])[..., 0]
    return S, gv, X[:, :, nt]


def gauss_jordan_solve(A, B):
    """A plain Gauss-Jordan elimination with partial pivoting, batched over the first axis: the second reference solve the
    m = 3, 4 tolerance is measured with."""
    A, B = A.copy(), B.copy()
    E, n, _ = A.shape
    ar = np.arange(E)
    for k in range(n):
        piv = k + np.abs(A[:, k:, k]).argmax(axis=1)
        A[ar, k], A[ar, piv] = A[ar, piv].copy(), A[ar, k].copy()
        B[ar, k], B[ar, piv] = B[ar, piv].copy(), B[ar, k].copy()
        akk = A[:, k, k].copy()
        A[:, k] /= akk[:, None]
        B[:, k] /= akk[:, None]
        f = A[:, :, k].copy()
        f[:, k] = 0.0
        A -= f[:, :, None] * A[:, None, k, :]
        B -= f[:, :, None] * B[:, None, k, :]
    return B


def entry_err(a, ref):
    """The project's per-entry criterion (crs_err of tests/ns_thermal_ref.py, a block's rows in the role of CRS rows):
    per-entry relative error with a cancellation floor of a thousandth of the row's largest entry, beside the
    array-relative measure."""
    a, b = np.asarray(a), np.asarray(ref)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    rowmax = np.abs(b2).max(axis=1, keepdims=True)
    den = np.maximum(np.maximum(np.abs(b2), 1e-3 * rowmax), 1e-300)
    return max(float((np.abs(a2 - b2) / den).max()), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)))


def nonlinear_solver(oracle, sm, qdeg, u, lam, side_types, ff, max_iter, tol, g=9.81, roe=True, transient=None):
    """SubGridDtN_Solver::nonlinearSolver (subgridDtN_solver.cpp:909-1041) per macro element, the protocol of
    oracle_lib.subgrid_nonlinear_solver with norms and du over the n_int unknowns of a macro element -> (u, iters, scaled)."""
    u = np.array(u, dtype=np.float64)
    Em, ni = sm["nmacro"], sm["n_int"]
    rows = interior_rows(sm)
    iters, scaled, rn0 = np.zeros(Em, np.int32), np.full(Em, 10.0 * tol), np.zeros(Em)
    inloop = np.ones(Em, bool)
    for it in range(max_iter):
        if not inloop.any():
            break
        res, blk = assemble(oracle, sm, qdeg, u, lam, side_types, ff, g=g, roe=roe, transient=transient)
        nrm = np.abs(res[:, :ni]).max(axis=1)
        for e in np.flatnonzero(inloop):
            if it == 0:
                rn0[e] = nrm[e]
                scaled[e] = 1.0 if nrm[e] > 0.0 else 0.0
            else:
                scaled[e] = nrm[e] / rn0[e]
            if scaled[e] > tol:
                u[rows[e]] += np.linalg.solve(blk[e, :ni, :ni], res[e, :ni])
            iters[e] += 1
            inloop[e] = scaled[e] > tol
    return u, iters, scaled


def seeded_case(sm, seed, transient=False, dt=None):
    """Seeded states with the depth well above zero (H in [1, 2], as tests/test_full_size_gpu.py does), so that no interior
    block is near-singular -> u, lam [Em][24], side_types [Em][4], farfield, transient dict or None."""
    rng = np.random.default_rng(seed)
    Em, nd = sm["nmacro"], sm["ndof"]
    isH = (np.arange(nd) % 3) == 0                          # rows are (node, variable) interleaved
    u = rng.uniform(-1, 1, nd)
    u[isH] = rng.uniform(1.0, 2.0, isH.sum())
    lam = rng.uniform(-1, 1, (Em, 3, 4, 2))
    lam[:, 0] = rng.uniform(1.0, 2.0, (Em, 4, 2))
    st = rng.integers(0, 3, (Em, 4)).astype(np.uint8)
    tr = None
    if transient:
        A, b, bdf = np.array([[0.5, 0.0], [0.3, 0.7]]), np.array([0.4, 0.6]), np.array([1.5, -2.0, 0.5])
        tr = dict(u_prev=rng.uniform(-1, 1, (nd, 2)), u_stage=rng.uniform(-1, 1, (nd, 2)), stage=1, butcher_A=A, butcher_b=b,
                  bdf=bdf, dt=0.05 if dt is None else dt)
        for k in ("u_prev", "u_stage"):
            tr[k][isH] = rng.uniform(1.0, 2.0, (isH.sum(), 2))
    return u, lam.reshape(Em, 24), st, np.array([1.4, -0.3, 0.5]), tr


# ---- the seeded cases of the GPU comparison and the bound measured on them ----
G = 7.3
NCELL = (5, 3)        # 15 macro elements: an odd count, ragged under any grouping of macro elements per workgroup
# Condensed S, g, du at m = 3 and m = 4 (48 and 75 interior unknowns): per-entry criterion (entry_err, the crs_err measure)
# with a bound of 10 x the largest per-entry difference between two REFERENCE solves of the restatement -- numpy.linalg.solve
# and a plain numpy Gauss-Jordan with partial pivoting -- on the GPU tests' own seeded inputs (reference_spread below, run on
# the CPU over the four (steady | transient) x (Roe | max-EV) cases of each m; profiles/swhdg_subgrids.md):
#   m = 3: measured 1.221e-11 -> bound 1.221e-10      m = 4: measured 9.776e-12 -> bound 9.776e-11
# (m = 2, for the record: 5.2e-12 by the same measure; its bound stays the one-element test's.)
# The 10 x covers the different elimination order and the matrix-core summation order.
# tests/test_swhdg_subgrids.py re-measures the spread and holds it against these constants.
SPREAD_MEASURED = {3: 1.221e-11, 4: 9.776e-12}
TOL_CONDENSED = {m: 10.0 * v for m, v in SPREAD_MEASURED.items()}


def case(m, transient, seed_shift=0, ncell=NCELL):
    """The seeded inputs of the m-case: warped macro mesh, mixed interface / far-field / slip macro sides, depth in [1, 2]."""
    sm = subgrid_mesh(ncell, m, warp=macro_warp)
    u, lam, st, ff, tr = seeded_case(sm, 100 + 10 * m + seed_shift, transient)
    return sm, u, lam, st, ff, tr


def reference_spread(oracle, m):
    """Largest per-entry difference (entry_err) between the two reference solves over the four cases of m."""
    worst = 0.0
    for transient in (False, True):
        for roe in (True, False):
            sm, u, lam, st, ff, tr = case(m, transient)
            res, blk = assemble(oracle, sm, 2, u, lam, st, ff, g=G, roe=roe, transient=tr)
            a = condense(res, blk, sm["n_int"])
            b = condense(res, blk, sm["n_int"], solve=gauss_jordan_solve)
            worst = max([worst] + [entry_err(x, y) for x, y in zip(b, a)])
    return worst
