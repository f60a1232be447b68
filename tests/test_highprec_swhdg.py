"""The shallowwaterHybridized yardstick (tests/highprec_swhdg_ref.py) against its own invariants, against mpmath alone and
against the reference's unit-test values; its guards (branch, regime, conditioning) on every case that
tests/test_highprec_swhdg_gpu.py runs on the device; and the CPU oracle against it entry by entry, which measures K_oracle
per input family -- one constant for the uncondensed arrays, one for the boundary groups, two for the condensed S, g, du --
and holds it to the constant
recorded in highprec_swhdg_ref.K_ORACLE from both sides."""
import os
import sys

import mpmath
import numpy as np
import pytest

import highprec_ref as H
import highprec_swhdg_ref as SW
import swhdg_subgrid_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import swhdg_unit_values as V  # noqa: E402

LD = np.longdouble
G = SW.GRAVITY
MS = (1, 2, 3, 4)


def all_cases(family, ms=MS):
    for m in ms:
        for roe in (True, False):
            for transient in (False, True):
                yield SW.build_case(family, m, roe, transient), "m=%d %s %s" % (m, "Roe" if roe else "maxEV", "stage 1" if transient else "steady")


# ---- plain mpmath restatements (scalars, no shared code with the yardstick) -----------------------------------------------------
def mp_flux_n(Sh, n, g):
    Hh, a, b = Sh
    p = g * Hh * Hh / 2
    return [a * n[0] + b * n[1], (a * a / Hh + p) * n[0] + a * b / Hh * n[1], a * b / Hh * n[0] + (b * b / Hh + p) * n[1]]


def mp_eig(Sh, n, g):
    mp = mpmath
    Hh, ux, uy = Sh[0], Sh[1] / Sh[0], Sh[2] / Sh[0]
    vn, a = ux * n[0] + uy * n[1], mp.sqrt(g * Hh)
    Rm = mp.matrix([[1, 0, 1], [ux + a * n[0], -a * n[1], ux - a * n[0]], [uy + a * n[1], a * n[0], uy - a * n[1]]])
    Lm = mp.matrix([[(a - vn) / (2 * a), n[0] / (2 * a), n[1] / (2 * a)], [(ux * n[1] - uy * n[0]) / a, -n[1] / a, n[0] / a],
                    [(a + vn) / (2 * a), -n[0] / (2 * a), -n[1] / (2 * a)]])
    return Lm, [vn + a, vn, vn - a], Rm


def mp_interface_flux(stype, roe, S, Sh, Sinf, n, g):
    """The flux of one point; complex arguments decide abs and max on the real part, ties as the device does."""
    mp = mpmath
    ab = lambda z: -z if mp.re(z) < 0 else z
    S, Sh = mp.matrix(S), mp.matrix(Sh)
    if stype == 2:
        vn = (S[1] * n[0] + S[2] * n[1]) / S[0]
        return [S[0] - Sh[0], S[1] / S[0] - vn * n[0] - Sh[1] / Sh[0], S[2] / S[0] - vn * n[1] - Sh[2] / Sh[0]]
    Lm, lam, Rm = mp_eig(Sh, n, g)
    if stype == 1:
        Ap = Rm * mp.diag([(l + ab(l)) / 2 for l in lam]) * Lm
        Am = Rm * mp.diag([(l - ab(l)) / 2 for l in lam]) * Lm
        out = Ap * (S - Sh) - Am * (mp.matrix(Sinf) - Sh)
        return [out[i] for i in range(3)]
    if roe:
        st = Rm * mp.diag([ab(l) for l in lam]) * Lm * (S - Sh)
    else:
        p, q = ab(lam[0]), ab(lam[2])
        st = (p if mp.re(p) > mp.re(q) else q) * (S - Sh)
    F = mp_flux_n(Sh, n, g)
    return [F[i] + st[i] for i in range(3)]


def ld_to_mp(x):
    """An 80-bit number as an mpf, exactly (hi + lo split into two doubles)."""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(x) - LD(hi)))


# ---- the yardstick's own checks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", SW.FAMILIES)
def test_eigendecomposition_identities(family):
    """L R = I and R Lambda L = d(F . n)/dShat, the latter against mpmath.diff at 50 digits, on one point of the family."""
    c = SW.build_case(family, 1, True, False)
    _, _, geo, S, Sh, _ = c["sd"]["pts"][1]
    S, Sh, n, ff = S.reshape(-1, 3), Sh.reshape(-1, 3), geo["n"].reshape(-1, 2), c["ff"]   # n in longdouble: a unit vector to 2^-64
    p = len(Sh) // 2
    pe = SW.side_point_eval(0, True, G, S[p:p + 1], Sh[p:p + 1], n[p:p + 1], ff)
    Lm, lam, Rm = pe["L"][0][0], pe["lam"][0][0], pe["R"][0][0]
    I = Lm @ Rm
    sI = pe["L"][1][0] @ pe["R"][1][0]
    assert np.all(np.abs(I - np.eye(3)) <= 8 * 2.0 ** -64 * sI), np.abs(I - np.eye(3)).max()
    A = Rm @ np.diag(lam) @ Lm
    sA = pe["R"][1][0] @ np.diag(pe["lam"][1][0]) @ pe["L"][1][0]
    with mpmath.workdps(50):
        shm, nm = [ld_to_mp(v) for v in Sh[p]], [ld_to_mp(v) for v in n[p]]
        for i in range(3):
            for j in range(3):
                f = lambda x, i=i, j=j: mp_flux_n([x if k == j else shm[k] for k in range(3)], nm, mpmath.mpf(G))[i]
                ref = mpmath.diff(f, shm[j])
                assert abs(ld_to_mp(A[i, j]) - ref) <= 16 * mpmath.mpf(2) ** -64 * ld_to_mp(sA[i, j]), (i, j)


def test_unit_test_values_are_reproduced():
    """tests/golden/swhdg_unit_values.py (the reference's own unit test; its values carry 15-17 digits)."""
    tol = lambda ref: 1e-14 * np.abs(np.asarray(ref)).max()
    pe = SW.side_point_eval(0, True, V.G, [V.EV2D["Shat"]], [V.EV2D["Shat"]], [V.EV2D["n"]], [0, 0, 0])
    for k in ("L", "lam", "R"):
        assert np.abs(pe[k][0][0] - np.array(V.EV2D[k])).max() <= tol(V.EV2D[k]), k
    s = V.STAB
    for roe, k in ((True, "roe"), (False, "maxEV")):
        pe = SW.side_point_eval(0, roe, V.G, [s["S"]], [s["Shat"]], [s["n"]], [0, 0, 0])
        assert np.abs(pe["term"][0][0] - np.array(s[k])).max() <= tol(s[k]), k
    f = V.FLUX
    for st, fx, fy in ((f["Shat"], "Fx_hat", "Fy_hat"), (f["S"], "Fx", "Fy")):
        pe = SW.side_point_eval(0, True, V.G, [f["S"]], [st], [[1.0, 0.0]], [0, 0, 0])
        assert np.abs(pe["fluxvec"][0][0][:, 0] - np.array(f[fx])).max() <= tol(f[fx])
        assert np.abs(pe["fluxvec"][0][0][:, 1] - np.array(f[fy])).max() <= tol(f[fy])
    b = V.BOUND
    pe = SW.side_point_eval(1, True, V.G, [b["S"]], [b["Shat"]], [b["n"]], b["Sinf"])
    assert np.abs(pe["term"][0][0] - np.array(b["farfield"])).max() <= tol(b["farfield"])
    assert np.array_equal(pe["term"][0], pe["iflux"][0])


@pytest.mark.parametrize("m", MS)
def test_constant_state_gives_zero_residual(m):
    """Constant interior state, equal trace, interface sides, no source, steady: the element residual vanishes (divergence
    theorem) to 1e-17 of each entry's scale; the volume term alone does not."""
    sm = R.subgrid_mesh(SW.NCELL[m], m, warp=SW.macro_vertices("unit"))
    sm.update(orders=np.array([1, 1, 1], np.int32), varptr=np.array([0, 4, 8, 12], np.int32))
    Em, ni = sm["nmacro"], sm["n_int"]
    const = np.array([1.7, 0.4, -0.3])
    rows = R.interior_rows(sm)
    u = np.zeros(sm["ndof"])
    u[rows] = np.repeat(const, (m + 1) ** 2)[None]
    for roe in (True, False):
        blk = H.Block(sm, SW.QDEG)
        el = H.element_arrays(blk, SW.MODULE, {"g": G, "source H": 0.0, "source Hux": 0.0, "source Huy": 0.0}, u)
        sd = SW.side_blocks(sm["nodes"], m, SW.QDEG, u[rows], 1.0, np.tile(np.repeat(const, 8), (Em, 1)), np.zeros((Em, 4), np.uint8),
                            const, G, roe)
        res, S = sd["res"].copy(), sd["S_res"].copy()
        off = np.asarray(sm["offsets"])
        vol = np.zeros((Em, ni), LD)
        for ey in range(m):
            for ex in range(m):
                gi = SW.interior_index(m, ex, ey).ravel()
                e = np.arange(Em) * m * m + ey * m + ex
                vol[:, gi] += el["local_res"][e][:, off]
                S[:, gi] += el["S_res"][e][:, off]
        res[:, :ni] += vol
        # the trace rows of an edge hold the flux of ONE side; the opposite element cancels it, not this one
        assert np.abs(vol).max() > 1e-3
        assert np.all(np.abs(res[:, :ni]) <= 1e-17 * S[:, :ni]), float((np.abs(res[:, :ni]) / S[:, :ni]).max())


def test_side_points_are_where_the_mesh_puts_them(oracle):
    """Points, weights and normals of every side of every sub-element against the mesh's sides (oracle_lib's
    physical_side_basis, the order of per-point boundary data), and the normals point out of the element."""
    for fam in ("unit", "stretched sheared"):
        sm = R.subgrid_mesh(SW.NCELL[2], 2, warp=SW.macro_vertices(fam))
        E = sm["nelem"]
        centre = sm["nodes"].mean(axis=1)
        size = np.abs(sm["nodes"]).max()
        for s in range(4):
            geo = SW.side_geometry(sm["nodes"], SW.QDEG, s)
            got = oracle.physical_side_basis(2, 1, SW.QDEG, sm["nodes"], np.arange(E, dtype=np.int32), np.full(E, s, np.int32))
            assert np.abs(geo["x"] - got["ip"]).max() < 1e-13 * size and np.abs(geo["w"] - got["wts"]).max() < 1e-13 * float(geo["w"].max())
            assert np.abs(geo["n"] - got["normals"]).max() < 1e-12 * (1e3 if fam == "stretched sheared" else 1)
            assert np.all((geo["n"] * (geo["x"] - centre[:, None, :])).sum(axis=2) > 0), (fam, s)
            assert np.abs((geo["n"] ** 2).sum(axis=2) - 1).max() < 1e-18


def test_one_warped_element_against_mpmath():
    """The side block of ONE warped element with one interface (Roe-like), one far-field, one slip and one max-EV-free
    side at 50 digits: plain loops, the derivative by a complex step in mpmath, to 1e-17 of each entry's scale."""
    mp = mpmath
    nodes = SW.macro_vertices("unit")(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])) * np.array([1.0, 0.6])
    rng = np.random.default_rng(5)
    ue, lam = rng.uniform(-1, 1, 12), rng.uniform(-1, 1, 24)
    ue[:4], lam[:8] = rng.uniform(1, 2, 4), rng.uniform(1, 2, 8)
    st, ff = np.array([[0, 1, 2, 1]], np.uint8), np.array([1.4, -0.3, 0.5])
    for roe in (True, False):
        sd = SW.side_blocks(nodes[None], 1, SW.QDEG, ue[None], 0.8, lam[None], st, ff, G, roe)
        with mp.workdps(50):
            h = mp.mpf(10) ** -40
            xs, ws = H.gauss_mp.__wrapped__(H.gauss_npts(SW.QDEG))
            X = [[mp.mpf(float(c)) for c in v] for v in nodes]
            sgn = [(-1, -1), (1, -1), (1, 1), (-1, 1)]                      # reference vertices, counter-clockwise
            side = [((0, -1), (1, 0)), ((1, 0), (0, 1)), ((0, 1), (-1, 0)), ((-1, 0), (0, -1))]   # centre, tangent
            unk = [mp.mpf(float(v)) for v in np.concatenate([ue, lam])]

            def residual(z):
                out = [mp.mpc(0)] * 36
                for s in range(4):
                    (cx, cy), (tx, ty) = side[s]
                    edge = SW.HFACE_EDGE[s]
                    for q in reversed(range(len(xs))):
                        xi, eta = cx + xs[q] * tx, cy + xs[q] * ty
                        dxs = [sum(X[v][d] * sgn[v][0] * (1 + sgn[v][1] * eta) / 4 for v in range(4)) * tx +
                               sum(X[v][d] * sgn[v][1] * (1 + sgn[v][0] * xi) / 4 for v in range(4)) * ty for d in range(2)]
                        ln = mp.sqrt(dxs[0] ** 2 + dxs[1] ** 2)
                        n = [dxs[1] / ln, -dxs[0] / ln]                        # the tangent turned clockwise: outward
                        phi = [(1 + a * xi) * (1 + b * eta) / 4 for b in (-1, 1) for a in (-1, 1)]
                        t = eta if edge in (0, 2) else xi
                        mu = [(1 - t) / 2, (1 + t) / 2]
                        S = [sum(phi[f] * z[4 * v + f] for f in range(4)) for v in range(3)]
                        Sh = [sum(mu[k] * z[12 + 8 * v + 2 * edge + k] for k in range(2)) for v in range(3)]
                        fl = mp_interface_flux(int(st[0, s]), roe, S, Sh, [mp.mpf(float(v)) for v in ff], n, mp.mpf(G))
                        for i in range(3):
                            for f in range(4):
                                out[4 * i + f] += fl[i] * ws[q] * ln * phi[f]
                            for k in range(2):
                                out[12 + 8 * i + 2 * edge + k] += fl[i] * ws[q] * ln * mu[k]
                return out
            r0 = residual(unk)
            for r in range(36):
                assert abs(ld_to_mp(sd["res"][0, r]) + mp.re(r0[r])) <= mp.mpf(10) ** -17 * ld_to_mp(sd["S_res"][0, r]), ("res", r)
            for c in range(36):
                z = list(unk)
                z[c] = mp.mpc(z[c], h)
                col = residual(z)
                scale = mp.mpf(0.8) if c < 12 else 1                # alpha_u (the double 0.8) on the interior columns
                for r in range(36):
                    ref = mp.im(col[r]) / h * scale
                    assert abs(ld_to_mp(sd["blocks"][0, r, c]) - ref) <= mp.mpf(10) ** -17 * ld_to_mp(sd["S_blocks"][0, r, c]), (r, c)
                    if sd["S_blocks"][0, r, c] == 0:
                        assert sd["blocks"][0, r, c] == 0 and ref == 0


# ---- the guards ------------------------------------------------------------------------------------------------------------------
# The steady subgrid cases whose cond_2(A_uu) exceeds 1e7 (profiles/extended_precision_yardstick.md): their condensed
# outputs are not compared, on the CPU or on the device.  Pinned, so that a change of inputs cannot drop more unnoticed.
UNCONDENSED_ONLY = {
    "shallow": ["m=3 Roe steady", "m=4 Roe steady"],
    "metric": ["m=3 Roe steady", "m=3 maxEV steady"],
    "rest": ["m=2 Roe steady", "m=3 Roe steady", "m=3 maxEV steady", "m=4 Roe steady", "m=4 maxEV steady"],
    "rest consistent": ["m=2 Roe steady", "m=3 Roe steady", "m=3 maxEV steady", "m=4 Roe steady", "m=4 maxEV steady"],
    "stretched sheared": ["m=3 Roe steady"],
}


@pytest.mark.parametrize("family", SW.FAMILIES)
def test_guards(family):
    """Branch, regime and conditioning guards on every case, and on the boundary groups' per-point trace states."""
    worst, skipped = 0.0, []
    for c, tag in all_cases(family):
        k = SW.check_guards(c)
        if c["cd"] is None:
            skipped.append(tag)
            print("    %-18s %s: cond_2(A_uu) = %.2g, compared uncondensed only" % (family, tag, k))
        else:
            worst = max(worst, k)
    print("%-18s largest cond_2(A_uu) among the condensed comparisons %.3g" % (family, worst))
    # the steady subgrid cases that the conditioning guard takes out of the condensed comparison are these and no others
    assert skipped == UNCONDENSED_ONLY.get(family, []), skipped
    for m in SW.BOUNDARY_MS:                                        # the groups' per-point trace states, every m that builds them
        c = SW.build_case(family, m, True, False)
        assert SW.boundary_guard(c, SW.boundary_groups(c)), ("branch guard of the boundary groups", family, m)
    c = SW.build_case(family, 1, True, False)
    if family == "supercritical":
        # the exact zeros: on a far-field side with every lambda < 0 the flux is -A- (Sinf - Shat), which does not depend on
        # the interior state: the trace rows of that edge have S == 0 (and 0) in every interior column; with every lambda > 0
        # A- = 0 and A+ = A: nothing of Sinf is left, and the yardstick's own zero weights say so
        ni, hit = c["n_int"], 0
        for s_, j, geo, S, Sh, pe in c["sd"]["pts"]:
            lam, _ = SW.eigenvalues(Sh, geo["n"], G)
            for e in np.flatnonzero((c["st"][:, s_] == SW.FARFIELD) & np.all(lam < 0, axis=(1, 2))):
                rows = ni + 8 * np.arange(3)[:, None] + 2 * SW.HFACE_EDGE[s_] + np.arange(2)[None]
                assert np.all(c["sd"]["S_blocks"][e][rows.ravel(), :ni] == 0) and np.all(c["sd"]["blocks"][e][rows.ravel(), :ni] == 0)
                assert np.all(pe["d_dS"][1][e] == 0) and np.all(pe["d_dS"][0][e] == 0)
                hit += 1
        assert hit > 0


# ---- the oracle against the yardstick ---------------------------------------------------------------------------------------------
def oracle_mesh(oracle, c):
    return R.oracle_mesh(oracle, c["m"])


def oracle_funcs(c):
    return {k: c["P"][k] for k in ("source H", "source Hux", "source Huy")}


def oracle_system(oracle, c):
    """The oracle's uncondensed system of the case: orc_swh_hdg_element + the volume blocks (m = 1), the numpy restatement
    of tests/swhdg_subgrid_ref.py on the oracle's point functions and volume blocks (m >= 2)."""
    sm, m, ni = c["m"], c["mm"], c["n_int"]
    om = oracle_mesh(oracle, c)
    if m > 1:
        return R.assemble(oracle, sm, c["qdeg"], c["u"], c["lam"], c["st"], c["ff"], g=G, roe=c["roe"], transient=c["tr"],
                          funcs=oracle_funcs(c))
    res, blk = oracle.swh_hdg_element(om, c["qdeg"], c["u"], c["lam"], c["st"], c["ff"], g=G, roe=c["roe"], transient=c["tr"])
    vol = oracle.assemble_block(om, oracle.PHYS_SHALLOWWATER_HYBRIDIZED, c["qdeg"], c["u"], params=[G], transient=c["tr"],
                                want_local=True, funcs=oracle_funcs(c))
    off = sm["offsets"]
    blk[:, :ni, :ni] += vol["local_J"][:, off][:, :, off]
    res[:, :ni] += vol["local_res"][:, off]
    return res, blk


def point_distances(oracle, family):
    """orc_swh_* at the family's side points, every side type and both stabilisations, against the yardstick's values."""
    S, Sh, n, ff = SW.point_inputs(family)
    d = {}
    for stype in (0, 1, 2):
        for roe in ((True, False) if stype == 0 else (True,)):
            pe = SW.side_point_eval(stype, roe, G, S, Sh, n, ff)
            got = dict(iflux=np.array([oracle.swh_interface_flux(2, stype, roe, S[p], Sh[p], ff, n[p], G) for p in range(len(S))]),
                       fluxvec=np.array([oracle.swh_flux_vector(2, Sh[p], G) for p in range(len(S))]),
                       term=np.array([oracle.swh_stab_term(2, S[p], Sh[p], n[p], G, roe) if stype == 0 else
                                      oracle.swh_boundary_term(2, stype, S[p], Sh[p], ff, n[p], G) for p in range(len(S))]))
            eig = [oracle.swh_eigendecomp(2, Sh[p], n[p], G) for p in range(len(S))]
            got.update(L=np.array([e[0] for e in eig]), lam=np.array([e[1] for e in eig]), R=np.array([e[2] for e in eig]))
            for k, v in got.items():
                d["point %s type %d %s" % (k, stype, "Roe" if roe else "maxEV")] = H.distance(v, pe[k][0], pe[k][1])
    return d


def measure(oracle, family):
    """-> five dicts of figures: the C oracle's uncondensed arrays, its boundary-group assembly, the numpy restatement's
    uncondensed subgrid blocks (m >= 2; for the record and held to the device's bound, not part of a constant), and the
    condensed S, g, du of numpy.linalg.solve on the oracle's blocks by the two scales of highprec_swhdg_ref.condensed."""
    fig, bnd, sub, cond, cw = dict(point_distances(oracle, family)), {}, {}, {}, {}
    for c, tag in all_cases(family):
        res, blk = oracle_system(oracle, c)
        into = fig if c["mm"] == 1 else sub
        into[tag + " res"] = H.distance(res, c["res"], c["S_res"])
        into[tag + " blocks"] = H.distance(blk, c["blocks"], c["S_blocks"])
        vol = oracle.assemble_block(oracle_mesh(oracle, c), oracle.PHYS_SHALLOWWATER_HYBRIDIZED, c["qdeg"], c["u"], params=[G],
                                    transient=c["tr"], want_local=True, funcs=oracle_funcs(c), rowptr=c["g"]["rowptr"],
                                    colind=c["g"]["colind"])
        el, g = c["el"], c["g"]
        fig[tag + " volume local_J"] = H.distance(vol["local_J"], el["local_J"], el["S_J"])
        fig[tag + " volume local_res"] = H.distance(vol["local_res"], el["local_res"], el["S_res"])
        fig[tag + " volume crs_vals"] = H.distance(vol["crs_vals"], g["crs_vals"], g["S_vals"])
        fig[tag + " volume res"] = H.distance(vol["res"], g["res"], g["S_res"])
        if c["mm"] in SW.BOUNDARY_MS:                               # the boundary-group assembly
            groups = SW.boundary_groups(c)
            b = SW.boundary_arrays(c, groups)
            vals, rg = np.zeros(len(g["colind"])), np.zeros(c["m"]["ndof"])
            for name, bc, be, bs, aux, ffp in groups:
                oracle.assemble_block_boundary(oracle_mesh(oracle, c), oracle.PHYS_SHALLOWWATER_HYBRIDIZED, c["qdeg"], c["u"], be, bs,
                                               bc, 0.0, rowptr=g["rowptr"], colind=g["colind"], crs_vals=vals, res=rg,
                                               params=[G, 1 if c["roe"] else 0], aux=aux, farfield=ffp, transient=c["tr"])
            bnd[tag + " boundary res"] = H.distance(rg, b["res"], b["S_res"])
            bnd[tag + " boundary vals"] = H.distance(vals, b["crs_vals"], b["S_vals"])
        if c["cd"] is not None:                                     # numpy.linalg.solve on the oracle's blocks
            ni, cd = c["n_int"], c["cd"]
            S, gv, du = R.condense(res, blk, ni)
            for name, got in (("schur", S), ("gvec", gv), ("du", du)):
                cond["%s %s" % (tag, name)] = H.distance(got, cd[name], cd["S_" + name])
                cw["%s %s (componentwise)" % (tag, name)] = H.distance(got, cd[name], cd["C_" + name])
    return fig, bnd, sub, cond, cw


@pytest.mark.parametrize("family", SW.FAMILIES)
def test_oracle_against_the_yardstick(oracle, family):
    """K_oracle per (array group, family), two-sided.  The uncondensed arrays and the boundary groups come from the C
    oracle alone (plain loops, -ffp-contract=off: the same figure on every run): the next integer at least one half above
    the measurement, above 1000 the next multiple of ten.  The condensed group goes through numpy.linalg.solve and matmul,
    whose summation order follows the vector units of the CPU: highprec_ref's rule for such measurements, the measurement
    times 1.25 rounded up to two digits, failing below two thirds of the constant."""
    fig, bnd, sub, cond, cw = measure(oracle, family)
    for k, v in [kv for d in (fig, bnd, sub, cond, cw) for kv in d.items()]:
        print("    %-18s %-46s d = %.4g" % (family, k, v))
    for module, d, exact in ((SW.MODULE, fig, True), (SW.BOUNDARY, bnd, True), (SW.CONDENSED, cond, False), (SW.CONDENSED_CW, cw, False)):
        k = max(d.values())
        rec = H.K_ORACLE.get((module, family))
        print("K_oracle[%s, %s] = %.5g (recorded %s, device bound %s)" %
              (module, family, k, rec, H.device_bound(module, family) if rec is not None else None))
        assert rec is not None, "no recorded K_oracle"
        assert k <= rec, "the oracle is farther from the yardstick than recorded"
        if exact:
            assert rec <= 1.5 * k + 1.0, "the recorded K_oracle is stale (more than half above the measurement)"
        else:
            assert k >= rec * 2.0 / 3.0, "the recorded K_oracle is stale (the measurement is below two thirds of it)"
    ks = max(sub.values())
    print("%-18s numpy restatement of the subgrid blocks (m >= 2): largest d = %.4g, held to the device's bound %.4g" %
          (family, ks, H.device_bound(SW.MODULE, family)))
    assert ks <= H.device_bound(SW.MODULE, family)


# ---- the tie convention --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", SW.REST)
def test_tie_convention_at_rest(oracle, family):
    """At rest lam1 = vn is exactly 0 in any precision and |vn + a| == |vn - a|: the yardstick under the device's convention
    (abs(0) -> +, max of equals -> the second) agrees with the oracle within K_oracle; the figure printed is how far the
    blocks move when a tie is taken the other way (the reference's AD library, which decides it there, is not available)."""
    for roe in (True, False):
        c = SW.build_case(family, 1, roe, False)
        res, blk = oracle.swh_hdg_element(oracle_mesh(oracle, c), c["qdeg"], c["u"], c["lam"], c["st"], c["ff"], g=G, roe=roe)
        sd = c["sd"]
        d = max(H.distance(res, sd["res"], sd["S_res"]), H.distance(blk, sd["blocks"], sd["S_blocks"]))
        assert d <= H.K_ORACLE[(SW.MODULE, family)], d
        us = c["blk"].seeded(c["u"], None)[0][c["rows"]]
        for tie, what in (((False, True), "abs(0) taken as -"), ((True, False), "max of equals takes the first")):
            o = SW.side_blocks(c["m"]["nodes"], 1, c["qdeg"], us, 1.0, c["lam"], c["st"], c["ff"], G, roe, tie=tie)
            pos = sd["S_blocks"] > 0
            move = float((np.abs(o["blocks"] - sd["blocks"])[pos] / sd["S_blocks"][pos]).max())
            mr = float(np.abs(o["res"] - sd["res"]).max())
            print("%-16s %-6s %-30s blocks move by at most %.3g of their scale, the residual by %.3g" %
                  (family, "Roe" if roe else "maxEV", what, move, mr))
            assert mr == 0.0                                         # the values do not depend on the tie, the derivatives may
