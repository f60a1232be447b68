"""shallowwaterHybridized on the device (through the C ABI) against the extended-precision yardstick of
tests/highprec_swhdg_ref.py, entry by entry: d = |device - yardstick| / (2^-53 S) with S the scale of the entry's own sum,
exact zeros where S == 0, a value that is not finite counts as infinite.  The bound per (array group, input family) is
max(8 K_oracle, 8) with K_oracle the CPU oracle's own d on the same inputs (highprec_swhdg_ref.K_ORACLE, re-measured by
tests/test_highprec_swhdg.py): one constant for the uncondensed arrays, one for the boundary groups, and for the condensed
S, g, du one per scale (the sum as formed, whose constant carries the conditioning, and the componentwise bound, whose
scale does).  It is never taken from the device.  Every test prints its largest d beside its bound.  The families: unit,
near-critical, supercritical, shallow, metric, rest, rest consistent, stretched sheared; both stabilisations, all three
side types, steady and stage 1 of the two-stage tableau; m = 1..4 sub-elements per macro element."""
import numpy as np
import pytest

import highprec_ref as H
import highprec_swhdg_ref as SW
from test_highprec_gpu import Worst

pytestmark = pytest.mark.gpu
G = SW.GRAVITY


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def dev(a, dtype=np.float64):
    return _torch().tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def full(shape, value=7.0, dtype=None):
    torch = _torch()
    return torch.full(shape, value, dtype=dtype or torch.float64, device="cuda")


def cases(family, ms, transients=(False, True), roes=(True, False)):
    for m in ms:
        for roe in roes:
            for transient in transients:
                yield SW.build_case(family, m, roe, transient), "m=%d %s %s" % (m, "Roe" if roe else "maxEV", "stage 1" if transient else "steady")


def make_block(c, layout=False, graph=False):
    import mrhyde_amd
    sm = c["m"]
    blk = mrhyde_amd.Block(2, quadrature=c["qdeg"], physics="shallowwaterHybridized", variables=[(0, 1)] * 3)
    blk.set_mesh(sm["nodes"], sm["lids"], sm["offsets"], sm["ndof"])
    if graph:
        blk.set_graph(c["g"]["rowptr"], c["g"]["colind"])
    else:
        blk.set_graph()
    blk.set_physics_parameter("g", G)
    blk.set_physics_parameter("Roe-like stabilization", 1 if c["roe"] else 0)
    for k in ("source H", "source Hux", "source Huy"):
        blk.set_function(k, c["P"][k])
    kw = {}
    tr = c["tr"]
    if tr is not None:
        blk.set_time_integration(True, 2, 2, tr["stage"], tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
        kw = dict(u_prev=dev(tr["u_prev"]), u_stage=dev(tr["u_stage"]))
    if layout:
        blk.set_swhdg_subgrids(c["mm"])
    return blk, kw


def side_kw(c):
    return dict(side_types=dev(c["st"], np.uint8), farfield=c["ff"])


class Both:
    """The condensed outputs by both scales of highprec_swhdg_ref.condensed, each with its own K_oracle."""

    def __init__(self, family):
        self.w, self.cw = Worst(SW.CONDENSED, family), Worst(SW.CONDENSED_CW, family)

    def finish(self):
        try:
            self.w.finish()
        finally:
            self.cw.finish()


def check_condensed(b, c, tag, S, g, du):
    cd = c["cd"]
    for name, got in (("schur", S), ("gvec", g), ("du", du)):
        b.w.add("%s %s" % (tag, name), H.distance(got.cpu().numpy(), cd[name], cd["S_" + name]))
        b.cw.add("%s %s (componentwise scale)" % (tag, name), H.distance(got.cpu().numpy(), cd[name], cd["C_" + name]))


# ---- the point functions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", SW.FAMILIES)
def test_point_functions(family):
    """mha_swhdg_side_terms and mha_swhdg_eigendecomp at the side points of the family: every side type, both
    stabilisations, values and both derivatives, per entry."""
    import mrhyde_amd
    w = Worst(SW.MODULE, family)
    S, Sh, n, ff = SW.point_inputs(family)
    Sinf = np.tile(ff, (len(S), 1))
    L, lam, R = mrhyde_amd.swhdg_eigendecomp(G, dev(Sh), dev(n))
    _torch().cuda.synchronize()
    eig = dict(L=L, lam=lam, R=R)
    for stype in (0, 1, 2):
        for roe in ((True, False) if stype == 0 else (True,)):
            pe = SW.side_point_eval(stype, roe, G, S, Sh, n, ff)
            out = mrhyde_amd.swhdg_side_terms(stype, roe, G, dev(S), dev(Sh), dev(n), dev(Sinf))
            _torch().cuda.synchronize()
            tag = "type %d %s" % (stype, "Roe" if roe else "maxEV")
            for k in ("fluxvec", "term", "iflux", "d_dS", "d_dShat"):
                w.add("%s %s" % (tag, k), H.distance(out[k].cpu().numpy(), pe[k][0], pe[k][1]))
            if stype == 0 and roe:
                for k in ("L", "lam", "R"):
                    w.add("eigendecomp %s" % k, H.distance(eig[k].cpu().numpy(), pe[k][0], pe[k][1]))
            if family == "supercritical" and stype == 1:
                # the exact zeros: A+ = 0 where every lambda < 0 (no dependence on S), and they were compared above as S == 0
                neg = np.all(pe["lam"][0] < 0, axis=1)
                assert neg.any() and np.all(pe["d_dS"][1][neg] == 0) and np.all(out["d_dS"].cpu().numpy()[neg] == 0.0)
    w.finish()


# ---- the volume term: assembly paths and matrix-free products -------------------------------------------------------------------------
@pytest.mark.parametrize("family", SW.FAMILIES)
def test_volume_paths_and_products(family):
    """assemble_jacres of the module on every path it has (the kernel that ran asserted), compute_local_jacres, and the
    matrix-free products by S_y: one-element meshes and 2 x 2 sub-meshes (shared interior rows), steady and stage 1."""
    import mrhyde_amd as M
    torch = _torch()
    w = Worst(SW.MODULE, family)
    for c, tag in cases(family, (1, 2), roes=(True,)):
        blk, kw = make_block(c, graph=True)
        g, el, nd = c["g"], c["el"], c["m"]["ndof"]
        ud = dev(c["u"])
        for name, path, last in (("AUTO", M.PATH_AUTO, M.PATH_ROW_GATHER), ("POINT_ENGINE", M.PATH_POINT_ENGINE, M.PATH_POINT_ENGINE),
                                 ("ROW_GATHER", M.PATH_ROW_GATHER, M.PATH_ROW_GATHER),
                                 ("LOCAL_THEN_SCATTER", M.PATH_LOCAL_THEN_SCATTER, M.PATH_LOCAL_THEN_SCATTER)):
            res, vals = full((nd,)), full((len(g["colind"]),), -3.0)
            blk.assemble_jacres(ud, res, vals, path=path, overwrite=True, **kw)
            torch.cuda.synchronize()
            assert blk.info("last_path") == last, (tag, name, blk.info("last_path"))
            w.add("%s %s crs_vals" % (tag, name), H.distance(vals.cpu().numpy(), g["crs_vals"], g["S_vals"]))
            w.add("%s %s res" % (tag, name), H.distance(res.cpu().numpy(), g["res"], g["S_res"]))
        E = c["m"]["nelem"]
        lJ, lr = full((E, 12, 12), 0.0), full((E, 12), 0.0)
        blk.compute_local_jacres(ud, lJ, lr, **kw)
        torch.cuda.synchronize()
        w.add(tag + " local_J", H.distance(lJ.cpu().numpy(), el["local_J"], el["S_J"]))
        w.add(tag + " local_res", H.distance(lr.cpu().numpy(), el["local_res"], el["S_res"]))
        rng = np.random.default_rng(211)
        X = rng.uniform(0.5, 1.0, (3, nd)) * rng.choice([-1.0, 1.0], (3, nd))
        for transpose in (False, True):
            Y, SY = H.matvec(g, X, transpose)
            y, Ym = full((nd,), 3.25), full((3, nd), 3.25)
            blk.apply_jacobian(ud, dev(X[0]), y, transpose=transpose, overwrite=True, **kw)
            blk.apply_jacobian_multi(ud, dev(X), Ym, transpose=transpose, overwrite=True, **kw)
            torch.cuda.synchronize()
            t = "transposed" if transpose else "forward"
            w.add("%s apply_jacobian %s" % (tag, t), H.distance(y.cpu().numpy(), Y[0], SY[0]))
            w.add("%s apply_jacobian_multi K = 3 %s" % (tag, t), H.distance(Ym.cpu().numpy(), Y, SY))
        d = full((nd,), 3.25)
        blk.jacobian_diagonal(ud, d, overwrite=True, **kw)
        torch.cuda.synchronize()
        dref, sref = H.diagonal(g)
        w.add(tag + " jacobian_diagonal", H.distance(d.cpu().numpy(), dref, sref))
    w.finish()


# ---- boundary groups ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", SW.FAMILIES)
def test_boundary_groups(family):
    """assemble_boundary with an interface, a far-field and a slip group over all sides of all elements, trace and far-field
    states as per-point arrays (swhdg_boundary.hip), and the matrix-free boundary products of boundary_apply.hip."""
    torch = _torch()
    w = Worst(SW.BOUNDARY, family)
    for c, tag in cases(family, (1, 2)):
        blk, kw = make_block(c, graph=True)
        blk.set_physics_parameter("Roe-like stabilization", 1 if c["roe"] else 0)
        groups = SW.boundary_groups(c)
        b = SW.boundary_arrays(c, groups)
        keep = []
        for name, bc, be, bs, aux, ffp in groups:
            blk.add_boundary_group(name, bc, be, bs)
            for i, v in enumerate(("H", "Hux", "Huy")):
                t, f = dev(aux[..., i]), dev(ffp[..., i])
                keep += [t, f]
                blk.set_function("aux %s %s" % (v, name), t)
                blk.set_function("Far-field %s %s" % (v, name), f)
        nd, g = c["m"]["ndof"], c["g"]
        ud = dev(c["u"])
        res, vals = full((nd,), 0.0), full((len(g["colind"]),), 0.0)
        blk.assemble_boundary(ud, res, vals, **kw)
        torch.cuda.synchronize()
        w.add(tag + " res", H.distance(res.cpu().numpy(), b["res"], b["S_res"]))
        w.add(tag + " vals", H.distance(vals.cpu().numpy(), b["crs_vals"], b["S_vals"]))
        gb = dict(rowptr=g["rowptr"], colind=g["colind"], crs_vals=b["crs_vals"], S_vals=b["S_vals"])
        rng = np.random.default_rng(223)
        x = rng.uniform(0.5, 1.0, nd) * rng.choice([-1.0, 1.0], nd)
        for transpose in (False, True):
            Y, SY = H.matvec(gb, x, transpose)
            y = full((nd,), 0.0)
            blk.apply_boundary_jacobian(ud, dev(x), y, transpose=transpose, **kw)
            torch.cuda.synchronize()
            w.add("%s y %s" % (tag, "transposed" if transpose else "forward"), H.distance(y.cpu().numpy(), Y[0], SY[0]))
        d = full((nd,), 0.0)
        blk.boundary_jacobian_diagonal(ud, d, **kw)
        torch.cuda.synchronize()
        dref, sref = H.diagonal(gb)
        w.add(tag + " diagonal", H.distance(d.cpu().numpy(), dref, sref))
    w.finish()


# ---- the HDG element: uncondensed blocks, fused and unfused condensation ------------------------------------------------------------------
@pytest.mark.parametrize("family", SW.FAMILIES)
def test_element_blocks_and_condensed_element(family):
    """swhdg_element_blocks (res [E][36], blocks [E][36][36]: the side part), then S, g, du of swhdg_condensed_element (one
    fused kernel) and of the unfused pipeline element blocks + compute_local_jacres + batched_condense (condense.hip)."""
    import mrhyde_amd
    torch = _torch()
    w, wc = Worst(SW.MODULE, family), Both(family)
    for c, tag in cases(family, (1,)):
        blk, kw = make_block(c)
        E, sd = c["m"]["nmacro"], c["sd"]
        ud, ld = dev(c["u"]), dev(c["lam"])
        res, blocks = full((E, 36)), full((E, 36, 36))
        blk.swhdg_element_blocks(ud, ld, res, blocks, **side_kw(c), **kw)
        torch.cuda.synchronize()
        w.add(tag + " element res", H.distance(res.cpu().numpy(), sd["res"], sd["S_res"]))
        w.add(tag + " element blocks", H.distance(blocks.cpu().numpy(), sd["blocks"], sd["S_blocks"]))
        S, gv, du, ns = full((E, 24, 24)), full((E, 24)), full((E, 12)), full((1,), 0, torch.int32)
        blk.swhdg_condensed_element(ud, ld, schur=S, gvec=gv, du=du, num_singular=ns, **side_kw(c), **kw)
        torch.cuda.synchronize()
        assert int(ns[0]) == 0, tag
        check_condensed(wc, c, tag + " fused", S, gv, du)
        lJ, lr = full((E, 12, 12), 0.0), full((E, 12), 0.0)
        blk.compute_local_jacres(ud, lJ, lr, **kw)
        off = torch.tensor(np.asarray(c["m"]["offsets"]), device="cuda", dtype=torch.long)
        blocks[:, :12, :12] += lJ[:, off][:, :, off]
        res[:, :12] += lr[:, off]
        torch.cuda.synchronize()
        w.add(tag + " full res", H.distance(res.cpu().numpy(), c["res"], c["S_res"]))
        w.add(tag + " full blocks", H.distance(blocks.cpu().numpy(), c["blocks"], c["S_blocks"]))
        S2, g2, du2, nsing = mrhyde_amd.batched_condense(12, 24, blocks, res)
        assert nsing == 0, tag
        check_condensed(wc, c, tag + " unfused", S2, g2, du2)
    try:
        w.finish()
    finally:
        wc.finish()


# ---- subgrids ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("family", SW.FAMILIES)
def test_subgrid_blocks_and_condensed_subgrid(family, m):
    """swhdg_subgrid_blocks (the uncondensed system of n_int + 24 unknowns) and swhdg_condensed_subgrid (S, g, du).  A
    steady subgrid case whose cond_2(A_uu) exceeds 1e7 is compared uncondensed only (the conditioning guard)."""
    torch = _torch()
    w, wc = Worst(SW.MODULE, family), Both(family)
    for c, tag in cases(family, (m,)):
        blk, kw = make_block(c, layout=True)
        Em, ni = c["m"]["nmacro"], c["n_int"]
        N = ni + 24
        ud, ld = dev(c["u"]), dev(c["lam"])
        res, blocks = full((Em, N)), full((Em, N, N))
        blk.swhdg_subgrid_blocks(ud, ld, res, blocks, **side_kw(c), **kw)
        torch.cuda.synchronize()
        w.add(tag + " res", H.distance(res.cpu().numpy(), c["res"], c["S_res"]))
        w.add(tag + " blocks", H.distance(blocks.cpu().numpy(), c["blocks"], c["S_blocks"]))
        if c["cd"] is None:
            print("    %s: cond_2(A_uu) = %.3g > 1e7, condensed outputs not compared" % (tag, c["cond"]))
            continue
        S, gv, du, ns = full((Em, 24, 24)), full((Em, 24)), full((Em, ni)), full((1,), 0, torch.int32)
        blk.swhdg_condensed_subgrid(ud, ld, schur=S, gvec=gv, du=du, num_singular=ns, **side_kw(c), **kw)
        torch.cuda.synchronize()
        assert int(ns[0]) == 0, tag
        check_condensed(wc, c, tag, S, gv, du)
    try:
        w.finish()
    finally:
        wc.finish()


@pytest.mark.parametrize("family", SW.FAMILIES)
def test_subgrid_solve_one_pass(family, monkeypatch):
    """swhdg_subgrid_solve with max_iter = 1: every loop has done one assembly and one update, u + du against the
    yardstick; iters == 1 and the scaled norm is 1 where the yardstick's max norm of the interior residual is not 0.
    (At pass 0 the driver stores nrm / nrm: that is all of the norm its output holds.)  m = 1 without a layout is run
    twice, the second time under MHA_SUBGRID_UNFUSED=1.  Which pipeline ran is NOT asserted (no info key exposes it): by
    the library's code, which reads the variable at every call, the first is the one-element fused kernel and the second
    swhdg_element.hip, the point engine, subgrid.hip and condense.hip.  With a layout the subgrid kernel runs."""
    torch = _torch()
    monkeypatch.delenv("MHA_SUBGRID_UNFUSED", raising=False)
    wc = Both(family)
    runs = [(1, False, None), (1, False, "1")] + [(m, True, None) for m in (1, 2, 3, 4)]
    for m, layout, unfused in runs:
        for c, tag in cases(family, (m,), transients=(True,)):
            blk, kw = make_block(c, layout=layout)
            if unfused:
                monkeypatch.setenv("MHA_SUBGRID_UNFUSED", unfused)
            ud = dev(c["u"])
            out = blk.swhdg_subgrid_solve(ud, dev(c["lam"]), 1, 1e-9, want_condensed=False, **side_kw(c), **kw)
            torch.cuda.synchronize()
            monkeypatch.delenv("MHA_SUBGRID_UNFUSED", raising=False)
            ni, rows, cd = c["n_int"], c["rows"], c["cd"]
            nrm = np.abs(c["res"][:, :ni]).max(axis=1)
            assert int(out["num_singular"][0]) == 0 and np.all(out["iters"].cpu().numpy() == 1), tag
            assert np.array_equal(out["resnorm"].cpu().numpy(), (nrm > 0).astype(np.float64)), tag
            un = c["u"].astype(np.longdouble)[rows] + cd["du"]
            how = "layout" if layout else ("no layout, unfused" if unfused else "no layout, fused")
            wc.w.add("%s (%s) u + du" % (tag, how), H.distance(ud.cpu().numpy()[rows], un, np.abs(c["u"])[rows] + cd["S_du"]))
            wc.cw.add("%s (%s) u + du (componentwise scale)" % (tag, how),
                      H.distance(ud.cpu().numpy()[rows], un, np.abs(c["u"])[rows] + cd["C_du"]))
    wc.finish()


def test_refusals():
    """What the device refuses is refused by name: a deck-string source in the fused forms, the subgrid entry points
    without a layout, a layout outside 1..4."""
    import mrhyde_amd
    torch = _torch()
    c = SW.build_case("unit", 2, True, False)
    blk, kw = make_block(c)
    Em, ni = c["m"]["nmacro"], c["n_int"]
    S, gv, du, ns = full((Em, 24, 24)), full((Em, 24)), full((Em, ni)), full((1,), 0, torch.int32)
    args = (dev(c["u"]), dev(c["lam"]))
    with pytest.raises(mrhyde_amd.MhaError, match="no subgrid layout"):
        blk.swhdg_condensed_subgrid(*args, schur=S, gvec=gv, du=du, num_singular=ns, **side_kw(c))
    with pytest.raises(mrhyde_amd.MhaError, match=r"outside 1\.\.4"):
        blk.set_swhdg_subgrids(5)
    blk.set_swhdg_subgrids(2)
    blk.set_function("source H", "0.1*sin(x)")
    with pytest.raises(mrhyde_amd.MhaError, match="deck-string"):
        blk.swhdg_condensed_subgrid(*args, schur=S, gvec=gv, du=du, num_singular=ns, **side_kw(c))
    c1 = SW.build_case("unit", 1, True, False)
    blk1, _ = make_block(c1)
    blk1.set_function("source H", "0.1*sin(x)")
    E = c1["m"]["nmacro"]
    with pytest.raises(mrhyde_amd.MhaError, match="deck-string"):
        blk1.swhdg_condensed_element(dev(c1["u"]), dev(c1["lam"]), schur=full((E, 24, 24)), gvec=full((E, 24)), du=full((E, 12)),
                                     num_singular=ns, **side_kw(c1))
