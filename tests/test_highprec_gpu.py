"""The device (through the C ABI) against the extended-precision yardstick of tests/highprec_ref.py, entry by entry:
d = |device - yardstick| / (2^-53 S) with S the scale of the entry's own sum, and exact zeros where S == 0.  The bound per
(module, input family) is max(8 K_oracle, 8) with K_oracle the CPU oracle's own d on the same inputs, recorded in
highprec_ref.K_ORACLE and re-measured by tests/test_highprec.py; it is never taken from the device.  Every test prints
its largest d beside its bound.  The yardstick's arrays are computed once per case (highprec_ref.build_case)."""
import re

import numpy as np
import pytest

import highprec_ref as H

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _dev(a):
    return _torch().tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def make_block(c):
    import mrhyde_amd
    m, P, mod, dim = c["m"], c["P"], c["module"], c["dim"]
    if mod == "thermal":
        blk = mrhyde_amd.Block(dim, c["orders"][0], quadrature=c["qdeg"], workset_size=100)
        funcs = {"thermal source": P["source"], "thermal diffusion": P["diffusion"], "density": P["rho"], "specific heat": P["cp"]}
        params = {}
        if P["adv"] is not None:                                   # (b . grad e, v): the point engine's thermal
            funcs.update(zip(("bx", "by", "bz"), P["adv"]))
            params["include advection"] = 1
        if callable(P["diffusion"]):                               # a deck string that reads the solution field
            funcs["thermal diffusion"] = P["diffusion_text"]
            funcs["thermal source"] = H.sinprod_text(P["source"], dim)
    else:
        # the deck as the case states it: numbers, ("sinprod", ..), per-point data as a tensor, deck text for the functions
        # that read the fields, their named helpers, and the functions that no term reads
        blk = mrhyde_amd.Block(dim, quadrature=c["qdeg"], physics=mod, variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
        funcs, params = H.deck(c)
        funcs = {k: _dev(v[1]) if isinstance(v, tuple) and v[0] == "array" else v for k, v in funcs.items()}
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], c["fixed"])
    if mod != "thermal":
        blk.set_orientation(m["orient"])
    blk.set_graph(c["g"]["rowptr"], c["g"]["colind"])
    for k, v in funcs.items():
        blk.set_function(k, v)
    for k, v in params.items():
        blk.set_physics_parameter(k, v)
    kw = {}
    tr = c["tr"]
    if tr is not None:
        blk.set_time_integration(True, 2, 2, tr["stage"], tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
        kw = dict(u_prev=_dev(tr["u_prev"]), u_stage=_dev(tr["u_stage"]))
    return blk, kw


class Worst:
    """The largest d of a test beside its bound; the assertion comes after every figure is printed."""

    def __init__(self, module, family):
        self.module, self.family, self.bound = module, family, H.device_bound(module, family)
        self.d, self.where = 0.0, None

    def add(self, what, d):
        print("    %-60s d = %.3g" % (what, d))
        if not d <= self.d:                                        # (a NaN counts as the largest)
            self.d, self.where = d, what

    def finish(self):
        print("%s, %s: largest d = %.3g (%s), bound max(8 K_oracle, 8) = %.3g" % (self.module, self.family, self.d, self.where, self.bound))
        assert self.d <= self.bound, (self.where, self.d, self.bound)   # false for a NaN too


def assemble(blk, c, kw, path):
    """overwrite=True on garbage: every entry must be written, fixed rows as zero rows."""
    torch = _torch()
    res = torch.full((c["m"]["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((len(c["g"]["colind"]),), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(_dev(c["u"]), res, vals, path=path, overwrite=True, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy(), vals.cpu().numpy()


def check_global(w, c, tag, res, vals):
    g = c["g"]
    w.add(tag + " crs_vals", H.distance(vals, g["crs_vals"], g["S_vals"]))
    w.add(tag + " res", H.distance(res, g["res"], g["S_res"]))


def check_local(w, blk, c, kw, tag):
    torch = _torch()
    E, n = c["m"]["lids"].shape
    lJ = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
    lr = torch.zeros((E, n), dtype=torch.float64, device="cuda")
    blk.compute_local_jacres(_dev(c["u"]), lJ, lr, **kw)
    torch.cuda.synchronize()
    el = c["el"]
    w.add(tag + " local_J", H.distance(lJ.cpu().numpy(), el["local_J"], el["S_J"]))
    w.add(tag + " local_res", H.distance(lr.cpu().numpy(), el["local_res"], el["S_res"]))


def cases(oracle, module, family):
    for shape, transient, variant in H.case_list(module, family):
        c = H.build_case(oracle, module, shape, family, transient, variant)
        yield c, c["tag"]


# ---- thermal -----------------------------------------------------------------------------------------------------------------
AFFINE_ROW_OWNER = {(2, 1), (2, 2), (2, 4), (3, 1), (3, 2)}       # (dim, order) of the fused affine kernels
# Q3 quads have the general row-owner kernel and the point engine only: the element kernels behind these refuse them
# (an error that names the shape, never another kernel in their place)
Q3_REFUSED = {"ELEMENT_ATOMIC", "LOCAL_THEN_SCATTER", "compute_local_jacres"}


def refused(fn):
    """True if the device refuses the call as unsupported for the shape (MHA_ERR_INVALID, message says so)."""
    import mrhyde_amd
    try:
        fn()
    except mrhyde_amd.MhaError as e:
        assert e.code == 1 and "unsupported" in str(e), str(e)
        return True
    return False


@pytest.mark.parametrize("family", H.families("thermal"))
def test_thermal_paths(oracle, monkeypatch, capfd, family):
    import mrhyde_amd as M

    def flush():                                                    # what the test printed so far, past the capture
        out, err = capfd.readouterr()
        with capfd.disabled():
            print(out, end="")
        return err
    for k in ("MHA_K1", "MHA_K2", "MHA_BP_DATABASE", "MHA_K1_ORDER"):
        monkeypatch.delenv(k, raising=False)
    w = Worst("thermal", family)
    affine = family in ("stretched aligned", "stretched sheared")
    trimmed = {}
    for c, tag in cases(oracle, "thermal", family):
        blk, kw = make_block(c)
        E = c["m"]["nelem"]
        fused = affine and (c["dim"], c["orders"][0]) in AFFINE_ROW_OWNER
        if family in H.THERMAL_ONLY:
            for name, path in (("AUTO", M.PATH_AUTO), ("POINT_ENGINE", M.PATH_POINT_ENGINE), ("ROW_GATHER", M.PATH_ROW_GATHER)):
                res, vals = assemble(blk, c, kw, path)
                assert blk.info("last_path") == (M.PATH_ROW_GATHER if name == "AUTO" else path), tag
                check_global(w, c, "%s %s" % (tag, name), res, vals)
            check_local(w, blk, c, kw, tag)
            continue
        for name, path in (("AUTO", M.PATH_AUTO), ("ROW_OWNER", M.PATH_ROW_OWNER), ("ELEMENT_ATOMIC", M.PATH_ELEMENT_ATOMIC),
                           ("LOCAL_THEN_SCATTER", M.PATH_LOCAL_THEN_SCATTER), ("POINT_ENGINE", M.PATH_POINT_ENGINE),
                           ("ROW_GATHER", M.PATH_ROW_GATHER)):
            if c["orders"][0] == 3:
                out = []
                no = refused(lambda: out.extend(assemble(blk, c, kw, path)))
                assert no == (name in Q3_REFUSED), (tag, name, "refused" if no else "ran")
                if no:
                    continue
                res, vals = out
            else:
                res, vals = assemble(blk, c, kw, path)
            if name in ("AUTO", "ROW_OWNER"):                       # which kernel really ran
                assert blk.info("last_path") == M.PATH_ROW_OWNER and blk.info("row_owner_kind") == (1 if fused else 2), tag
                if fused:
                    assert blk.info("num_affine_elems") == E, tag
                elif not affine:
                    assert blk.info("num_affine_elems") < E, tag
                if fused:
                    # geometry-database mode (one representative row block per pattern, rows replicated) where the block
                    # has one element geometry: the axis-aligned 2^dim meshes, whose spacings are exact; the 3 x 2 meshes
                    # (spacing 1/3) and the sheared ones classify into several geometries and run the full kernel
                    db = 1 if family == "stretched aligned" and set(c["shape"][2]) == {2} else 0
                    assert blk.info("block_patterns") > 0 and blk.info("jacobian_database_mode") == db, (tag, db)
                    name += " (affine, database mode %d)" % db
            else:
                assert blk.info("last_path") == path, tag
            check_global(w, c, "%s %s" % (tag, name), res, vals)
        if c["orders"][0] == 3:
            assert refused(lambda: check_local(w, blk, c, kw, tag)) == ("compute_local_jacres" in Q3_REFUSED), tag
        else:
            check_local(w, blk, c, kw, tag)
        if fused:
            # the full block-pattern kernel (no geometry database), then the LDS-accumulator row-block kernel
            for env, val, what in (("MHA_BP_DATABASE", "0", "full block-pattern kernel"), ("MHA_K2", "blocks", "K2 = blocks")):
                monkeypatch.setenv(env, val)
                monkeypatch.setenv("MHA_VERBOSE", "1")                # the plan's unit shapes on stderr
                flush()
                blk2, kw2 = make_block(c)
                res, vals = assemble(blk2, c, kw2, M.PATH_ROW_OWNER)
                monkeypatch.delenv("MHA_VERBOSE")
                units = re.findall(r"units ks (\d+) tiles (\d+) tail (\d) trim (\d) fixed (\d): (\d+)", flush())
                if env == "MHA_BP_DATABASE":
                    assert units, tag
                    trimmed[tag] = sum(int(u[5]) for u in units if u[3] != "0")
                assert blk2.info("row_owner_kind") == 1 and blk2.info("jacobian_database_mode") == 0, tag
                assert (blk2.info("block_patterns") > 0) == (env == "MHA_BP_DATABASE"), tag
                check_global(w, c, "%s ROW_OWNER, %s" % (tag, what), res, vals)
                monkeypatch.delenv(env)
    try:
        if affine:
            # the zero-block shortcut of the block-pattern kernel (trim classes 1..4 of the 8-element vertex units) really ran
            print("units with a trim class per case:", trimmed)
            assert trimmed["Q2 hex steady"] > 0 and trimmed["Q2 hex stage 1"] > 0, trimmed
        w.finish()
    finally:
        flush()


# ---- navierstokes and linearelasticity -----------------------------------------------------------------------------------------
def products(w, blk, c, kw, tag):
    """apply_jacobian forward and transposed, jacobian_diagonal and apply_jacobian_multi (K = 3) against the yardstick's
    matrix times the same vectors."""
    torch = _torch()
    g, nd = c["g"], c["m"]["ndof"]
    rng = np.random.default_rng(211)
    amp = 1e3 if c["family"].startswith("units") else 1.0
    X = amp * rng.uniform(0.5, 1.0, (3, nd)) * rng.choice([-1.0, 1.0], (3, nd))
    ud = _dev(c["u"])
    for transpose in (False, True):
        Y, SY = H.matvec(g, X, transpose)
        y = torch.full((nd,), 3.25, dtype=torch.float64, device="cuda")
        blk.apply_jacobian(ud, _dev(X[0]), y, transpose=transpose, overwrite=True, **kw)
        Ym = torch.full((3, nd), 3.25, dtype=torch.float64, device="cuda")
        blk.apply_jacobian_multi(ud, _dev(X), Ym, transpose=transpose, overwrite=True, **kw)
        torch.cuda.synchronize()
        t = "transposed" if transpose else "forward"
        w.add("%s apply_jacobian %s" % (tag, t), H.distance(y.cpu().numpy(), Y[0], SY[0]))
        w.add("%s apply_jacobian_multi K = 3 %s" % (tag, t), H.distance(Ym.cpu().numpy(), Y, SY))
    d = torch.full((nd,), 3.25, dtype=torch.float64, device="cuda")
    blk.jacobian_diagonal(ud, d, overwrite=True, **kw)
    torch.cuda.synchronize()
    dref, sref = H.diagonal(g)
    w.add("%s jacobian_diagonal" % tag, H.distance(d.cpu().numpy(), dref, sref))


@pytest.mark.parametrize("module,family", [(mod, fam) for mod in ("navierstokes", "linearelasticity") + H.LATER for fam in H.families(mod)])
def test_engine_modules(oracle, module, family):
    """Every case of the (module, family) key on AUTO, POINT_ENGINE and ROW_GATHER, compute_local_jacres and the
    matrix-free products, each array judged by H.distance against max(8 K_oracle, 8).  [cdr-unit fields] is the case
    that found jacobian_diagonal returning 0.0 or stale values in 3-D with a deck string that reads the fields
    (profiles/extended_precision_yardstick.md)."""
    import mrhyde_amd as M
    w = Worst(module, family)
    for c, tag in cases(oracle, module, family):
        if c["variant"] == 0:
            blk, kw = make_block(c)
        else:                                                       # the same mesh, data and functions: the switches alone
            for k, v in H.deck(c)[1].items():
                blk.set_physics_parameter(k, v)
        for name, path, last in (("AUTO", M.PATH_AUTO, M.PATH_ROW_GATHER), ("POINT_ENGINE", M.PATH_POINT_ENGINE, M.PATH_POINT_ENGINE),
                                 ("ROW_GATHER", M.PATH_ROW_GATHER, M.PATH_ROW_GATHER)):
            res, vals = assemble(blk, c, kw, path)
            assert blk.info("last_path") == last, tag
            check_global(w, c, "%s %s" % (tag, name), res, vals)
        if module.startswith("navierstokes") and c["dim"] == 3:     # the reference's uz-offset quirk: uz rows stay empty
            uz = res[(c["m"]["dof_var"] == 3) & (c["fixed"] == 0)]
            assert np.all(uz == 0.0) if not c["P"]["fix_uz_offsets"] else np.all(uz != 0.0), tag
        check_local(w, blk, c, kw, tag)
        products(w, blk, c, kw, tag)
    w.finish()
