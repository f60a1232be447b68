"""The geometry-database step with kept representatives on the GPU: one sequence of assemblies per mesh -- unchanged
inputs, new coefficient, new time-integration weights, mesh and graph set again, the caller's array overwritten with NaN
between calls, an accumulating assembly, copies enqueued right behind a call -- run three times: as it is, with the
representatives recomputed every call (MHA_BP_REP_CACHE=0) and with the full kernel (MHA_BP_DATABASE=0).  The CRS
values of every call must agree bit for bit, and the info key "block_pattern_rep_launches" must show that the kept
representatives really were used."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = np.array([[0.2928932188, 0.0], [0.7071067812, 0.2928932188]])
BB = np.array([0.7071067812, 0.2928932188])
BDF = np.array([1.5, -2.0, 0.5])
BDF2 = np.array([1.0, -1.0, 0.0])
NSTEPS, NSTAGES = 2, 2


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _sequence(monkeypatch, mode, dim, order, ncell, transient):
    """-> (labels, CRS values of every call, representative launches after every call, database mode of every call)"""
    torch = _torch()
    import mrhyde_amd
    for k in ("MHA_K1", "MHA_K2", "MHA_BP_DATABASE", "MHA_BP_REP_CACHE"):
        monkeypatch.delenv(k, raising=False)
    if mode == "recompute":
        monkeypatch.setenv("MHA_BP_REP_CACHE", "0")
    elif mode == "full":
        monkeypatch.setenv("MHA_BP_DATABASE", "0")
    m = mrhyde_amd.mesh_structured(dim, order, ncell)   # spacings are powers of two: one geometry shape
    nrows = m["ndof"]
    rng = np.random.default_rng(17)
    u = torch.tensor(rng.uniform(-1, 1, nrows), device="cuda")
    u_prev = torch.tensor(rng.uniform(-1, 1, (nrows, NSTEPS)), device="cuda")
    u_stage = torch.tensor(rng.uniform(-1, 1, (nrows, NSTAGES)), device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    labels, vals_out, launches, dbmode = [], [], [], []
    with torch.cuda.stream(stream):
        blk = mrhyde_amd.Block(dim, order, quadrature=2 * order, workset_size=100)
        blk.set_stream(stream.cuda_stream)
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], nrows, m["boundary"])
        blk.set_graph()
        blk.set_function("thermal source", ("sinprod", 3.0, [1.3, 0.7, 2.1][:dim]))
        blk.set_function("thermal diffusion", 1.7)
        blk.set_function("density", 1.3)
        blk.set_function("specific heat", 0.7)
        kw = {}
        if transient:
            blk.set_time_integration(True, NSTEPS, NSTAGES, 1, 0.02, A, BB, BDF)
            kw = dict(u_prev=u_prev, u_stage=u_stage)
        nnz = blk.get_graph()[1].shape[0]
        res = torch.zeros(nrows, dtype=torch.float64, device="cuda")
        vals = torch.empty(nnz, dtype=torch.float64, device="cuda")
        assert vals.data_ptr() % 128 == 0

        def call(label, overwrite=True, fill=float("nan"), copies=False):
            vals.fill_(fill)   # every entry, the representatives' positions included
            blk.assemble_jacres(u, res, vals, path=mrhyde_amd.PATH_ROW_OWNER, compute_jacobian=True, overwrite=overwrite, **kw)
            if copies:  # enqueued on the caller's stream right behind the call, nothing in between
                vc, rc = vals.clone(), res.clone()
            stream.synchronize()
            if copies:
                assert np.array_equal(vc.cpu().numpy(), vals.cpu().numpy()), "copy of vals behind the call: " + label
                assert np.array_equal(rc.cpu().numpy(), res.cpu().numpy()), "copy of res behind the call: " + label
                assert not np.any(np.isnan(rc.cpu().numpy()))
            labels.append(label)
            vals_out.append(vals.cpu().numpy().copy())
            launches.append(blk.info("block_pattern_rep_launches"))
            dbmode.append(blk.info("jacobian_database_mode"))

        call("first")
        assert blk.info("block_patterns") > 1 and blk.info("affine_shapes") == 1
        call("second, unchanged", copies=True)
        call("third, unchanged", copies=True)
        blk.set_function("thermal diffusion", 2.3)
        call("new diffusion", copies=True)
        blk.set_time_integration(True, NSTEPS, NSTAGES, 0, 0.05, A, BB, BDF2)
        kw = dict(u_prev=u_prev, u_stage=u_stage)
        call("new time-integration weights", copies=True)
        call("unchanged again")
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], nrows, m["boundary"])
        blk.set_graph()
        call("mesh and graph set again", copies=True)
        call("accumulating", overwrite=False, fill=1.0)
        call("after the accumulating call")
        del blk
    return labels, vals_out, launches, dbmode


@pytest.mark.parametrize("dim,order,ncell,transient", [(3, 2, (16, 8, 8), False), (3, 2, (16, 8, 8), True),
                                                       (3, 1, (32, 16, 8), False), (3, 1, (32, 16, 8), True),
                                                       (2, 2, (64, 32), False), (2, 2, (64, 32), True)])
def test_kept_representatives_bit_identical(monkeypatch, dim, order, ncell, transient):
    labels, kept, n_kept, db_kept = _sequence(monkeypatch, "kept", dim, order, ncell, transient)
    _, again, n_again, db_again = _sequence(monkeypatch, "recompute", dim, order, ncell, transient)
    _, full, n_full, db_full = _sequence(monkeypatch, "full", dim, order, ncell, transient)
    # first 1; unchanged 1 1; diffusion 2; weights 3; unchanged 3; mesh + graph 4; accumulating (full kernel) 4; then 4
    assert n_kept == [1, 1, 1, 2, 3, 3, 4, 4, 4], n_kept
    assert db_kept == [1, 1, 1, 1, 1, 1, 1, 0, 1], db_kept
    assert n_again == [1, 2, 3, 4, 5, 6, 7, 7, 8], n_again
    assert db_again == db_kept
    assert n_full == [0] * 9 and db_full == [0] * 9
    for label, a, b, c in zip(labels, kept, again, full):
        assert not np.any(np.isnan(c)), "the full kernel writes every entry: " + label
        assert np.array_equal(a, b), "kept vs. recomputed representatives: " + label
        assert np.array_equal(a, c), "database mode vs. the full kernel: " + label
    # the sequence does change the values where it changes the inputs
    assert not np.array_equal(kept[2], kept[3]) and not np.array_equal(kept[3], kept[4])
    assert np.array_equal(kept[0], kept[1]) and np.array_equal(kept[0], kept[2]) and np.array_equal(kept[4], kept[5])
    assert np.array_equal(kept[5], kept[6]) and np.array_equal(kept[6], kept[8])
