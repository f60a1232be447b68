"""The geometry-database mode's representatives kernel (one wavefront per unit column tile) on meshes of several roles:
3-D Q2 and Q1 hexes and 2-D Q2 quads, steady and transient.  The CRS values start as NaN inside a larger tensor: the
database mode must write every entry, bit for bit what the full kernel writes, and nothing outside the caller's view."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096  # entries of the larger tensor before and after the caller's view (a multiple of 16: the view stays aligned)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.mark.parametrize("dim,order,ncell,transient", [(3, 2, (16, 8, 8), False), (3, 2, (16, 8, 8), True),
                                                       (3, 1, (32, 16, 8), False), (3, 1, (32, 16, 8), True),
                                                       (2, 2, (64, 32), False), (2, 2, (64, 32), True)])
def test_database_representatives_bit_identical(monkeypatch, dim, order, ncell, transient):
    torch = _torch()
    import mrhyde_amd
    for k in ("MHA_K1", "MHA_K2", "MHA_BP_DATABASE"):
        monkeypatch.delenv(k, raising=False)
    qdeg = 2 * order
    m = mrhyde_amd.mesh_structured(dim, order, ncell)   # spacings are powers of two: one geometry shape
    nrows = m["ndof"]
    rng = np.random.default_rng(11)
    u = torch.tensor(rng.uniform(-1, 1, nrows), device="cuda")
    nsteps, nstages, stage = 2, 2, 1
    A = np.array([[0.2928932188, 0.0], [0.7071067812, 0.2928932188]])
    bb = np.array([0.7071067812, 0.2928932188])
    bdf = np.array([1.5, -2.0, 0.5])
    u_prev = torch.tensor(rng.uniform(-1, 1, (nrows, nsteps)), device="cuda")
    u_stage = torch.tensor(rng.uniform(-1, 1, (nrows, nstages)), device="cuda")
    got = {}
    for db in (True, False):
        if not db:
            monkeypatch.setenv("MHA_BP_DATABASE", "0")
        blk = mrhyde_amd.Block(dim, order, quadrature=qdeg, workset_size=100)
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], nrows, m["boundary"])
        blk.set_graph()
        blk.set_function("thermal source", ("sinprod", 3.0, [1.3, 0.7, 2.1][:dim]))
        blk.set_function("thermal diffusion", 1.7)
        kw = {}
        if transient:
            blk.set_function("density", 1.3)
            blk.set_function("specific heat", 0.7)
            blk.set_time_integration(True, nsteps, nstages, stage, 0.02, A, bb, bdf)
            kw = dict(u_prev=u_prev, u_stage=u_stage)
        nnz = blk.get_graph()[1].shape[0]
        res = torch.zeros(nrows, dtype=torch.float64, device="cuda")
        big = torch.full((nnz + 2 * GUARD,), 1234.5, dtype=torch.float64, device="cuda")
        vals = big[GUARD:GUARD + nnz]
        vals.fill_(float("nan"))
        assert vals.data_ptr() % 128 == 0
        blk.assemble_jacres(u, res, vals, path=mrhyde_amd.PATH_ROW_OWNER, compute_jacobian=True, overwrite=True, **kw)
        torch.cuda.synchronize()
        assert blk.info("block_patterns") > 1 and blk.info("affine_shapes") == 1
        assert blk.info("jacobian_database_mode") == (1 if db else 0)
        g = np.concatenate([big[:GUARD].cpu().numpy(), big[GUARD + nnz:].cpu().numpy()])
        assert np.all(g == 1234.5), "entries outside the caller's view were written"
        got[db] = vals.cpu().numpy()
        del blk, big, vals, res
    assert not np.any(np.isnan(got[False])), "the full kernel writes every entry"
    assert np.array_equal(got[True], got[False])
