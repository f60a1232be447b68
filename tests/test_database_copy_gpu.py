"""The database modes' line-aligned copy at the benchmark's full sizes (config 2: thermal Q2 hexes on 64^3, geometry
database; config 3: porousMixed on 128^3, row classes).  The CRS values start as NaN inside a larger tensor: the
database mode must write every entry (bit for bit what the full kernel writes) and nothing outside the caller's view."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HGRAD, HVOL, HDIV = 0, 1, 2
GUARD = 4096  # entries of the larger tensor before and after the caller's view (a multiple of 16: the view stays aligned)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _guarded(torch, nnz):
    big = torch.full((nnz + 2 * GUARD,), 1234.5, dtype=torch.float64, device="cuda")
    vals = big[GUARD:GUARD + nnz]
    vals.fill_(float("nan"))
    assert vals.data_ptr() % 128 == 0
    return big, vals


def _check_guards(big, nnz):
    g = np.concatenate([big[:GUARD].cpu().numpy(), big[GUARD + nnz:].cpu().numpy()])
    assert np.all(g == 1234.5), "entries outside the caller's view were written"


def test_thermal_config2_database_copy(monkeypatch):
    torch = _torch()
    import mrhyde_amd
    for k in ("MHA_K1", "MHA_K2", "MHA_BP_DATABASE"):
        monkeypatch.delenv(k, raising=False)
    dim, order, qdeg, ncell = 3, 2, 4, (64, 64, 64)
    m = mrhyde_amd.mesh_structured(dim, order, ncell)
    nrows = m["ndof"]
    u = torch.tensor(np.random.default_rng(2).uniform(-1, 1, nrows), device="cuda")
    got = {}
    for db in (True, False):
        if not db:
            monkeypatch.setenv("MHA_BP_DATABASE", "0")
        blk = mrhyde_amd.Block(dim, order, quadrature=qdeg, workset_size=100)
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], nrows, m["boundary"])
        blk.set_graph()
        blk.set_function("thermal source", ("sinprod", 12 * np.pi ** 2, [2 * np.pi] * 3))
        blk.set_function("thermal diffusion", 1.0)
        nnz = blk.get_graph()[1].shape[0]
        res = torch.zeros(nrows, dtype=torch.float64, device="cuda")
        big, vals = _guarded(torch, nnz)
        blk.assemble_jacres(u, res, vals, compute_jacobian=True, overwrite=True)
        torch.cuda.synchronize()
        assert blk.info("jacobian_database_mode") == (1 if db else 0)
        _check_guards(big, nnz)
        got[db] = vals.cpu().numpy()
        del blk, big, vals, res
        torch.cuda.empty_cache()
    assert not np.any(np.isnan(got[False])), "the full kernel writes every entry"
    assert np.array_equal(got[True], got[False])


def test_porous_config3_database_copy(monkeypatch):
    torch = _torch()
    import mrhyde_amd
    monkeypatch.delenv("MHA_POROUS_DATABASE", raising=False)
    nc = 128
    m = mrhyde_amd.mesh_multi(3, (nc,) * 3, [HVOL, HDIV], [0, 1], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    nrows = m["ndof"]
    u = torch.tensor(np.random.default_rng(4).uniform(-1, 1, nrows), device="cuda")
    got = {}
    for db in (True, False):
        if not db:
            monkeypatch.setenv("MHA_POROUS_DATABASE", "0")
        blk = mrhyde_amd.Block(3, quadrature=2, physics="porousMixed", variables=[(HVOL, 0), (HDIV, 1)])
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], nrows)
        blk.set_orientation(m["orient"])
        blk.set_graph()
        blk.set_function("source", ("sinprod", 12 * np.pi ** 2, [2 * np.pi] * 3))
        nnz = blk.get_graph()[1].shape[0]
        res = torch.zeros(nrows, dtype=torch.float64, device="cuda")
        big, vals = _guarded(torch, nnz)
        blk.assemble_jacres(u, res, vals, compute_jacobian=True, overwrite=True)
        torch.cuda.synchronize()
        assert blk.info("porous_direct") == (2 if db else 1)
        _check_guards(big, nnz)
        got[db] = vals.cpu().numpy()
        del blk, big, vals, res
        torch.cuda.empty_cache()
    assert not np.any(np.isnan(got[False])), "the direct form writes every entry"
    assert np.array_equal(got[True], got[False])
