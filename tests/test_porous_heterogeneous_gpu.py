"""GPU tests of porousMixed's heterogeneous permeability: "use permeability data" (Kinv = 1 / element data, updatePerm,
porousMixed.cpp:550-563) and "use KL expansion" (Kinv / exp of a Karhunen-Loeve field at every point, updateKLPerm,
porousMixed.cpp:567-714) on every porousMixed volume path -- the direct form, the dense local arrays, the point engine,
residual-only, transient, worksets smaller than the block -- against the same block with Kinv_* given as IP arrays
and against the CPU oracle; the regression/porous/Mixed_PermData gold end to end; database mode declining; a coefficient
vector changed between two assemblies."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_multi_gpu import RTOL, _torch, crs_err, make_block, rel_err, transient_state, warp
from test_porous_heterogeneous import np_kl_indices, np_kl_roots

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
FUNCS = {"source": ("sinprod", 2.0, [1.1, 0.7, 1.9]), "total_mobility": 1.9}


def _funcs(dim):
    return {"source": ("sinprod", 2.0, FUNCS["source"][2][:dim]), "total_mobility": 1.9}


def _ip_points(oracle, m, qdeg=2):
    return oracle.physical_basis_var(m["dim"], oracle.HVOL, 0, qdeg, m["nodes"])["ip"]  # [E][nq][dim]


def _assemble_all(blk, m, u, nnz, tr=None, monkeypatch=None):
    """Every porousMixed volume path of a block -> dict of numpy arrays."""
    torch = _torch()
    import mrhyde_amd
    kw = {}
    if tr is not None:
        blk.set_time_integration(True, 2, 2, 1, tr["dt"], tr["butcher_A"], tr["butcher_b"], tr["bdf"])
        kw = dict(u_prev=torch.tensor(tr["u_prev"], device="cuda"), u_stage=torch.tensor(tr["u_stage"], device="cuda"))
    ud = torch.tensor(u, device="cuda")
    out = {}
    res = torch.full((m["ndof"],), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.full((nnz,), -3.0, dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, overwrite=True, **kw)  # AUTO: the direct form
    torch.cuda.synchronize()
    assert blk.info("porous_direct") == 1
    out["res"], out["crs_vals"] = res.cpu().numpy().copy(), vals.cpu().numpy().copy()
    blk.assemble_jacres(ud, res, vals, compute_jacobian=False, overwrite=True, **kw)  # residual only: the lean build
    out["res_only"] = res.cpu().numpy().copy()
    r, v = torch.zeros_like(res), torch.zeros_like(vals)
    blk.assemble_jacres(ud, r, v, path=mrhyde_amd.PATH_POINT_ENGINE, **kw)  # the point engine (atomic scatter)
    out["res_engine"], out["crs_engine"] = r.cpu().numpy(), v.cpu().numpy()
    r, v = torch.zeros_like(res), torch.zeros_like(vals)
    blk.assemble_jacres(ud, r, v, path=mrhyde_amd.PATH_LOCAL_THEN_SCATTER, **kw)  # dense arrays, workset by workset
    out["res_local"], out["crs_local"] = r.cpu().numpy(), v.cpu().numpy()
    E, n = m["lids"].shape
    lJ = torch.zeros((E, n, n), dtype=torch.float64, device="cuda")
    lr = torch.zeros((E, n), dtype=torch.float64, device="cuda")
    blk.compute_local_jacres(ud, lJ, lr, **kw)
    out["local_J"], out["local_res"] = lJ.cpu().numpy(), lr.cpu().numpy()
    torch.cuda.synchronize()
    return out


def _check_against(got, ip, ref, strict):
    """got / ip: _assemble_all of the heterogeneous block and of its IP-array twin; ref: the oracle."""
    for k in got:
        assert rel_err(got[k], ip[k]) < strict, k
    for k in ("crs_vals", "crs_engine", "crs_local"):
        assert crs_err(got[k], ref) < RTOL, k
    for k in ("res", "res_only", "res_engine", "res_local"):
        assert rel_err(got[k], ref["res"]) < RTOL, k
    assert rel_err(got["local_J"], ref["local_J"]) < RTOL and rel_err(got["local_res"], ref["local_res"]) < RTOL


@pytest.mark.parametrize("dim,ncell", [(2, (7, 5)), (3, (4, 3, 3))])
@pytest.mark.parametrize("transient", [False, True])
def test_element_data_equals_ip_arrays(oracle, dim, ncell, transient):
    torch = _torch()
    import mrhyde_amd
    rng = np.random.default_rng(81)
    m = warp(oracle.mesh_multi(dim, ncell, [oracle.HVOL, oracle.HDIV], [0, 1]))
    E, nq = m["nelem"], oracle.ref_sizes(dim, 1, 2)[1]
    data = np.stack([rng.uniform(0.2, 5.0, E), rng.uniform(-1, 1, E)], 1)  # two columns: column 0 is read
    kinv = np.repeat(1.0 / data[:, :1], nq, axis=1)
    u = rng.uniform(-1, 1, m["ndof"])
    tr = transient_state(rng, m["ndof"], u) if transient else None
    funcs = _funcs(dim)
    ref = oracle.assemble_block(m, oracle.PHYS_POROUS_MIXED, 2, u, transient=tr, want_local=True,
                                funcs=dict(funcs, Kinv_xx=("array", kinv), Kinv_yy=("array", kinv), Kinv_zz=("array", kinv)))
    graph = (ref["rowptr"], ref["colind"])
    blocks = {}
    for het in (True, False):
        blk = mrhyde_amd.Block(dim, quadrature=2, physics="porousMixed", workset_size=E // 3 + 1,
                               variables=list(zip(m["types"].tolist(), m["orders"].tolist())))
        blk.set_mesh(m["nodes"], m["lids"], m["offsets"], m["ndof"], None)
        blk.set_orientation(m["orient"])
        blk.set_graph(*graph)
        assert blk.num_worksets() == 3
        for k, v in funcs.items():
            blk.set_function(k, v)
        if het:
            blk.set_function("Kinv_xx", 123.0)  # replaced by the data
            blk.set_element_data(data)
            blk.set_physics_parameter("use permeability data", 1)
        else:
            keep = torch.tensor(kinv, device="cuda")
            for k in ("Kinv_xx", "Kinv_yy", "Kinv_zz"):
                blk.set_function(k, keep)
        blocks[het] = (blk, _assemble_all(blk, m, u, len(ref["colind"]), tr))
    _check_against(blocks[True][1], blocks[False][1], ref, 1e-14)


def _kl_field(dim, x, kl, uq, stoch, fix):
    """numpy restatement of updateKLPerm at points x [..., dim] -> log-fields [..., dim] (KL_xx, KL_yy[, KL_zz])."""
    N = [k["N"] for k in kl]
    ex = [np_kl_roots(k["N"], k["L"], k["sigma"], k["eta"]) for k in kl]

    def phi(d, i, xd):
        w, eta, L = ex[d][0][i], kl[d]["eta"], kl[d]["L"]
        return (eta * w * np.cos(w * xd) + np.sin(w * xd)) / np.sqrt((eta * eta * w * w + 1.0) * L / 2.0 + eta)

    idx = np_kl_indices(dim, N + [1] * (3 - dim))
    out = np.zeros(x.shape[:-1] + (dim,))

    def term(t, c, quirk):
        i, j = idx[t][0], idx[t][1]
        lam = ex[0][1][i] * ex[1][1][j]
        ev = phi(0, i, x[..., 0]) * phi(1, j, x[..., 1])
        if dim == 3:
            k = idx[t][2]
            lam *= ex[1][1][k] if quirk else ex[2][1][k]
            ev = ev * phi(2, k, x[..., 2])
        v = c * np.sqrt(lam) * ev
        if quirk:
            out[..., 0] += 2 * v
            out[..., 1] += v
        else:
            out[..., :] += v[..., None]

    prog = 0
    if uq is not None:
        for t in range(min(len(uq), len(idx))):
            term(t, uq[t], dim == 3 and not fix)
        prog = len(uq)
    if stoch is not None:
        for t in range(prog, min(len(idx), prog + len(stoch))):
            term(t, stoch[t - prog], False)
    return out


def _set_kl(blk, kl, fix):
    blk.set_physics_parameter("use KL expansion", 1)
    blk.set_physics_parameter("fix_KL_3d", fix)
    for d, p in zip("xyz", kl):
        for key in ("N", "L", "sigma", "eta"):
            blk.set_physics_parameter("KL %s %s" % (key, d), p[key])


KL3 = [dict(N=3, L=1.0, sigma=1.0, eta=0.3), dict(N=4, L=1.2, sigma=1.0, eta=0.5), dict(N=2, L=0.9, sigma=1.0, eta=0.2)]


@pytest.mark.parametrize("dim,fix", [(2, 0), (3, 0), (3, 1)])
@pytest.mark.parametrize("coeffs", ["uq", "stoch", "both", "both+data"])
def test_kl_field_vs_restatement(oracle, dim, fix, coeffs):
    torch = _torch()
    rng = np.random.default_rng(91 + dim + 10 * fix)
    ncell = (6, 5) if dim == 2 else (3, 4, 3)
    m = warp(oracle.mesh_multi(dim, ncell, [oracle.HVOL, oracle.HDIV], [0, 1]))
    kl = KL3[:dim]
    nidx = int(np.prod([k["N"] for k in kl]))
    uq = rng.normal(0, 1, 5) if coeffs != "stoch" else None
    stoch = rng.normal(0, 1, nidx) if coeffs != "uq" else None  # (with uq: terms 5 .. nidx-1, the rest dropped)
    data = rng.uniform(0.5, 2.0, m["nelem"]) if coeffs.endswith("data") else None
    x = _ip_points(oracle, m)
    klf = _kl_field(dim, x, kl, uq, stoch, fix)
    assert np.abs(klf).max() > 0.3  # the field clearly changes the matrix
    base = [1.3, 0.7, 2.1]
    kinv = [(1.0 / data[:, None] if data is not None else base[d]) / np.exp(klf[..., d]) for d in range(dim)]
    u = rng.uniform(-1, 1, m["ndof"])
    funcs = _funcs(dim)
    arrays = {"Kinv_" + "xyz"[d] * 2: ("array", np.ascontiguousarray(kinv[d])) for d in range(dim)}
    ref = oracle.assemble_block(m, oracle.PHYS_POROUS_MIXED, 2, u, want_local=True, funcs=dict(funcs, **arrays))
    blk = make_block(m, "porousMixed", 2, graph=(ref["rowptr"], ref["colind"]))
    for k, v in funcs.items():
        blk.set_function(k, v)
    for d in range(3):
        blk.set_function("Kinv_" + "xyz"[d] * 2, base[d])
    _set_kl(blk, kl, fix)
    if uq is not None:
        blk.set_parameter_vector("KLUQcoeffs", uq)
    if stoch is not None:
        blk.set_parameter_vector("KLStochcoeffs", stoch)
    if data is not None:
        blk.set_element_data(data)
        blk.set_physics_parameter("use permeability data", 1)
    got = _assemble_all(blk, m, u, len(ref["colind"]))
    for k in ("crs_vals", "crs_engine", "crs_local"):
        assert crs_err(got[k], ref) < RTOL, k
    for k in ("res", "res_only", "res_engine", "res_local"):
        assert rel_err(got[k], ref["res"]) < RTOL, k
    assert rel_err(got["local_J"], ref["local_J"]) < RTOL
    del torch


def test_mixed_permdata_gold_end_to_end(oracle):
    """regression/porous/Mixed_PermData (tests/golden/reference/porous_Mixed_PermData.*: input.yaml, perm.dat,
    perm_xy.dat, gold): 10x10 quads, HVOL0/HDIV1, quadrature 2, permeability from the data point nearest to each element
    centre, p = 1 weakly on all four sides; GPU volume and boundary assembly, one linear solve (the second Newton step of
    the deck changes nothing)."""
    torch = _torch()
    import mrhyde_amd
    import scipy.sparse.linalg as spla
    from test_oracle_multi import fmt, gold_errors
    dim, ncell, qdeg = 2, (10, 10), 2
    pts = np.loadtxt(os.path.join(GOLD, "porous_Mixed_PermData.perm_xy.dat"))
    vals_pts = np.loadtxt(os.path.join(GOLD, "porous_Mixed_PermData.perm.dat"))
    m = oracle.mesh_multi(dim, ncell, [oracle.HVOL, oracle.HDIV], [0, 1])
    blk = make_block(m, "porousMixed", qdeg)
    blk.set_function("source", ("sinprod", 8 * np.pi ** 2, [2 * np.pi] * 2))
    seed = blk.import_mesh_data(pts, vals_pts)
    centres = m["nodes"].mean(axis=1)
    d2 = ((centres[:, None, :] - pts[None]) ** 2).sum(-1)
    assert np.array_equal(seed, np.argmin(d2, axis=1))
    blk.set_physics_parameter("use permeability data", 1)
    for name in ("left", "right", "bottom", "top"):
        be, bs = oracle.boundary_sides(dim, ncell, name)
        blk.add_boundary_group(name, mrhyde_amd.BC_WEAK_DIRICHLET, be, bs)
        blk.set_function("Dirichlet p " + name, 1.0)
    rowptr, colind = blk.get_graph()
    ud = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    res = torch.empty(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.empty(len(colind), dtype=torch.float64, device="cuda")
    blk.assemble_jacres(ud, res, vals, overwrite=True)
    blk.assemble_boundary(ud, res, vals)
    torch.cuda.synchronize()
    J = sp.csr_matrix((vals.cpu().numpy(), colind, rowptr), shape=(m["ndof"],) * 2)
    u = spla.spsolve(J.tocsc(), res.cpu().numpy())
    pb = oracle.physical_basis_var(dim, oracle.HVOL, 0, qdeg, m["nodes"])
    ub = oracle.physical_basis_var(dim, oracle.HDIV, 1, qdeg, m["nodes"], m["orient"][:, m["varptr"][1]:])
    x, w = pb["ip"], pb["wts"]
    s, c = np.sin(2 * np.pi * x), np.cos(2 * np.pi * x)
    ep = np.sqrt(np.sum((u[m["lids"][:, m["offsets"][0]]][:, None] - 1.0 - np.prod(s, axis=-1)) ** 2 * w))
    uh = np.einsum("ef,efqd->eqd", u[m["lids"][:, m["offsets"][m["varptr"][1]:]]], ub["basis"])
    eu = np.sum((uh[..., 0] + 2 * np.pi * c[..., 0] * s[..., 1]) ** 2 * w) + \
        np.sum((uh[..., 1] + 2 * np.pi * s[..., 0] * c[..., 1]) ** 2 * w)
    g = gold_errors("porous_Mixed_PermData.gold")
    assert fmt(ep) == fmt(g["p"]) == "0.332462" and fmt(np.sqrt(eu)) == fmt(g["u"]) == "1.52868"


@pytest.mark.parametrize("option", ["data", "kl"])
def test_database_mode_declines(oracle, monkeypatch, option):
    """A uniform box, overwriting, 128-byte-aligned CRS values: database mode would run (porous_direct 2) with constant
    coefficients; with either option it declines (porous_direct 1) and equals the MHA_POROUS_DATABASE=0 result."""
    torch = _torch()
    rng = np.random.default_rng(5)
    dim, ncell = 3, (64, 2, 4)
    m = oracle.mesh_multi(dim, ncell, [oracle.HVOL, oracle.HDIV], [0, 1])
    u = rng.uniform(-1, 1, m["ndof"])
    data, coeffs = rng.uniform(0.5, 2.0, m["nelem"]), rng.normal(0, 1, 24)
    got = {}
    for db in (True, False):
        if db:
            monkeypatch.delenv("MHA_POROUS_DATABASE", raising=False)
        else:
            monkeypatch.setenv("MHA_POROUS_DATABASE", "0")
        blk = make_block(m, "porousMixed", 2)
        for k, v in _funcs(dim).items():
            blk.set_function(k, v)
        rowptr, colind = blk.get_graph()
        ud = torch.tensor(u, device="cuda")
        res = torch.full((m["ndof"],), 7.0, dtype=torch.float64, device="cuda")
        vals = torch.full((len(colind) + 16,), -3.0, dtype=torch.float64, device="cuda")
        v = vals[(-vals.data_ptr() % 128) // 8:][:len(colind)]
        assert v.data_ptr() % 128 == 0
        if db:
            blk.assemble_jacres(ud, res, v, overwrite=True)
            torch.cuda.synchronize()
            assert blk.info("porous_direct") == 2  # constant coefficients: the database mode runs
        if option == "data":
            blk.set_element_data(data)
            blk.set_physics_parameter("use permeability data", 1)
        else:
            _set_kl(blk, KL3, 1)
            blk.set_parameter_vector("KLStochcoeffs", coeffs)
        blk.assemble_jacres(ud, res, v, overwrite=True)
        torch.cuda.synchronize()
        assert blk.info("porous_direct") == 1
        got[db] = (res.cpu().numpy(), v.cpu().numpy())
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(got[True][1], got[False][1])


def test_coefficient_update_between_assemblies(oracle):
    """Changing KLStochcoeffs between two assemblies, with no other call: the second result equals a fresh block's."""
    torch = _torch()
    rng = np.random.default_rng(17)
    dim = 3
    m = warp(oracle.mesh_multi(dim, (4, 3, 3), [oracle.HVOL, oracle.HDIV], [0, 1]))
    u = rng.uniform(-1, 1, m["ndof"])
    c1, c2 = rng.normal(0, 1, 24), rng.normal(0, 1, 24)

    def block(coeffs):
        blk = make_block(m, "porousMixed", 2)
        for k, v in _funcs(dim).items():
            blk.set_function(k, v)
        _set_kl(blk, KL3, 0)
        blk.set_parameter_vector("KLStochcoeffs", coeffs)
        return blk

    def run(blk):
        rowptr, colind = blk.get_graph()
        res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
        vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
        blk.assemble_jacres(torch.tensor(u, device="cuda"), res, vals, overwrite=True)
        return res, vals  # (not synchronised: the next call must order itself after this assembly)

    blk = block(c1)
    r1, v1 = run(blk)
    blk.set_parameter_vector("KLStochcoeffs", c2)
    r2, v2 = run(blk)
    torch.cuda.synchronize()
    fr, fv = run(block(c2))
    torch.cuda.synchronize()
    assert np.array_equal(r2.cpu().numpy(), fr.cpu().numpy()) and np.array_equal(v2.cpu().numpy(), fv.cpu().numpy())
    assert rel_err(v1.cpu().numpy(), fv.cpu().numpy()) > 1e-3


def test_refusals_on_a_block(oracle):
    _torch()
    import mrhyde_amd
    torch = _torch()
    m = oracle.mesh_multi(2, (3, 2), [oracle.HVOL, oracle.HDIV], [0, 1])
    blk = make_block(m, "porousMixed", 2)
    rowptr, colind = blk.get_graph()
    ud = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    res = torch.zeros(m["ndof"], dtype=torch.float64, device="cuda")
    vals = torch.zeros(len(colind), dtype=torch.float64, device="cuda")
    blk.set_physics_parameter("use permeability data", 1)
    with pytest.raises(mrhyde_amd.MhaError) as e:  # no element data
        blk.assemble_jacres(ud, res, vals, overwrite=True)
    assert e.value.code == 2  # MHA_ERR_STATE
    with pytest.raises(mrhyde_amd.MhaError):
        blk.set_element_data(np.zeros((m["nelem"], 0)))  # ncols < 1
    for bad in (0.0, np.inf, np.nan):
        d = np.ones(m["nelem"])
        d[3] = bad
        with pytest.raises(mrhyde_amd.MhaError, match="zero or not finite"):
            blk.set_element_data(d)
    blk.set_physics_parameter("use permeability data", 0)
    with pytest.raises(mrhyde_amd.MhaError):
        blk.set_physics_parameter("KL N x", mrhyde_amd.KL_MAX_TERMS + 1)
    with pytest.raises(mrhyde_amd.MhaError):
        blk.set_parameter_vector("KLcoeffs", np.ones(3))
    blk.set_physics_parameter("use KL expansion", 1)
    blk.set_physics_parameter("KL N x", 2)
    blk.set_physics_parameter("KL L x", 1.0)
    blk.set_physics_parameter("KL sigma x", 1.0)
    blk.set_physics_parameter("KL eta x", 0.1)
    with pytest.raises(mrhyde_amd.MhaError, match="KL N y"):  # y direction missing
        blk.assemble_jacres(ud, res, vals, overwrite=True)
    for key, v in (("N", 2), ("L", 0.001), ("sigma", 1.0), ("eta", 0.1)):
        blk.set_physics_parameter("KL %s y" % key, v)
    with pytest.raises(mrhyde_amd.MhaError, match="roots"):  # fewer than N roots
        blk.assemble_jacres(ud, res, vals, overwrite=True)
    blk.set_physics_parameter("KL L y", 1.0)
    blk.assemble_jacres(ud, res, vals, overwrite=True)
    torch.cuda.synchronize()
    thermal = mrhyde_amd.Block(2, 1, quadrature=2)
    tm = mrhyde_amd.mesh_structured(2, 1, (2, 2))
    thermal.set_mesh(tm["nodes"], tm["lids"], tm["offsets"], tm["ndof"], tm["boundary"])
    with pytest.raises(mrhyde_amd.MhaError):
        thermal.set_parameter_vector("KLUQcoeffs", np.ones(2))
