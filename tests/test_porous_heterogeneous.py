"""Host-only tools of porousMixed's heterogeneous permeability (no GPU): the 1-D Karhunen-Loeve expansions against a
numpy restatement of klexpansion::computeRoots (tools/klexpansion.hpp:38-125), the total order of the multi-indices
(porousMixed.cpp:73-118), the exact nearest-point search of mesh-data import against brute force (tools/data.cpp:391-420)
and the refusals of these entry points."""
import numpy as np
import pytest

import mrhyde_amd
from mrhyde_amd import MhaError


def np_kl_roots(N, L, sigma, eta):
    """numpy restatement of computeRoots: scan from 1 in steps of 1, at most 10 Newton steps, duplicates within 1e-6."""
    f = lambda w: (eta * eta * w * w - 1.0) * np.sin(w * L) - 2.0 * eta * w * np.cos(w * L)
    df = lambda w: (2.0 * w * eta * eta * np.sin(w * L) + (eta * eta * w * w - 1.0) * L * np.cos(w * L)
                    - 2.0 * eta * np.cos(w * L) + 2.0 * eta * w * L * np.sin(w * L))
    roots, ig, fprev, it = [], 1.0, f(1.0), 0
    while len(roots) < N and it < 1000:
        it += 1
        ig += 1.0
        w, fw = ig, f(ig)
        if fw * fprev < 0:
            fprev = fw
            nl = 0
            while abs(fw) > 1e-10 and nl < 10:
                nl += 1
                w = w - fw / df(w)
                fw = f(w)
            if all(abs(w - r) >= 1e-6 for r in roots):
                roots.append(w)
    om = np.array(roots)
    return om, 2.0 * eta * sigma * sigma / (eta * eta * om * om + 1.0)


def np_kl_indices(dim, N):
    out = []
    nz = N[2] if dim == 3 else 1
    for a in range(sum(N[:dim]) + (1 if dim == 2 else 0)):
        for k in range(nz):
            for j in range(N[1]):
                for i in range(N[0]):
                    if i + j + k == a:
                        out.append([i, j, k][:dim])
    return np.array(out)


def test_kl_expansion_check_values():
    om, lam = mrhyde_amd.kl_expansion(4, 1.0, 0.1, 0.1)
    np.testing.assert_allclose(om, [2.62767543, 5.3073248, 8.06713558, 10.90870751], rtol=0, atol=5e-8)
    np.testing.assert_allclose(lam, [1.87083e-3, 1.56046e-3, 1.21154e-3, 9.1324e-4], rtol=5e-6)


@pytest.mark.parametrize("N,L,sigma,eta", [(4, 1.0, 0.1, 0.1), (8, 1.0, 1.0, 0.3), (3, 2.5, 0.7, 0.05), (6, 0.7, 2.0, 1.5),
                                           (1, 1.0, 1.0, 0.1), (5, 3.0, 0.2, 0.02)])
def test_kl_expansion_vs_restatement(N, L, sigma, eta):
    om, lam = mrhyde_amd.kl_expansion(N, L, sigma, eta)
    rom, rlam = np_kl_roots(N, L, sigma, eta)
    assert len(rom) == N
    np.testing.assert_allclose(om, rom, rtol=1e-14, atol=0)
    np.testing.assert_allclose(lam, rlam, rtol=1e-14, atol=0)
    f = (eta * eta * om * om - 1.0) * np.sin(om * L) - 2.0 * eta * om * np.cos(om * L)
    # (like the reference, Newton may land on a negative root: omega and -omega give the same lambda and -phi)
    assert np.all(np.abs(f) < 1e-8)


@pytest.mark.parametrize("dim,N", [(2, (3, 2)), (2, (1, 4)), (2, (4, 4)), (3, (2, 3, 2)), (3, (4, 1, 3)), (3, (4, 4, 4))])
def test_kl_indices_total_order(dim, N):
    idx = mrhyde_amd.kl_indices(dim, list(N))
    ref = np_kl_indices(dim, N)
    assert idx.shape == (int(np.prod(N[:dim])), dim)
    assert np.array_equal(idx, ref)
    # total order by alpha, then z, then y, then x
    key = [tuple([r.sum()] + list(r[::-1])) for r in idx]
    assert key == sorted(key)


def _brute(q, p):
    d = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return np.argmin(d, axis=1)  # first (lowest) index among equal minima


@pytest.mark.parametrize("dim", [2, 3])
def test_closest_points_vs_brute_force(dim):
    rng = np.random.default_rng(7 + dim)
    p = rng.uniform(-1, 2, (700, dim))
    q = np.concatenate([rng.uniform(-1.5, 2.5, (900, dim)), p[:50] + 1e-13, p[50:60]])
    assert np.array_equal(mrhyde_amd.closest_points(q, p), _brute(q, p))
    # clustered points and far queries
    p2 = np.concatenate([rng.normal(0, 0.01, (300, dim)), rng.normal(5, 1, (20, dim))])
    q2 = rng.uniform(-10, 10, (400, dim))
    assert np.array_equal(mrhyde_amd.closest_points(q2, p2), _brute(q2, p2))


@pytest.mark.parametrize("dim", [2, 3])
def test_closest_points_ties_to_lowest_index(dim):
    # a lattice with every query equidistant from several lattice points, and duplicated points
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * dim, indexing="ij"), -1).reshape(-1, dim)
    p = np.concatenate([g[::-1], g])  # each location twice, the higher copy first
    q = np.concatenate([g, g + 0.5, np.full((1, dim), 1.5)])
    idx = mrhyde_amd.closest_points(q, p)
    assert np.array_equal(idx, _brute(q, p))
    # the exact lattice points resolve to the first listed copy
    assert np.array_equal(idx[:len(g)], len(g) - 1 - np.arange(len(g)))


def test_closest_points_degenerate_layouts():
    p = np.array([[0.5, 0.5]] * 3 + [[0.5, 0.7]])
    q = np.array([[0.5, 0.0], [0.5, 0.65], [3.0, 0.6]])
    assert mrhyde_amd.closest_points(q, p).tolist() == _brute(q, p).tolist() == [0, 3, 0]  # (the last query is equidistant)
    line = np.stack([np.linspace(0, 1, 11), np.zeros(11), np.zeros(11)], 1)
    q3 = np.random.default_rng(1).uniform(-1, 2, (50, 3))
    assert np.array_equal(mrhyde_amd.closest_points(q3, line), _brute(q3, line))


def test_refusals():
    with pytest.raises(MhaError):
        mrhyde_amd.kl_expansion(mrhyde_amd.KL_MAX_TERMS + 1, 1.0, 1.0, 0.1)  # above the kernels' cap
    with pytest.raises(MhaError):
        mrhyde_amd.kl_expansion(0, 1.0, 1.0, 0.1)
    with pytest.raises(MhaError, match="roots"):
        mrhyde_amd.kl_expansion(4, 0.001, 1.0, 0.1)  # roots ~ pi / L apart: fewer than N within 1000 steps
    with pytest.raises(MhaError):
        mrhyde_amd.kl_expansion(4, -1.0, 1.0, 0.1)
    with pytest.raises(MhaError):
        mrhyde_amd.kl_expansion(4, 1.0, 1.0, 0.0)
    with pytest.raises(MhaError):
        mrhyde_amd.kl_indices(1, [3])
    with pytest.raises(MhaError):
        mrhyde_amd.kl_indices(2, [0, 2])
    with pytest.raises(MhaError):
        mrhyde_amd.closest_points(np.zeros((3, 2)), np.zeros((0, 2)))
    with pytest.raises(MhaError):
        mrhyde_amd.closest_points(np.zeros((1, 2)), np.array([[0.0, np.nan]]))
