"""Seeded cases and the checks of ``ForecastPool.pair_sums`` / ``fit_weights``,
shared by the CPU tests (the package's torch path, tests/test_pool_fit.py) and the GPU tests
(the kernel ``gine_pool_pairs``, tests/test_gpu_pool_fit.py): the same properties at the same
bounds on either device.

Members and targets as tests/pool_cases.py: member ``m`` is ``forecast_cases.make_params(kind,
n, seed=m)``, targets ``forecast_cases.make_targets`` (about 5 % NaN).

Bounds:
  fixture      distance of one-row segments against tests/golden/pool_pair_rows.npz (mpmath, the
               direct integrals with the pair's own breakpoints): 1e-11 x the case's largest
               entry, the project's bound for this rule
  identity     sum of ForecastPool(weights=w).score(y).crps_rows over the valid rows against
               c . w - 1/2 w' D w: 1e-11 x count x the largest |crps row|; the same for
               member_crps_rows against c . w and diversity_rows against 1/2 w' D w
  exact        equal members: distance exactly 0; zero diagonal; distance == its transpose;
               permuted members give the permuted arrays bit for bit; a segment's sums are
               those of its row slice alone bit for bit; two calls give the same bits
  segments     count exact; the segments added in order against the single segment: (n - 1)
               2^-52 relative (n rows; sums of non-negative row values in two groupings, each
               within (n - 1) 2^-53 of the exact sum)
"""
import os

import numpy as np
import torch

import forecast_cases as FC
import pool_cases as PC
from conftest import GOLDEN
from raincast_gnn.pool import ForecastPool

KIND_XI = FC.KIND_XI
same_bits = PC.same_bits


def _np(t):
    return t.detach().cpu().numpy()


def make_pool(kind, xi, params, device, weights=None):
    u = FC.U_FIXED if kind == "mixed" else None
    return ForecastPool(torch.from_numpy(np.ascontiguousarray(params)).to(device), kind, u=u,
                        xi=xi, weights=weights)


def sums(pool, y, folds=None):
    return pool.pair_sums(torch.from_numpy(y), folds)


def weight_vectors(M):
    """1 / M, a seeded non-uniform vector, 0.97 on one member."""
    r = np.random.default_rng(40 + M)
    v = r.random(M) + 0.1
    out = [np.full(M, 1.0 / M), v / v.sum()]
    if M > 1:
        w = np.full(M, 0.03 / (M - 1))
        w[M // 2] = 0.97
        out.append(w)
    return out


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(GOLDEN, "pool_pair_rows.npz"))
    return _fixture


def check_fixture(device):
    """One row per segment, every target valid: distance[g] is row g's pair integrals -> the
    worst error / the case's largest entry, asserted <= 1e-11."""
    fx = fixture()
    worst = 0.0
    for name, kind, xi in zip(fx["names"], fx["kinds"], fx["xis"]):
        name, kind = str(name), str(kind)
        xi = None if np.isnan(xi) else float(xi)
        params, ref = fx[f"{name}_params"], fx[f"{name}_pairs"]
        M, rows = params.shape[0], params.shape[1]
        pool = make_pool(kind, xi, params, device)
        ps = sums(pool, np.zeros(rows, dtype=np.float32), np.arange(rows + 1))
        D = _np(ps.distance)
        assert np.array_equal(_np(ps.count), np.ones(rows))
        got = np.stack([D[:, m, l] for m in range(M) for l in range(m + 1, M)], 1)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"  fixture {name}: {err:.2e} of the largest entry")
        worst = max(worst, err)
    assert worst <= 1e-11, worst
    return worst


def check_identity(kind, xi, n, M, device):
    """-> the worst of the three errors / (count x largest |crps row|), asserted <= 1e-11."""
    params = PC.members(kind, n, M)
    y = FC.make_targets(n, seed=M)
    ok = ~np.isnan(y)
    ps = sums(make_pool(kind, xi, params, device), y)
    count = float(_np(ps.count)[0])
    assert count == ok.sum()
    c, D = _np(ps.member_crps)[0], _np(ps.distance)[0]
    worst = 0.0
    for w in weight_vectors(M):
        weighted = make_pool(kind, xi, params, device, weights=w)
        sc = weighted.score(torch.from_numpy(y))
        w = _np(weighted.weights)                            # as the pool normalised them
        crps, mem, div = _np(sc.crps_rows)[ok], _np(sc.member_crps_rows)[ok], \
            _np(sc.diversity_rows)[ok]
        if count == 0:
            assert not c.any() and not D.any()
            continue
        scale = count * np.abs(crps).max()
        quad = 0.5 * (w @ (D @ w))
        errs = (abs(crps.sum() - (c @ w - quad)), abs(mem.sum() - c @ w), abs(div.sum() - quad))
        worst = max(worst, max(errs) / scale)
    assert worst <= 1e-11, worst
    return worst


def check_zeros_and_symmetry(kind, xi, n, M, device):
    """Equal members, the diagonal, the transpose, and a seeded permutation of the members."""
    params = PC.members(kind, n, M)
    y = FC.make_targets(n, seed=11)
    ps = sums(make_pool(kind, xi, params, device), y, 2)
    D = ps.distance
    assert ps.count.dtype == ps.member_crps.dtype == D.dtype == torch.float64
    assert D.shape == (2, M, M) and ps.member_crps.shape == (2, M) and ps.count.shape == (2,)
    assert torch.all(torch.diagonal(D, dim1=1, dim2=2) == 0.0)
    assert same_bits(D, D.transpose(1, 2).contiguous())
    assert torch.all(D >= 0.0)
    if M >= 3:
        twin = params.copy()
        twin[2] = twin[0]
        pt = sums(make_pool(kind, xi, twin, device), y, 2)
        assert torch.all(pt.distance[:, 0, 2] == 0.0) and torch.all(pt.distance[:, 2, 0] == 0.0)
        assert same_bits(pt.distance[:, 0, 1].contiguous(), pt.distance[:, 2, 1].contiguous())
        assert same_bits(pt.member_crps[:, 0].contiguous(), pt.member_crps[:, 2].contiguous())
    perm = np.random.default_rng(5 + M).permutation(M)
    pp = sums(make_pool(kind, xi, params[perm], device), y, 2)
    idx = torch.from_numpy(perm).to(D.device)
    assert same_bits(pp.count, ps.count)
    assert same_bits(pp.member_crps, ps.member_crps[:, idx].contiguous())
    assert same_bits(pp.distance, D[:, idx][:, :, idx].contiguous())


def segment_ptr(n):
    """An empty segment, a one-row segment, a boundary at row 65 (no tile multiple)."""
    return np.minimum(np.array([0, 0, 1, 65, n], dtype=np.int64), n)


def check_segments(kind, xi, n, M, device):
    """-> the worst relative difference of the segments added in order against one segment."""
    params = PC.members(kind, n, M)
    y = FC.make_targets(n, seed=12)
    ok = ~np.isnan(y)
    ptr = segment_ptr(n)
    pool = make_pool(kind, xi, params, device)
    ps = sums(pool, y, ptr)
    for form in (list(int(v) for v in ptr), torch.from_numpy(ptr)):
        other = sums(pool, y, form)
        assert same_bits(other.distance, ps.distance) and same_bits(other.count, ps.count)
    G = ptr.size - 1
    assert ps.distance.shape == (G, M, M)
    for g in range(G):
        a, b = int(ptr[g]), int(ptr[g + 1])
        assert float(ps.count[g]) == ok[a:b].sum()
        alone = sums(make_pool(kind, xi, params[:, a:b], device), y[a:b])
        assert same_bits(alone.count, ps.count[g:g + 1])
        assert same_bits(alone.member_crps[0], ps.member_crps[g].contiguous())
        assert same_bits(alone.distance[0], ps.distance[g].contiguous())
    one = sums(pool, y)
    worst = 0.0
    for name in ("member_crps", "distance"):
        parts, whole = _np(getattr(ps, name)), _np(getattr(one, name))[0]
        total = np.zeros_like(whole)
        for g in range(G):
            total = total + parts[g]
        nz = whole != 0.0
        assert np.all(total[~nz] == 0.0)
        if nz.any():
            worst = max(worst, float((np.abs(total - whole)[nz] / np.abs(whole)[nz]).max()))
    assert float(one.count[0]) == ok.sum() == float(ps.count.sum())
    assert worst <= max(n - 1, 0) * 2.0 ** -52, worst
    k = sums(pool, y, 3)                                     # K blocks of ceil(n / K) rows
    size = -(-n // 3)
    want = sums(pool, y, np.minimum(np.arange(4) * size, n))
    assert same_bits(k.distance, want.distance) and same_bits(k.member_crps, want.member_crps)
    return worst


def check_missing(kind, xi, n, M, device):
    """All targets NaN: zero counts and zero sums; fit_weights raises."""
    import pytest
    pool = make_pool(kind, xi, PC.members(kind, n, M), device)
    y = np.full(n, np.nan, dtype=np.float32)
    ps = sums(pool, y, segment_ptr(n))
    for t in (ps.count, ps.member_crps, ps.distance):
        assert torch.all(t == 0.0)
    with pytest.raises(ValueError):
        pool.fit_weights(torch.from_numpy(y))
    with pytest.raises(ValueError):
        pool.fit_weights(torch.from_numpy(y), folds=2)


def check_determinism(kind, xi, n, M, device):
    """Two calls: the same bits; a third after a score call in between as well."""
    pool = make_pool(kind, xi, PC.members(kind, n, M), device)
    y = FC.make_targets(n, seed=13)
    ptr = segment_ptr(n)
    a, b = sums(pool, y, ptr), sums(pool, y, ptr)
    pool.score(torch.from_numpy(y), [0.0, 1.0])
    third = sums(pool, y, ptr)
    for other in (b, third):
        for name in ("count", "member_crps", "distance"):
            assert same_bits(getattr(a, name), getattr(other, name)), name
