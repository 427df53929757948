"""Seeded cases and the checks of raincast_gnn.pool against tests/pool_oracle.py and the
mpmath fixture tests/golden/pool_crps_rows.npz, shared by the CPU tests (the package's torch
path) and the GPU tests (the kernels of csrc/gine_pool.hip): the same properties at the same
bounds on either device.

Members: ``forecast_cases.make_params(kind, n, seed=m)`` for member ``m``.

Bounds:
  Fbar               1e-13 absolute; sfbar 1e-11 relative where the oracle is >= 1e-300
                     (forecast_cases' bounds: a convex combination of values that each meet
                     them); exactly 0 and 1 below c
  quantiles          in probability space through the oracle: |Fbar(Q(q)) - q| <= 1e-12 outside
                     a 1e-12 band around the pooled atom, |sfbar(Q(s)) - s| <= 1e-10 s for s
                     from 1e-12 to 0.5; c bitwise on the atom; the edge levels; per-row levels
                     [N, T] give the bits of shared levels [T]
  CRPS               the fixture's rows within 1e-11 x the largest |row| of their case;
                     crps_rows == member_crps_rows - diversity_rows exactly; member_crps_rows
                     1e-12 of max_row |oracle| (the members' closed forms)
  PIT, Brier         1e-13 absolute; count exact
"""
import os

import numpy as np
import torch

import forecast_cases as FC
from conftest import GOLDEN
from pool_oracle import PoolDist
from raincast_gnn.forecast import Forecast
from raincast_gnn.pool import ForecastPool

KIND_XI = FC.KIND_XI


def members(kind, n, M):
    """[M, n, K] float32: member m is make_params(kind, n, seed=m)."""
    return np.stack([FC.make_params(kind, n, seed=m) for m in range(M)])


def build(kind, xi, params, device, weights=None):
    u = FC.U_FIXED if kind == "mixed" else None
    pool = ForecastPool(torch.from_numpy(params).to(device), kind, u=u, xi=xi, weights=weights)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    orc = PoolDist(kind, params.astype(np.float64), u=u, xi=xi,
                   weights=None if w is None else w / w.sum())
    return pool, orc


def thresholds(kind, params, T):
    return FC.thresholds(kind, params[0], T)


def _np(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    """Equal bits wherever a value is held, NaN in the same places."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and \
        torch.equal(bits(a)[~na], bits(b)[~nb])


check_prob = FC.check_prob


def check_quantile(pool, orc, Q):
    """forecast_cases' quantile checks on the pool, the edge levels, and per-row levels."""
    err = FC.check_quantile(pool, orc, Q)
    FC.check_edge_levels(pool, orc)
    n = pool.preds.size(1)
    for upper in (False, True):
        lv = np.concatenate([np.linspace(0.001, 0.999, Q), [0.0, 1.0]]) if not upper else \
            np.concatenate([np.logspace(-12, np.log10(0.5), Q), [0.0, 1.0]])
        f = pool.return_level if upper else pool.quantile
        shared = f(lv)
        per_row = f(torch.from_numpy(np.tile(lv, (n, 1))).to(pool.preds.device))
        assert same_bits(shared, per_row)
    return err


def check_score(pool, orc, y, x):
    """-> worst errors (member crps / scale, pit, brier) against the oracle."""
    sc = pool.score(torch.from_numpy(y).to(pool.preds.device), x)
    ok = ~np.isnan(y)
    crps, mem, div = _np(sc.crps_rows), _np(sc.member_crps_rows), _np(sc.diversity_rows)
    lo, hi = _np(sc.pit_lo), _np(sc.pit_hi)
    for a in (crps, mem, lo, hi):
        assert np.all(np.isnan(a[~ok])) and not np.isnan(a[ok]).any()
    assert np.all(div >= 0.0)                               # NaN targets included
    assert np.array_equal(crps[ok], mem[ok] - div[ok])
    ref = orc.member_crps_rows(y.astype(np.float64))
    scale = np.abs(ref[ok]).max() if ok.any() else 1.0
    err_c = float(np.abs(mem - ref)[ok].max() / scale) if ok.any() else 0.0
    plo, phi = orc.pit(y)
    err_p = float(max(np.abs(lo - plo)[ok].max(), np.abs(hi - phi)[ok].max())) if ok.any() else 0.0
    bo, cnt = orc.brier(y, x)
    brier = _np(sc.brier)
    assert float(_np(sc.valid)[0]) == cnt
    if cnt == 0:
        assert np.all(np.isnan(brier))
        err_b = 0.0
    else:
        err_b = float(np.abs(brier - bo).max()) if len(x) else 0.0
    assert err_c <= 1e-12, err_c
    assert err_p <= 1e-13, err_p
    assert err_b <= 1e-13, err_b
    if orc.atom and ok.any():
        at = ok & (y.astype(np.float64) <= orc.c)
        assert np.all(lo[at] == 0.0) and np.all(lo[ok & ~at] == hi[ok & ~at])
    return err_c, err_p, err_b


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(GOLDEN, "pool_crps_rows.npz"))
    return _fixture


def check_fixture(device):
    """Every case of the mpmath fixture -> the worst |crps - reference| / max |reference of
    the case|, asserted <= 1e-11.  One score call per case: row i at each of the case's y."""
    fx = fixture()
    worst = 0.0
    for name, kind, xi in zip(fx["names"], fx["kinds"], fx["xis"]):
        name, kind = str(name), str(kind)
        xi = None if np.isnan(xi) else float(xi)
        params, ys, ref = fx[f"{name}_params"], fx[f"{name}_y"], fx[f"{name}_crps"]
        rows, J = ref.shape
        assert np.all(ys >= FC.C) and np.all(ys == ys.astype(np.float32))
        tiled = np.repeat(params, J, axis=1)                 # row i, y j -> i * J + j
        y = np.tile(ys, rows).astype(np.float32)
        pool, _ = build(kind, xi, tiled, device)
        sc = pool.score(torch.from_numpy(y).to(device))
        got = _np(sc.crps_rows).reshape(rows, J)
        div = _np(sc.diversity_rows).reshape(rows, J)
        assert np.all(div == div[:, :1])                     # V depends on no target
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"  fixture {name}: {err:.2e} of max |row|")
        worst = max(worst, err)
    assert worst <= 1e-11, worst
    return worst


def check_copies(kind, xi, n, copies, device):
    """A pool of `copies` copies of one member (default weights): Forecast's bits everywhere,
    and a diversity of exactly 0."""
    params = FC.make_params(kind, n, seed=3)
    u = FC.U_FIXED if kind == "mixed" else None
    one = torch.from_numpy(params).to(device)
    fc = Forecast(one, kind, u=u, xi=xi)
    pool = ForecastPool(torch.stack([one] * copies), kind, u=u, xi=xi)
    x = FC.thresholds(kind, params, 7)
    q = np.concatenate([np.linspace(0.001, 0.999, 9), [0.0, 1.0, np.nan, -0.1, 1.5]])
    s = np.concatenate([np.logspace(-12, np.log10(0.5), 9), [0.0, 1.0, np.nan, -0.1, 1.5]])
    assert same_bits(pool.cdf(x), fc.cdf(x))
    assert same_bits(pool.exceedance(x), fc.exceedance(x))
    assert same_bits(pool.quantile(q), fc.quantile(q))
    assert same_bits(pool.return_level(s), fc.return_level(s))
    assert same_bits(pool.return_level(s, unit="mm"), fc.return_level(s, unit="mm"))
    y = torch.from_numpy(FC.make_targets(n, seed=4)).to(device)
    a, b = pool.score(y, x), fc.score(y, x)
    for name in ("crps_rows", "pit_lo", "pit_hi", "brier", "valid"):
        assert same_bits(getattr(a, name), getattr(b, name)), name
    assert same_bits(a.member_crps_rows, b.crps_rows)
    assert torch.all(a.diversity_rows == 0.0)


def check_weights(kind, xi, device):
    """Non-uniform weights against the oracle; unnormalised weights are normalised; zero,
    negative, non-finite or wrong-length weights raise."""
    import pytest
    n, M = 9, 3
    params = members(kind, n, M)
    x = thresholds(kind, params, 7)
    y = FC.make_targets(n, seed=5)
    pool, orc = build(kind, xi, params, device, weights=[0.5, 0.3, 0.2])
    check_prob(pool, orc, x)
    check_quantile(pool, orc, 5)
    check_score(pool, orc, y, x)
    scaled, _ = build(kind, xi, params, device, weights=[5.0, 3.0, 2.0])
    assert abs(float(scaled.weights.sum()) - 1.0) <= 1e-15
    assert same_bits(scaled.exceedance(x), pool.exceedance(x))
    t = torch.from_numpy(params).to(device)
    u = FC.U_FIXED if kind == "mixed" else None
    for bad in ([0.5, 0.5, 0.0], [0.7, 0.5, -0.2], [0.5, 0.5], [0.5, 0.5, float("nan")],
                [0.5, 0.5, float("inf")]):
        with pytest.raises(ValueError):
            ForecastPool(t, kind, u=u, xi=xi, weights=bad)
