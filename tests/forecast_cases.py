"""Seeded cases and the checks of raincast_gnn.forecast against tests/forecast_oracle.py,
shared by the CPU tests (the package's torch path) and the GPU tests (the kernels): the same
properties at the same bounds on either device.

Bounds (fp64 results; z = (x - mu) / sigma is formed by the same three roundings on both sides):
  F                  1e-13 absolute
  P(Y > x)           1e-11 relative where the oracle's value is >= 1e-300: erfc's conditioning
                     in z is about z^2 + 1 <= 1.5e3 before underflow, times a few ulp of
                     erfc / pow (1/xi <= 5): under 1e-12
  quantile           in probability space, through the oracle: |F(Q(q)) - q| <= 1e-12 outside
                     the atom, |sf(Q(s)) - s| <= 1e-10 s for the upper form; atoms and edge
                     levels exactly
  CRPS rows          1e-12 of max_row |oracle|; PIT and Brier 1e-13 absolute; count exact
"""
import numpy as np
import torch

from forecast_oracle import C, Dist
from raincast_gnn.forecast import Forecast

U_FIXED = float(np.float32(1.71))
# (kind, xi): every kind, and the tail shapes around the experiments' 0.5
KIND_XI = [("normal", None), ("mixed_normal", None)] + \
          [(k, xi) for k in ("mixed", "mixed_u") for xi in (0.2, 0.5, 0.8)]
WIDTH = {"normal": 2, "mixed_normal": 3, "mixed": 4, "mixed_u": 5}
C_F32 = float(np.float32(C))  # what a dataset's fp32 target holds at 0 mm


def _softplus(v):
    return np.log1p(np.exp(v)) + 1e-6


def make_params(kind, n, seed=0):
    """[n, K] float32 rows in the ranges PostProcess produces."""
    r = np.random.default_rng(1000 * seed + n)
    cols = [r.normal(-1.0, 2.0, n), _softplus(r.normal(0, 1, n)),
            1 / (1 + np.exp(-r.normal(0, 1, n))), _softplus(r.normal(0, 1, n)),
            2.12 / (1 + np.exp(-r.normal(0, 1, n)))]
    return np.stack(cols[:WIDTH[kind]], axis=1).astype(np.float32)


def make_targets(n, seed=0):
    """float32 targets: about half at 0 mm, about 5 % missing."""
    r = np.random.default_rng(77 + 1000 * seed + n)
    y = np.where(r.random(n) < 0.5, C_F32, np.maximum(r.normal(0.5, 1.5, n), -4.0))
    y = y.astype(np.float32)
    y[r.random(n) < 0.05] = np.nan
    return y


def build(kind, xi, params, device):
    u = U_FIXED if kind == "mixed" else None
    fc = Forecast(torch.from_numpy(params).to(device), kind, u=u, xi=xi)
    return fc, Dist(kind, params.astype(np.float64), u=u, xi=xi)


def thresholds(kind, params, T):
    """Below c, exactly c, exactly u, u + 50 sigma_u, then a grid over body and tail."""
    u = float(params[0, 4]) if kind == "mixed_u" else U_FIXED
    su = float(params[0, 3]) if params.shape[1] > 3 else 1.0
    special = [C, C - 1.0, u, u + 50.0 * su, float(np.nextafter(C, -np.inf))]
    grid = np.linspace(-6.0, 12.0, 28)
    return np.array((special + list(grid))[:T], dtype=np.float64)


def _np(t):
    return t.detach().cpu().numpy()


def check_prob(fc, orc, x):
    """-> (worst |F - F_oracle|, worst relative error of the upper form)."""
    F, S = _np(fc.cdf(x)), _np(fc.exceedance(x))
    Fo, So = orc.cdf(x), orc.sf(x)
    assert F.shape == Fo.shape == S.shape
    err_f = float(np.abs(F - Fo).max())
    big = So >= 1e-300
    err_s = float((np.abs(S - So)[big] / So[big]).max()) if big.any() else 0.0
    assert err_f <= 1e-13, err_f
    assert err_s <= 1e-11, err_s
    assert np.all(S[~big] <= 1e-299)
    below = x < orc.c
    if orc.atom and below.any():
        assert np.all(F[:, below] == 0.0) and np.all(S[:, below] == 1.0)
    return err_f, err_s


def check_quantile(fc, orc, Q):
    """-> (worst |F(Q(q)) - q|, worst |sf(Q(s)) - s| / s)."""
    q = np.linspace(0.001, 0.999, Q) if Q > 1 else np.array([0.9])
    x = _np(fc.quantile(q))
    qq = np.broadcast_to(q[None, :], x.shape)
    if orc.atom:
        at = qq <= orc.P_c * (1 - 1e-12)
        assert np.all(x[at] == orc.c)                       # bitwise c on the atom
        free = qq > orc.P_c * (1 + 1e-12)
    else:
        free = np.ones_like(qq, dtype=bool)
    err_q = float(np.abs(orc.cdf(x) - qq)[free].max()) if free.any() else 0.0
    assert err_q <= 1e-12, err_q
    s = np.logspace(-12, np.log10(0.5), Q) if Q > 1 else np.array([1e-12])
    xs = _np(fc.return_level(s))
    ss = np.broadcast_to(s[None, :], xs.shape)
    if orc.atom:
        at = ss >= orc.S_c * (1 + 1e-12)
        assert np.all(xs[at] == orc.c)
        free = ss < orc.S_c * (1 - 1e-12)
    else:
        free = np.ones_like(ss, dtype=bool)
    err_s = float((np.abs(orc.sf(xs) - ss) / ss)[free].max()) if free.any() else 0.0
    assert err_s <= 1e-10, err_s
    return err_q, err_s


def check_edge_levels(fc, orc):
    lv = np.array([0.0, 1.0, np.nan, -0.1, 1.5])
    for upper in (False, True):
        x = _np(fc.return_level(lv) if upper else fc.quantile(lv))
        lo, hi = (1, 0) if upper else (0, 1)
        assert np.all(x[:, lo] == (orc.c if orc.atom else -np.inf))
        assert np.all(x[:, hi] == np.inf)
        assert np.all(np.isnan(x[:, 2:]))


def check_score(fc, orc, y, x):
    """-> worst errors (crps / scale, pit, brier) against the oracle."""
    sc = fc.score(torch.from_numpy(y).to(fc.pred.device), x)
    ok = ~np.isnan(y)
    crps, lo, hi = _np(sc.crps_rows), _np(sc.pit_lo), _np(sc.pit_hi)
    for a in (crps, lo, hi):
        assert np.all(np.isnan(a[~ok])) and not np.isnan(a[ok]).any()
    ref = orc.crps_rows(y.astype(np.float64))
    scale = np.abs(ref[ok]).max() if ok.any() else 1.0
    err_c = float(np.abs(crps - ref)[ok].max() / scale) if ok.any() else 0.0
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
    if orc.atom and ok.any():  # the PIT is an interval only at the atom
        at = ok & (y.astype(np.float64) <= orc.c)
        assert np.all(lo[at] == 0.0) and np.all(lo[ok & ~at] == hi[ok & ~at])
    return err_c, err_p, err_b
