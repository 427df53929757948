"""Seeded cases and the checks of raincast_gnn.ensemble against tests/ensemble_oracle.py, shared
by the CPU tests (the package's torch formulation) and the GPU tests (the kernels): the same
properties at the same bounds on either device.

Members are log(r + 0.01) in fp32 with r = 0 w.p. 0.5, else Gamma(0.7, 6): many exact ties at
c = log 0.01; |values| <= 10; about 5 % NaN.  From three rows on, row 1 has no valid member and
row 2 a single one.  Targets: about half at c (exactly the dry members' value), every seventh
row exactly equal to one of its members, about 5 % NaN.

Bounds: score fields 1e-12 absolute (values <= 10, sums over <= 64^2 fp64 terms: a few hundred
ulp of 10); ranks, m and prob exactly (integer counts, and one IEEE division of exact operands).
"""
import functools
import math

import numpy as np
import torch

import ensemble_oracle as EO
from raincast_gnn.ensemble import RawEnsemble

C = math.log(0.01)
C_F32 = np.float32(C)
THRESHOLDS = np.array([C, math.log(1.0 + 0.01), math.log(10.0 + 0.01)])  # 0, 1, 10 mm
SCORE_TOL = 1e-12
ROW_FIELDS = (("crps_rows", "crps"), ("crps_fair_rows", "crps_fair"))


def make_members(n, M, seed=0):
    r = np.random.default_rng(1000 * seed + 97 * n + M)
    rain = np.where(r.random((n, M)) < 0.5, 0.0, r.gamma(0.7, 6.0, (n, M)))
    x = np.clip(np.log(rain + 0.01), -10.0, 10.0).astype(np.float32)
    x[r.random((n, M)) < 0.05] = np.nan
    if n >= 3:
        x[1, :] = np.nan
        x[2, :] = np.nan
        x[2, M // 2] = np.float32(0.75)
    return x


def make_targets(members, seed=0):
    n, M = members.shape
    r = np.random.default_rng(31 + 1000 * seed + 97 * n + M)
    y = np.where(r.random(n) < 0.5, C_F32, np.clip(r.normal(0.5, 1.5, n), -4.0, 10.0))
    y = y.astype(np.float32)
    for i in range(3, n, 7):  # exactly one of the row's members (which may be NaN: missing)
        y[i] = members[i, i % M]
    y[r.random(n) < 0.05] = np.nan
    if n >= 3:
        y[2] = np.float32(0.75)  # the single member itself
    return y


@functools.lru_cache(maxsize=None)
def case(n, M, seed=0):
    """Members, targets and the oracle's results, computed once per shape (read-only)."""
    mem = make_members(n, M, seed)
    y = make_targets(mem, seed)
    ref = reference(mem, y)
    for a in (mem, y):
        a.setflags(write=False)
    return mem, y, ref


def reference(mem, y, scale=1.0, shift=0.0, thresholds=THRESHOLDS):
    x = EO.values(mem, scale, shift)
    ref = EO.score_rows(x, y)
    ref["prob"] = EO.prob(x, thresholds)
    ref["brier"], ref["valid"] = EO.brier(ref["prob"], y, thresholds, ref["crps"])
    ref["x"] = x
    return ref


def _np(t):
    return t.detach().cpu().numpy()


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def check_score(raw, y, ref, thresholds=THRESHOLDS):
    """The score of `raw` against the oracle's `ref`; -> worst absolute error of the fp fields."""
    sc = raw.score(torch.from_numpy(np.array(y)).to(raw.device), thresholds)
    worst = 0.0
    for name, key in ROW_FIELDS:
        got = _np(getattr(sc, name))
        assert same_nan(got, ref[key]), name
        ok = ~np.isnan(ref[key])
        if ok.any():
            worst = max(worst, float(np.abs(got - ref[key])[ok].max()))
    for name in ("rank_lo", "rank_hi"):
        assert np.array_equal(_np(getattr(sc, name)), ref[name], equal_nan=True), name
    assert np.array_equal(_np(sc.members_valid), ref["m"])
    assert np.array_equal(_np(sc.prob), ref["prob"], equal_nan=True)
    assert float(_np(sc.valid)[0]) == ref["valid"]
    got = _np(sc.brier)
    assert same_nan(got, ref["brier"])
    if ref["valid"] and len(thresholds):
        worst = max(worst, float(np.abs(got - ref["brier"]).max()))
    for prop, rows in (("crps", "crps"), ("crps_fair", "crps_fair")):
        ok = ~np.isnan(ref[rows])
        if ok.any():
            worst = max(worst, abs(float(getattr(sc, prop)) - float(ref[rows][ok].mean())))
    assert worst <= SCORE_TOL, worst
    return worst, sc


def level_table(M):
    """Every ECC level an ensemble of up to M members can take, computed on the host, and the
    column of (rule, m, r) in it."""
    levels, col = [], {}
    for m in range(1, M + 1):
        for r in range(1, m + 1):
            col["uniform", m, r] = len(levels)
            levels.append(np.float64(r) / np.float64(m + 1))
            col["midpoint", m, r] = len(levels)
            levels.append((np.float64(r) - 0.5) / np.float64(m))
    return np.array(levels), col


def expected_ecc(fc, x, rule):
    """Forecast.quantile on fc's device at the host-computed levels, gathered by the oracle's
    ranks: [N, M] fp64, NaN where the member is missing."""
    N, M = x.shape
    levels, col = level_table(M)
    Q = _np(fc.quantile(levels))
    r, m = EO.ranks(x)
    want = np.full((N, M), np.nan)
    for n in range(N):
        for i in range(M):
            if r[n, i]:
                want[n, i] = Q[n, col[rule, int(m[n]), int(r[n, i])]]
    return want


def check_ecc(fc, raw, x, rule):
    """-> (worst absolute difference, bitwise equal?) of Forecast.ecc against expected_ecc."""
    got = _np(fc.ecc(raw, levels=rule))
    want = expected_ecc(fc, x, rule)
    assert got.shape == want.shape and same_nan(got, want)
    ok = ~np.isnan(want)
    assert np.all(np.isfinite(want[ok]))  # the levels lie strictly inside (0, 1)
    err = float(np.abs(got - want)[ok].max()) if ok.any() else 0.0
    exact = bool(np.array_equal(got.view(np.int64)[ok], want.view(np.int64)[ok]))
    assert err <= 1e-12, err
    return err, exact


def raw_on(mem, device, **kw):
    return RawEnsemble(torch.from_numpy(np.array(mem)).to(device), **kw)
