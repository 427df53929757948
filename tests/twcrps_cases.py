"""Seeded cases and checks of the threshold-weighted CRPS against tests/twcrps_oracle.py, shared
by the CPU tests (the package's torch formulation) and the GPU tests (the kernels): the same
properties at the same bounds on either device.

Rows: forecast_cases.make_params / make_targets (about half the targets at 0 mm, 5 % NaN).
Thresholds: -inf, nextafter(c, -inf), c, -1, u - 1e-9, u exactly, u + 1e-9, 2.5, 4,
u + 50 sigma_u, NaN; for "mixed_u" u is row 0's own, so the other rows take either branch at that
threshold (asserted).  For the kinds without a tail u is the fixed 1.71 and sigma_u is 1 all the
same, as in forecast_cases.thresholds (every row is 1e-110 or smaller at that last threshold).

Bounds: closed forms (b) 1e-12 of the largest |oracle| row of the threshold (the project's
CRPS-row bound); quadrature (a) quad's own error estimate + that bound.
"""
import functools
import math

import numpy as np
import torch

import forecast_cases as FC
import twcrps_oracle as TO
from forecast_oracle import C

ROW_TOL = 1e-12


def thresholds(kind, params):
    u = float(params[0, 4]) if kind == "mixed_u" else FC.U_FIXED
    su = float(params[0, 3]) if params.shape[1] > 3 else 1.0  # as forecast_cases.thresholds
    return np.array([-np.inf, np.nextafter(C, -np.inf), C, -1.0, u - 1e-9, u, u + 1e-9, 2.5, 4.0,
                     u + 50.0 * su, np.nan], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case(kind, xi, n, with_quad=False):
    """Parameters, targets, thresholds and the oracle's rows [N, T], computed once per shape
    (read-only): ``closed`` always, ``quad`` / ``quad_est`` on request."""
    P, y = FC.make_params(kind, n), FC.make_targets(n)
    x = thresholds(kind, P)
    _, orc = FC.build(kind, xi, P, "cpu")
    y64 = y.astype(np.float64)
    ref = {"closed": np.stack([TO.closed_rows(orc, y64, float(t)) for t in x], axis=1)}
    if with_quad:
        qs = [TO.quad_rows(orc, y64, float(t)) for t in x]
        ref["quad"] = np.stack([q[0] for q in qs], axis=1)
        ref["quad_est"] = np.stack([q[1] for q in qs], axis=1)
    for a in (P, y, x, *ref.values()):
        a.setflags(write=False)
    return P, y, x, ref


def branches(kind, P, x):
    """For the kinds with a tail: per threshold, whether some row takes the body form and
    whether some takes the tail form."""
    u = P[:, 4].astype(np.float64) if kind == "mixed_u" else np.full(len(P), FC.U_FIXED)
    tp = np.maximum(x[None, :], C)
    return (tp < u[:, None]).any(0), (tp >= u[:, None]).any(0)


def _np(t):
    return t.detach().cpu().numpy()


def check_rows(kind, xi, n, device, with_quad=False):
    """Forecast.twcrps on ``device`` against the oracle -> (worst closed-form error / scale,
    worst quadrature error / scale, worst quad estimate / scale)."""
    P, y, x, ref = case(kind, xi, n, with_quad)
    fc, _ = FC.build(kind, xi, np.array(P), device)
    sc = fc.twcrps(torch.from_numpy(np.array(y)).to(device), np.array(x), rows=True)
    rows, mean = _np(sc.rows), _np(sc.mean)
    ok = ~np.isnan(y)
    assert rows.shape == ref["closed"].shape
    assert float(_np(sc.valid)[0]) == ok.sum()
    assert np.all(np.isnan(rows[~ok])) and np.all(np.isnan(rows[:, -1]))  # NaN y, NaN threshold
    assert np.isnan(mean[-1])
    if not ok.any():
        assert np.all(np.isnan(mean))
        return 0.0, 0.0, 0.0
    worst_b = worst_a = worst_e = 0.0
    for t in range(len(x) - 1):
        want = ref["closed"][ok, t]
        assert not np.isnan(rows[ok, t]).any() and not np.isnan(want).any()
        scale = np.abs(want).max()
        err = np.abs(rows[ok, t] - want).max()
        assert err <= ROW_TOL * scale, (kind, xi, n, x[t], err, scale)
        scale = scale if scale > 0 else 1.0  # every row 0 on both sides: far above all mass
        worst_b = max(worst_b, float(err / scale))
        assert abs(mean[t] - want.mean()) <= ROW_TOL * scale
        if with_quad:
            q, e = ref["quad"][ok, t], ref["quad_est"][ok, t]
            d = np.abs(rows[ok, t] - q)
            worst_a = max(worst_a, float(d.max() / scale))
            worst_e = max(worst_e, float(e.max() / scale))
            assert np.all(d <= e + ROW_TOL * scale), (kind, xi, n, x[t], float(d.max() / scale))
    if kind in ("mixed", "mixed_u") and n > 1:
        body, tail = branches(kind, P, x[:-1])
        assert body.any() and tail.any()
        if kind == "mixed_u":  # one threshold, both branches among the rows
            assert (body & tail).any()
    return worst_b, worst_a, worst_e


@functools.lru_cache(maxsize=None)
def ensemble_case(n, M, seed=0):
    """ensemble_cases' members and targets with the oracle's twCRPS rows at ENS_THRESHOLDS."""
    import ensemble_cases as EC
    import ensemble_oracle as EO
    mem = EC.make_members(n, M, seed)
    y = EC.make_targets(mem, seed)
    ref = ensemble_reference(EO.values(mem, 1.0, 0.0), y)
    for a in (mem, y):
        a.setflags(write=False)
    return mem, y, ref


# below every member, the dry members' value (ties at c), mid-range, above most, NaN
ENS_THRESHOLDS = np.array([-np.inf, C, math.log(1.01), math.log(10.01), 9.0, np.nan])


def ensemble_reference(x, y, thresholds=ENS_THRESHOLDS):
    rows = [TO.ensemble_rows(x, y.astype(np.float64), float(t)) for t in thresholds]
    return np.stack([r[0] for r in rows], axis=1), np.stack([r[1] for r in rows], axis=1)


def check_ensemble(raw, y, ref, thresholds=ENS_THRESHOLDS):
    """RawEnsemble.twcrps against the double-sum oracle -> worst absolute error."""
    sc = raw.twcrps(torch.from_numpy(np.array(y)).to(raw.device), thresholds)
    worst = 0.0
    for got, want in ((_np(sc.rows), ref[0]), (_np(sc.fair_rows), ref[1])):
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            worst = max(worst, float(np.abs(got - want)[ok].max()))
    has = ~np.isnan(ref[0])
    assert float(_np(sc.valid)[0]) == has[:, 0].sum()
    for t in range(len(thresholds)):
        if has[:, t].any():
            worst = max(worst, abs(float(sc.mean[t]) - ref[0][has[:, t], t].mean()))
        else:
            assert np.isnan(float(sc.mean[t]))
    assert worst <= ROW_TOL, worst
    return worst
