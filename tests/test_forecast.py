"""CPU: the predictive distribution of raincast_gnn.forecast.

(a) the oracle (tests/forecast_oracle.py) is the distribution the reference's losses score:
    quadrature of (F - 1{x >= y})^2 and its closed-form CRPS against
    tests/golden/reference_crps_rows.npz (the reference's own per-row values);
(b) the package's torch path against the oracle, at the bounds of the GPU tests
    (tests/forecast_cases.py);
(c) the conventions: atom, continuity at u, monotonicity, edge levels, units, from_model;
(d) the C entries' host-side validation (no device needed).
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch
from scipy.integrate import quad

import forecast_cases as FC
from conftest import GOLDEN
from forecast_oracle import C, Dist
from raincast_gnn import _lib, evaluate
from raincast_gnn.forecast import Forecast, ForecastScore, pit_sample
from raincast_gnn.params import EXPERIMENTS

FIXTURE = {"normal": "normal", "mixed_normal": "normal_mixed", "mixed": "mixed",
           "mixed_u": "mixed_u"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "reference_crps_rows.npz"))


def fixture_dist(golden, kind):
    name = FIXTURE[kind]
    pp = golden[f"{name}_pp"]
    return name, pp, Dist(kind, pp.astype(np.float64), u=FC.U_FIXED, xi=float(golden["xi"][0]))


def _quad_crps(one, y):
    """Integral of (F(x) - 1{x >= y})^2 for a one-row Dist, with breakpoints at c, y, u."""
    f = lambda x: (one.cdf([x])[0, 0] - (x >= y)) ** 2  # noqa: E731
    lo = one.c if one.atom else -np.inf
    pts = sorted({lo, y, np.inf} | ({float(one.u[0, 0])} if one.tail else set()))
    total = 0.0
    for a, b in zip(pts[:-1], pts[1:]):
        total += quad(f, a, b, epsabs=1e-14, epsrel=1e-11, limit=200)[0]
    return total


@pytest.mark.parametrize("kind", list(FIXTURE))
def test_oracle_integrates_to_the_reference_crps(golden, kind):
    """16 rows per kind (censored, body and -- for the tail kinds -- y >= u rows, the first of
    each in the fixture's order): the quadrature of the oracle's F equals the reference's
    closed form evaluated in float64.  Measured worst |quad - ref| / max(|ref|, 1e-3): normal
    1.15e-7 (crps_no_avg keeps 1/sqrt(pi) and sqrt(2 pi) as fp32 tensors), mixed_normal
    1.4e-15, mixed 1.6e-15, mixed_u 5.9e-16.  Bound: ten times the worst measured (1.6e-15
    for the three censored kinds), and never looser than 1e-6, which caps the normal kind's."""
    name, pp, orc = fixture_dist(golden, kind)
    y = golden[f"{name}_y64"]
    ref = golden[f"{name}_crps64"]
    ok = ~np.isnan(y)
    u = orc.u[:, 0] if orc.tail else np.full(len(y), np.inf)
    groups = [ok & (y == C), ok & (y > C) & (y < u)] if orc.atom else [ok & (y < 0), ok & (y >= 0)]
    if orc.tail:
        groups.append(ok & (y >= u))
    per = [6, 5, 5] if orc.tail else [8, 8]
    rows = np.concatenate([np.flatnonzero(g)[:k] for g, k in zip(groups, per)])
    assert len(rows) == 16
    worst = 0.0
    for i in rows:
        one = Dist(kind, pp[i:i + 1].astype(np.float64), u=FC.U_FIXED, xi=orc.xi)
        worst = max(worst, abs(_quad_crps(one, float(y[i])) - ref[i]) / max(abs(ref[i]), 1e-3))
    print(f"{kind}: worst relative quadrature error {worst:.2e}")
    bound = 1e-6 if kind == "normal" else 1.6e-14
    assert worst <= bound, worst


@pytest.mark.parametrize("kind", list(FIXTURE))
def test_oracle_closed_form_matches_the_reference_rows(golden, kind):
    """The oracle's closed-form CRPS against the reference's rows on the fp32 tensors, within
    the project's loss bound 1e-6 * max_row |ref| (the reference's fp32 sub-expressions
    account for about 1e-7 of that scale)."""
    name, pp, orc = fixture_dist(golden, kind)
    y, ref = golden[f"{name}_y"], golden[f"{name}_crps"]
    ok = ~np.isnan(y)
    got = orc.crps_rows(y.astype(np.float64))
    err = np.abs(got - ref)[ok].max() / np.abs(ref[ok]).max()
    print(f"{kind}: closed form vs reference rows {err:.2e} of max |ref|")
    assert err <= 1e-6


@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
@pytest.mark.parametrize("n", [1, 65, 257])
def test_cpu_path_matches_the_oracle(kind, xi, n):
    params = FC.make_params(kind, n)
    fc, orc = FC.build(kind, xi, params, "cpu")
    for T in (1, 5, 33):
        x = FC.thresholds(kind, params, T)
        FC.check_prob(fc, orc, x)
        FC.check_quantile(fc, orc, T)
        FC.check_score(fc, orc, FC.make_targets(n, seed=T), x)
    FC.check_edge_levels(fc, orc)
    FC.check_score(fc, orc, np.full(n, np.nan, dtype=np.float32), FC.thresholds(kind, params, 5))
    FC.check_score(fc, orc, FC.make_targets(n), np.zeros(0))


@pytest.mark.parametrize("kind", list(FIXTURE))
def test_cpu_score_matches_the_reference_rows(golden, kind):
    name, pp, _ = fixture_dist(golden, kind)
    fc = Forecast(torch.from_numpy(pp), kind, u=FC.U_FIXED, xi=0.5)
    y, ref = golden[f"{name}_y"], golden[f"{name}_crps"]
    ok = ~np.isnan(y)
    sc = fc.score(torch.from_numpy(y))
    err = np.abs(sc.crps_rows.numpy() - ref)[ok].max() / np.abs(ref[ok]).max()
    assert err <= 1e-6
    assert isinstance(sc, ForecastScore) and float(sc.valid[0]) == ok.sum()
    assert abs(float(sc.crps) - ref[ok].mean()) <= 1e-6 * np.abs(ref[ok]).max()


@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
def test_conventions(kind, xi):
    params = FC.make_params(kind, 33, seed=3)
    fc, orc = FC.build(kind, xi, params, "cpu")
    grid = np.sort(np.concatenate([np.linspace(-8, 15, 400), [C, FC.U_FIXED]]))
    F = fc.cdf(grid).numpy()
    assert np.all(np.diff(F, axis=1) >= 0) and F.min() >= 0 and F.max() <= 1
    S = fc.exceedance(grid).numpy()
    assert np.all(np.diff(S, axis=1) <= 0)
    assert np.abs(F + S - 1).max() <= 1e-15 * 4
    if orc.atom:
        just_below = np.nextafter(C, -np.inf)
        at = fc.cdf([just_below, C]).numpy()
        assert np.all(at[:, 0] == 0.0)
        assert np.abs(at[:, 1] - orc.P_c[:, 0]).max() <= 1e-15
        assert np.all(fc.exceedance([just_below]).numpy() == 1.0)
        q = orc.P_c[:, 0].min() * np.array([0.0, 0.5, 1 - 1e-9])
        assert np.all(fc.quantile(q).numpy() == C)  # bitwise
        assert np.all(fc.quantile(q, unit="mm").numpy() <= 1e-17)
    if orc.tail:  # continuous at u: from the left (body) and at u itself (tail)
        for i in range(params.shape[0]):
            u = float(orc.u[i, 0])
            pair = fc.cdf([np.nextafter(u, -np.inf), u]).numpy()[i]
            assert abs(pair[0] - pair[1]) <= 1e-15 and abs(pair[1] - orc.m_u[i, 0]) <= 1e-15


def test_units_round_trip():
    params = FC.make_params("mixed", 17, seed=5)
    fc, orc = FC.build("mixed", 0.5, params, "cpu")
    mm = np.array([0.0, 0.1, 1.0, 20.0, 250.0])
    y = np.log(mm + 0.01)
    assert y[0] == C
    assert torch.equal(fc.cdf(mm, unit="mm"), fc.cdf(y))
    assert torch.equal(fc.exceedance(mm, unit="mm"), fc.exceedance(y))
    assert torch.all(fc.exceedance([-1.0], unit="mm") == 1.0)
    q = np.array([0.05, 0.5, 0.9, 0.99])
    x_mm, x = fc.quantile(q, unit="mm").numpy(), fc.quantile(q).numpy()
    assert np.all(x_mm >= 0) and np.all(x_mm[x == C] <= 1e-17)
    wet = x > C
    assert np.abs(np.log(x_mm[wet] + 0.01) - x[wet]).max() <= 1e-12
    # exceedance of the return level, through millimetres, gives the level back
    s = np.array([0.2, 0.01, 1e-6])
    lv = fc.return_level(s, unit="mm").numpy()
    for i in range(params.shape[0]):
        back = fc.exceedance(lv[i], unit="mm").numpy()[i]
        keep = s < orc.S_c[i, 0] * (1 - 1e-9)
        assert np.abs(back - s)[keep].max(initial=0.0) <= 1e-9 * 1.0
    with pytest.raises(ValueError):
        fc.cdf(mm, unit="inch")


def test_pit_sample():
    lo = torch.tensor([0.0, 0.3, float("nan")], dtype=torch.float64)
    hi = torch.tensor([0.6, 0.3, float("nan")], dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    a = pit_sample(lo, hi, g)
    assert 0.0 <= a[0] < 0.6 and a[1] == 0.3 and torch.isnan(a[2])
    assert torch.equal(a[:2], pit_sample(lo, hi, torch.Generator().manual_seed(1))[:2])


@pytest.mark.parametrize("variant,kind,K", [("normal", _lib.LOSS_NORMAL, 2),
                                            ("normal_mixed", _lib.LOSS_MIXED_NORMAL, 3),
                                            ("mixed", _lib.LOSS_MIXED, 4),
                                            ("mixed_u", _lib.LOSS_MIXED_U, 5)])
def test_from_model_reads_the_params_json_styles(variant, kind, K):
    cfg = EXPERIMENTS[f"24h_{variant}"]
    assert isinstance(cfg["grad_u"], str)  # "True" / "False", as params.json spells it
    model = types.SimpleNamespace(loss=cfg["loss"], grad_u=cfg["grad_u"], u=cfg["u"],
                                  xi=cfg["xi"])
    pred = torch.from_numpy(FC.make_params({2: "normal", 3: "mixed_normal", 4: "mixed",
                                            5: "mixed_u"}[K], 9))
    fc = Forecast.from_model(model, pred)
    assert fc.kind == kind and fc.c == C
    if K >= 4:
        assert fc.xi == 0.5
    if K == 4:
        assert fc.u == float(np.float32(1.71)) != 1.71
    y = torch.from_numpy(FC.make_targets(9))
    sc = evaluate.verify(model, pred, y, [1.0, 10.0, 50.0])
    assert sc.brier.shape == (3,) and sc.crps_rows.shape == (9,)
    want = fc.score(y, np.log(np.array([1.0, 10.0, 50.0]) + 0.01))
    assert torch.equal(sc.brier, want.brier)
    with pytest.raises(ValueError):
        Forecast.from_model(model, pred[:, :1])


def test_constructor_rejects_what_the_distribution_excludes():
    p4 = torch.from_numpy(FC.make_params("mixed", 3))
    for kw in ({"u": C, "xi": 0.5}, {"u": 1.0, "xi": 1.0}, {"u": 1.0, "xi": 0.0}, {"xi": 0.5},
               {"u": 1.0}):
        with pytest.raises(ValueError):
            Forecast(p4, "mixed", **kw)
    with pytest.raises(ValueError):
        Forecast(torch.from_numpy(FC.make_params("mixed_u", 3)), "mixed_u", xi=0.5, c=0.0)
    with pytest.raises(ValueError):
        Forecast(p4, "mixed_normal")


def test_entries_validate_before_any_device_call():
    """Bad kind, xi = 1, a fixed u <= c, negative N or T, NULL pred: GINE_ERR_INVALID (1);
    more than 2^24 thresholds: GINE_ERR_TOO_LARGE (4); N = 0: GINE_OK.  No device here, so
    any HIP call would fail with a status of 1000 or more."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    c = C
    for fn in (lib.gine_forecast_prob, lib.gine_forecast_quantile):
        assert fn(p, 4, 7, 1.71, 0.5, c, p, 2, 0, p, None) == 1           # kind
        assert fn(p, 4, -1, 1.71, 0.5, c, p, 2, 0, p, None) == 1
        assert fn(p, 4, 2, 1.71, 1.0, c, p, 2, 0, p, None) == 1           # xi = 1
        assert fn(p, 4, 3, 0.0, 0.0, c, p, 2, 0, p, None) == 1            # xi = 0
        assert fn(p, 4, 3, 0.0, float("nan"), c, p, 2, 0, p, None) == 1
        assert fn(p, 4, 2, c, 0.5, c, p, 2, 0, p, None) == 1              # u <= c
        assert fn(p, 4, 3, 0.0, 0.5, 0.0, p, 2, 0, p, None) == 1          # mixed_u, c >= 0
        assert fn(p, -1, 0, 0.0, 0.5, c, p, 2, 0, p, None) == 1           # N < 0
        assert fn(p, 4, 0, 0.0, 0.5, c, p, -2, 0, p, None) == 1           # T < 0
        assert fn(p, 4, 0, 0.0, 0.5, c, p, 2, 2, p, None) == 1            # flag
        assert fn(None, 4, 0, 0.0, 0.5, c, p, 2, 0, p, None) == 1         # NULL pred
        assert fn(p, 4, 0, 0.0, 0.5, c, None, 2, 0, p, None) == 1
        assert fn(p, 4, 0, 0.0, 0.5, c, p, 2, 0, None, None) == 1
        assert fn(p, 4, 0, 0.0, 0.5, c, p, (1 << 24) + 1, 0, p, None) == 4
        assert fn(None, 0, 2, 1.71, 0.5, c, None, 2, 0, None, None) == 0  # N = 0
        assert fn(p, 4, 1, 0.0, 7.0, c, None, 0, 1, None, None) == 0      # T = 0; xi unused
    f = lib.gine_forecast_score
    args = lambda **kw: [kw.get(k, d) for k, d in (  # noqa: E731
        ("pred", p), ("y", p), ("n", 4), ("kind", 2), ("u", 1.71), ("xi", 0.5), ("c", c),
        ("x", p), ("T", 2), ("crps", None), ("lo", None), ("hi", None), ("brier", p),
        ("valid", None), ("partials", p), ("ticket", p), ("stream", None))]
    for bad in ({"kind": 4}, {"xi": 1.0}, {"u": c - 1}, {"n": -1}, {"T": -1}, {"pred": None},
                {"y": None}, {"partials": None}, {"ticket": None}, {"brier": None},
                {"x": None}, {"kind": 3, "c": 0.5}):
        assert f(*args(**bad)) == 1, bad
    assert f(*args(T=(1 << 24) + 1)) == 4
    assert f(*args(n=0, pred=None, y=None)) == 0
    n = ctypes.c_size_t(0)
    q = lib.gine_forecast_score_partials
    assert q(16000, 8, ctypes.byref(n)) == 0 and n.value == 250 * 9
    assert q(0, 0, ctypes.byref(n)) == 0 and n.value == 1
    assert q(65, 3, ctypes.byref(n)) == 0 and n.value == 2 * 4
    assert q(-1, 3, ctypes.byref(n)) == 1 and q(5, -1, ctypes.byref(n)) == 1
    assert q(5, 3, None) == 1
