"""CPU: the EMOS baseline (raincast_gnn.emos) on its fp64 torch path, with the
checks tests/emos_cases.py shares with the GPU tests, the host-side validation of the three C
entry points (no device needed) and the evaluate wrappers.

Measured here (each test prints its own with -s): worst excess of the objective over the
fixture's J_ref 4.1e-14 of max(1, |J_ref|) (bound 1e-10); worst oracle gradient at the
returned theta 0.98 of gtol max(1, |J|) (bound 2); the CPU formulation's rows at theta0
against the reference's 1.8e-16 of the largest row (bound 1e-6); the torch predictors against
the member-by-member oracle: mean 0, sd 2e-15 (bound 1e-13); the score of the fp32 prediction
against the fit's CRPS 2.4e-8 at the most, 0.12 of its bound.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import emos_cases as EC
from raincast_gnn import Emos, EmosFit, _lib, evaluate
from raincast_gnn.ensemble import RawEnsemble
from raincast_gnn.forecast import Forecast

CPU = "cpu"


@pytest.mark.parametrize("name,T", EC.fixture_cases())
def test_objective_reaches_the_reference_minimum(name, T):
    excess, ratio = EC.check_fixture_case(name, T, CPU)
    print(f"{name} T={T}: excess {excess:.2e}, gradient {ratio:.2f} of gtol max(1, |J|)")


def test_the_fixture_kept_its_cases():
    """15 of the 16 cases: at mixed (u 0.5, xi 0.3), T = 8, station 2, scipy's two optimisers
    ended in different minima 1.7e-3 apart, and the generator drops what they disagree on."""
    cases = EC.fixture_cases()
    assert len(cases) == 15 and ("mixed_xi03", 8) not in cases
    g = EC.fixture()
    assert max(float(g[f"{n}_T{T}_gap"].max()) for n, T in cases) <= 1e-12


@pytest.mark.parametrize("name,T", EC.fixture_cases())
def test_crps_at_the_start_matches_the_reference_rows(name, T):
    print(f"{name} T={T}: rows at theta0 {EC.check_crps_pinned(name, T):.2e} of the largest row")


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
@pytest.mark.parametrize("S,T,M", [(1, 8, 1), (3, 65, 2), (7, 130, 11), (0, 300, 64),
                                   (3, 65, 65)])
def test_descent_report_and_stationarity(kind, u, xi, S, T, M):
    f, ratio = EC.check_shape(kind, u, xi, S, T, M, CPU)
    print(f"{kind} xi={xi} S={S} T={T} M={M}: status {f['status'].tolist()}, gradient "
          f"{ratio:.2f} of gtol max(1, |J|)")


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
def test_edge_cases(kind, u, xi):
    EC.check_edge_cases(kind, u, xi, CPU)


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
def test_independence(kind, u, xi):
    """Repeated calls bit for bit; a station alone, permuted stations and other members under
    missing targets to the objective's bound: torch's batched reductions promise no bits across
    batch shapes (the kernel does: tests/test_gpu_emos.py)."""
    EC.check_independence(kind, u, xi, 65, 11, CPU, exact=False)


@pytest.mark.parametrize("S,T,M", [(1, 8, 1), (3, 65, 11), (0, 130, 64), (7, 8, 65)])
def test_predictors(S, T, M):
    err = EC.check_predictors(S, T, M, CPU)
    print(f"S={S} T={T} M={M}: mean {err[0]:.1e}, sd {err[1]:.1e}")


@pytest.mark.parametrize("kind,u,xi", EC.KINDS)
@pytest.mark.parametrize("S,T,M", [(3, 65, 11), (0, 130, 2)])
def test_predict_and_forecast(kind, u, xi, S, T, M):
    ulps, diff, bound = EC.check_predict(kind, u, xi, S, T, M, CPU)
    print(f"{kind} xi={xi} S={S}: {ulps:.2f} ulp, score against the fit {diff:.2e} "
          f"(bound {bound:.2e})")


def test_mixed_u_and_bad_arguments_are_rejected():
    with pytest.raises(ValueError, match="mixed_u"):
        Emos("mixed_u", xi=0.5)
    with pytest.raises(ValueError, match="mixed_u"):
        Emos(_lib.LOSS_MIXED_U, xi=0.5)
    model = types.SimpleNamespace(loss="MixedLoss", grad_u="True", u=1.71, xi=0.5)
    with pytest.raises(ValueError, match="mixed_u"):
        Emos.from_model(model)
    for kw in (dict(xi=None, u=0.5), dict(xi=1.0, u=0.5), dict(xi=0.5, u=None),
               dict(xi=0.5, u=EC.C)):
        with pytest.raises(ValueError):
            Emos("mixed", **kw)
    for kw in (dict(ridge=-1.0), dict(ridge=float("nan")), dict(gtol=float("inf")),
               dict(max_iter=-1), dict(min_rows=0)):
        with pytest.raises(ValueError):
            Emos("normal", **kw)
    e = Emos("normal")
    raw = RawEnsemble(torch.zeros(10, 3))
    with pytest.raises(ValueError, match="multiple"):
        e.fit(raw, torch.zeros(10), 3)
    with pytest.raises(ValueError, match="entries"):
        e.fit(raw, torch.zeros(9), 2)
    with pytest.raises(ValueError, match="positive"):
        e.fit(raw, torch.zeros(10), 0)


def test_from_model_reads_the_loss_as_forecast_does():
    model = types.SimpleNamespace(loss="MixedLoss", grad_u="False", u=1.71, xi=0.3)
    e = Emos.from_model(model, ridge=1e-2)
    fc = Forecast.from_model(model, torch.zeros(1, 4))
    assert (e.kind, e.u, e.xi, e.c, e.ridge) == (fc.kind, fc.u, fc.xi, fc.c, 1e-2)
    assert e.u == float(np.float32(1.71)) and e.xi == float(np.float32(0.3))
    assert Emos.from_model(types.SimpleNamespace(loss="NormalCRPS")).K == 2
    assert Emos.from_model(types.SimpleNamespace(loss="MixedNormalCRPS")).K == 3


def test_host_validation_without_device():
    """The three entry points return before any HIP call on bad arguments (and on nothing to
    do), in the style of tests/test_abi.py."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    c = EC.C
    pr = lib.gine_emos_predictors
    assert pr(p, 11, 1, 11, 1.0, 0.0, c, p, 0, 0, p, None) == 0            # no rows
    assert pr(None, 11, 1, 11, 1.0, 0.0, c, p, 0, 3, None, None) == 0
    assert pr(p, 11, 1, 0, 1.0, 0.0, c, p, 10, 0, p, None) == 1            # no members
    assert pr(p, 65, 1, 65, 1.0, 0.0, c, p, 10, 0, p, None) == 1           # M > 64
    assert pr(p, -1, 1, 11, 1.0, 0.0, c, p, 10, 0, p, None) == 1           # stride
    assert pr(p, 11, -1, 11, 1.0, 0.0, c, p, 10, 0, p, None) == 1
    assert pr(p, 11, 1, 11, 1.0, 0.0, c, p, -1, 0, p, None) == 1           # rows
    assert pr(p, 11, 1, 11, 1.0, 0.0, c, p, 10, -1, p, None) == 1          # stations
    assert pr(p, 11, 1, 11, 1.0, 0.0, c, p, 10, 3, p, None) == 1           # N % S
    assert pr(p, 11, 1, 11, 1.0, 0.0, float("nan"), p, 10, 0, p, None) == 1
    assert pr(None, 11, 1, 11, 1.0, 0.0, c, p, 10, 0, p, None) == 1        # NULL members
    assert pr(p, 11, 1, 11, 1.0, 0.0, c, p, 10, 0, None, None) == 1        # NULL pack
    ft = lib.gine_emos_fit

    def fit(kind=_lib.LOSS_MIXED, G=3, R=30, u=0.5, xi=0.5, ridge=1e-3, gtol=1e-8, it=200,
            rows=30, pack=p, ptr=p, theta=p, report=p):
        return ft(pack, ptr, G, R, kind, u, xi, c, ridge, gtol, it, rows, theta, report, None)

    assert fit(G=0) == 0                                                    # no groups
    assert fit(kind=_lib.LOSS_MIXED_U) == 1 and fit(kind=7) == 1 and fit(kind=-1) == 1
    assert fit(G=-1) == 1 and fit(R=-1) == 1
    assert fit(xi=0.0) == 1 and fit(xi=1.0) == 1 and fit(xi=float("nan")) == 1
    assert fit(u=c) == 1 and fit(u=c - 1.0) == 1
    assert fit(kind=_lib.LOSS_NORMAL, G=0, xi=7.0, u=c - 1.0) == 0          # not read there
    assert fit(ridge=-1e-3) == 1 and fit(ridge=float("nan")) == 1 and fit(ridge=float("inf")) == 1
    assert fit(gtol=-1.0) == 1 and fit(gtol=float("nan")) == 1
    assert fit(it=-1) == 1 and fit(it=_lib.EMOS_MAX_ITER + 1) == 1 and fit(rows=0) == 1
    assert fit(pack=None) == 1 and fit(ptr=None) == 1 and fit(theta=None) == 1
    assert fit(report=None) == 1
    pd = lib.gine_emos_predict
    assert pd(p, p, 0, 0, _lib.LOSS_NORMAL, p, None) == 0
    assert pd(p, p, 10, 0, _lib.LOSS_MIXED_U, p, None) == 1
    assert pd(p, p, 10, 3, _lib.LOSS_NORMAL, p, None) == 1                  # N % S
    assert pd(p, p, -1, 0, _lib.LOSS_NORMAL, p, None) == 1
    assert pd(None, p, 10, 0, _lib.LOSS_NORMAL, p, None) == 1
    assert pd(p, None, 10, 0, _lib.LOSS_NORMAL, p, None) == 1
    assert pd(p, p, 10, 0, _lib.LOSS_NORMAL, None, None) == 1


def test_fit_pack_needs_a_device():
    with pytest.raises(_lib.GineError, match="HIP devices only"):
        Emos("normal").fit_pack(torch.zeros(4, 4, dtype=torch.float64), torch.tensor([0, 4]))


def test_verify_against_emos_on_a_tiny_run():
    """A 'model' whose predictions are EMOS's own, shifted: finite skills, and rows that
    evaluate.compare takes."""
    S, T, M = 3, 40, 11
    model = types.SimpleNamespace(loss="MixedLoss", grad_u="False", u=0.5, xi=0.5)
    members, y = EC.make_data(S, T, M, seed=9)
    raw, yt = RawEnsemble(torch.from_numpy(members)), torch.from_numpy(y)
    fit = evaluate.fit_emos(model, raw, yt, S, min_rows=10)
    assert isinstance(fit, EmosFit) and fit.theta.shape == (S, 8)
    assert set(fit.status.tolist()) <= {0, 1, 2}
    preds = Emos.from_model(model).predict(raw, fit, S).clone()
    preds[:, 0] += 2.0                                            # a far worse location
    v = evaluate.verify_against_emos(model, preds, yt, raw, fit, S, thresholds=[0.1, 1.0])
    fs, es, crpss = v
    assert torch.isfinite(crpss) and float(crpss) < 0.0           # the shifted copy loses
    assert torch.isfinite(v.model_crps) and torch.isfinite(v.emos_crps)
    assert float(v.valid) == float((~torch.isnan(yt)).sum())
    assert torch.isfinite(es.brier).all() and torch.isfinite(fs.brier).all()
    # the EMOS score on the training rows is the fit's CRPS, station by station
    for s in range(S):
        rows = v.emos_rows[s::S]
        assert abs(float(torch.nanmean(rows)) - float(fit.crps[s])) <= 1e-6
    res = evaluate.compare(v.model_rows, v.emos_rows, S, replicates=50, seed=1)
    assert res.scores is not None and res.bootstrap is not None
