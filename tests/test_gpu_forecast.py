"""GPU: the forecast kernels (csrc/gine_forecast.hip) against the independent oracle
(tests/forecast_oracle.py), the reference's per-row CRPS (tests/golden/
reference_crps_rows.npz) and the shipped fused loss; bounds in tests/forecast_cases.py.

Shapes: N in {1, 65, 257, 1031} (one row, one row past a 64-row tile, a partial tile after
four, several workgroups), T and Q in {1, 5, 33} (fewer pairs than lanes, T not dividing 256,
more thresholds than waves), every kind, xi in {0.2, 0.5, 0.8}.

Measured on MI355X, worst over all cases (each test prints its own with -s): F 3.3e-16
absolute; P(Y > x) 2.3e-13 relative; quantiles |F(Q(q)) - q| 2.4e-15 and |sf(Q(s)) - s| / s
3.1e-14; CRPS rows 7.1e-16 of the largest row, PIT 2.2e-16, Brier 3.9e-16; CRPS rows against
the reference's fp32 rows 1.1e-7 of the largest; mean of the rows against the fused loss 2.2e-16.
"""
import os

import numpy as np
import pytest
import torch

import forecast_cases as FC
from conftest import GOLDEN
from forecast_oracle import Dist
from raincast_gnn import _lib, forecast, loss
from raincast_gnn.forecast import Forecast

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = {"normal": "normal", "mixed_normal": "normal_mixed", "mixed": "mixed",
           "mixed_u": "mixed_u"}


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
@pytest.mark.parametrize("n", [1, 65, 257, 1031])
def test_kernels_match_the_oracle(kind, xi, n):
    params = FC.make_params(kind, n)
    fc, orc = FC.build(kind, xi, params, DEV)
    worst = np.zeros(7)
    for T in (1, 5, 33):
        x = FC.thresholds(kind, params, T)
        worst[0:2] = np.maximum(worst[0:2], FC.check_prob(fc, orc, x))
        worst[2:4] = np.maximum(worst[2:4], FC.check_quantile(fc, orc, T))
        worst[4:7] = np.maximum(worst[4:7], FC.check_score(fc, orc, FC.make_targets(n, seed=T), x))
    FC.check_edge_levels(fc, orc)
    print(f"{kind} xi={xi} N={n}: F {worst[0]:.1e} abs, upper {worst[1]:.1e} rel, "
          f"F(Q(q))-q {worst[2]:.1e}, sf(Q(s))/s-1 {worst[3]:.1e}, crps {worst[4]:.1e} of "
          f"scale, pit {worst[5]:.1e}, brier {worst[6]:.1e}")


@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
def test_score_edge_cases(kind, xi):
    """All targets NaN: NaN rows, NaN Brier, count 0.  No thresholds.  Row outputs left out
    (NULL).  Two launches: the same bits, and the ticket back at 0."""
    n = 257
    params = FC.make_params(kind, n, seed=2)
    fc, orc = FC.build(kind, xi, params, DEV)
    x = FC.thresholds(kind, params, 5)
    FC.check_score(fc, orc, np.full(n, np.nan, dtype=np.float32), x)
    FC.check_score(fc, orc, FC.make_targets(n, seed=9), np.zeros(0))
    y = torch.from_numpy(FC.make_targets(n, seed=9)).to(DEV)
    a, b = fc.score(y, x), fc.score(y, x)
    for name in ("crps_rows", "pit_lo", "pit_hi", "brier", "valid"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert int(forecast._ticket(DEV).item()) == 0
    # brier and the count alone
    xt = torch.from_numpy(x).to(DEV)
    brier = torch.empty(5, dtype=torch.float64, device=DEV)
    partials = torch.empty(5 * 6, dtype=torch.float64, device=DEV)
    _lib.call("gine_forecast_score", _lib.ptr(fc.pred), _lib.ptr(y), n, fc.kind, fc.u, fc.xi,
              fc.c, _lib.ptr(xt), 5, None, None, None, _lib.ptr(brier), None,
              _lib.ptr(partials), _lib.ptr(forecast._ticket(DEV)), _lib.stream_handle(DEV))
    assert torch.equal(bits(brier), bits(a.brier))
    # nothing to do: no launch, no error
    empty = Forecast(fc.pred[:0], fc.kind, u=fc.u, xi=fc.xi)
    assert empty.cdf(x).shape == (0, 5) and empty.quantile([0.5]).shape == (0, 1)
    sc = empty.score(y[:0], x)
    assert torch.isnan(sc.brier).all() and float(sc.valid[0]) == 0.0
    assert fc.cdf(np.zeros(0)).shape == (n, 0)


@pytest.mark.parametrize("kind", list(FIXTURE))
def test_score_matches_the_reference_rows_and_the_fused_loss(kind):
    """crps_rows against the reference's own rows (1e-6 of max_row |ref|, the project's loss
    bound) and the oracle (forecast_cases.check_score); for the three kinds whose training
    loss is the CRPS of the distribution, the mean over valid rows against the shipped fused
    pass of csrc/gine_loss.hip in fp64 (1e-12 relative; NormalCRPS.crps itself rounds that
    pass's result to fp32, so the pass is called directly for it)."""
    golden = np.load(os.path.join(GOLDEN, "reference_crps_rows.npz"))
    name = FIXTURE[kind]
    pp, y, ref = golden[f"{name}_pp"], golden[f"{name}_y"], golden[f"{name}_crps"]
    fc = Forecast(torch.from_numpy(pp).to(DEV), kind, u=FC.U_FIXED, xi=0.5)
    orc = Dist(kind, pp.astype(np.float64), u=FC.U_FIXED, xi=0.5)
    x = FC.thresholds(kind, pp, 5)
    FC.check_score(fc, orc, y, x)
    yt = torch.from_numpy(y).to(DEV)
    sc = fc.score(yt, x)
    ok = ~np.isnan(y)
    err = np.abs(sc.crps_rows.cpu().numpy() - ref)[ok].max() / np.abs(ref[ok]).max()
    print(f"{kind}: crps rows vs reference {err:.2e} of max |ref|")
    assert err <= 1e-6
    if kind == "mixed_u":
        return
    if kind == "normal":
        fused = loss._fused(fc.pred, yt, _lib.LOSS_NORMAL)
    elif kind == "mixed_normal":
        fused = loss.MixedNormalCRPS().crps(fc.pred, yt)
    else:
        fused = loss.MixedLoss(grad_u=False, u=1.71, xi=0.5).crps(fc.pred, yt)
    assert fused.dtype == torch.float64
    mean = sc.crps_rows[torch.from_numpy(ok).to(DEV)].mean()
    rel = abs(float(mean) - float(fused)) / abs(float(fused))
    print(f"{kind}: mean of rows vs fused loss {rel:.2e}")
    assert rel <= 1e-12
    assert abs(float(sc.crps) - float(fused)) <= 1e-12 * abs(float(fused))


def test_prob_and_score_replay_from_one_graph():
    """gine_forecast_prob and gine_forecast_score recorded in one graph on one stream;
    replayed after pred and y were refilled in place: the bits of the eager calls."""
    n, kind = 1031, "mixed_u"
    pred = torch.from_numpy(FC.make_params(kind, n, seed=1)).to(DEV)
    y = torch.from_numpy(FC.make_targets(n, seed=1)).to(DEV)
    x = torch.from_numpy(FC.thresholds(kind, FC.make_params(kind, n, seed=1), 5)).to(DEV)
    fc = Forecast(pred, kind, xi=0.5)
    assert fc.pred.data_ptr() == pred.data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first calls (the ticket's allocation) outside the capture
        fc.exceedance(x), fc.score(y, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        S = fc.exceedance(x)
        sc = fc.score(y, x)
    pred.copy_(torch.from_numpy(FC.make_params(kind, n, seed=2)).to(DEV))
    y.copy_(torch.from_numpy(FC.make_targets(n, seed=2)).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    want_S, want = fc.exceedance(x), fc.score(y, x)
    assert torch.equal(bits(S), bits(want_S))
    for name in ("crps_rows", "pit_lo", "pit_hi", "brier", "valid"):
        assert torch.equal(bits(getattr(sc, name)), bits(getattr(want, name))), name
    _, orc = FC.build(kind, 0.5, FC.make_params(kind, n, seed=2), "cpu")
    assert float(sc.valid[0]) == orc.brier(FC.make_targets(n, seed=2), x.cpu().numpy())[1]
    assert int(forecast._ticket(DEV).item()) == 0


def test_model_to_exceedance_probabilities():
    """24h_mixed at 2 x 60 stations: the Predictor's output to P(rain > 1, 10, 50 mm)."""
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.inference import Predictor
    from raincast_gnn.models import gnn_from_params
    from raincast_gnn.params import EXPERIMENTS
    torch.manual_seed(0)
    model = gnn_from_params(EXPERIMENTS["24h_mixed"]).to(DEV).eval()
    batch = synthetic_batch(60, 2, k=5, seed=1).to(DEV)
    predictor = Predictor(model, capture=False)
    fc = Forecast.from_model(model, predictor(batch))
    assert fc.kind == _lib.LOSS_MIXED and fc.u == float(np.float32(1.71))
    prob = fc.exceedance([1.0, 10.0, 50.0], unit="mm")
    assert prob.shape == (120, 3) and prob.dtype == torch.float64
    assert torch.isfinite(prob).all() and prob.min() >= 0 and prob.max() <= 1
    assert (prob[:, 1:] <= prob[:, :-1]).all()
