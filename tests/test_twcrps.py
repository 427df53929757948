"""CPU: the threshold-weighted CRPS (raincast_gnn.twcrps; Forecast.twcrps, RawEnsemble.twcrps,
the loss classes' tw term, evaluate.verify_tw) in its fp64 torch formulation against the
independent oracle tests/twcrps_oracle.py: the integral by quadrature and the closed forms.
Cases and bounds: tests/twcrps_cases.py.
"""
import json
import math

import numpy as np
import pytest
import torch

import ensemble_cases as EC
import forecast_cases as FC
import twcrps_cases as TC
import twcrps_oracle as TO
from forecast_oracle import C, Dist
from raincast_gnn import RawEnsemble
from raincast_gnn.loss import MixedLoss, MixedNormalCRPS, NormalCRPS, tw_threshold_from_mm
from raincast_gnn.models import GNN, gnn_from_params, make_loss

CPU = torch.device("cpu")
N = 24
# the smallest fp32 at or above c: a target there is its own max(y, c)
C_UP = np.nextafter(np.float32(C), np.float32(0)) if float(np.float32(C)) < C else np.float32(C)


@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
def test_rows_match_closed_forms_and_quadrature(kind, xi):
    b, a, e = TC.check_rows(kind, xi, N, CPU, with_quad=True)
    print(f"{kind} xi={xi}: closed {b:.1e}, quadrature {a:.1e} (quad's estimate {e:.1e}) of scale")


def test_oracle_scalar_cdf_is_the_distribution():
    for kind, xi in FC.KIND_XI:
        P = FC.make_params(kind, 5).astype(np.float64)
        orc = Dist(kind, P, u=FC.U_FIXED if kind == "mixed" else None, xi=xi)
        x = np.array([-6.0, np.nextafter(C, -np.inf), C, -1.0, FC.U_FIXED, 2.0, 2.5, 9.0])
        for i in range(5):
            F, S = TO._row_cdf(orc, i)
            got = np.array([F(float(v)) for v in x])
            assert np.abs(got - orc.cdf(x)[i]).max() <= 1e-15
            up = np.array([S(float(v)) for v in x])
            # (two erfc's far out: their arguments' rounding is z^2 eps / 2 of the value)
            assert np.all(np.abs(up - orc.sf(x)[i]) <= 1e-12 * orc.sf(x)[i])


@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
def test_identities(kind, xi):
    P, y = FC.make_params(kind, N), FC.make_targets(N)
    fc, _ = FC.build(kind, xi, P, CPU)
    ok = ~np.isnan(y)
    # t = -inf is the CRPS at max(y, c) (at y for "normal"); max(y, c) as an fp32 target
    ye = y if kind == "normal" else np.maximum(y, C_UP)
    yt = torch.from_numpy(ye)
    crps = fc.score(yt).crps_rows.numpy()
    tw = fc.twcrps(yt, [-np.inf], rows=True).rows.numpy()[:, 0]
    scale = np.abs(crps[ok]).max()
    assert np.abs(tw - crps)[ok].max() <= 1e-12 * scale
    # non-increasing in t; +inf leaves nothing
    grid = np.concatenate([[-np.inf], np.linspace(-6.0, 8.0, 57), [np.inf]])
    rows = fc.twcrps(torch.from_numpy(y), grid, rows=True).rows.numpy()[ok]
    assert np.all(np.diff(rows, axis=1) <= 1e-13 * scale)
    assert np.all(rows[:, -1] == 0.0) and np.all(rows >= -1e-13 * scale)
    # continuous across t = u (each row's own u for mixed_u)
    if kind in ("mixed", "mixed_u"):
        for i in np.flatnonzero(ok)[:8]:
            u = float(P[i, 4]) if kind == "mixed_u" else FC.U_FIXED
            r = fc.twcrps(torch.from_numpy(y), [u - 1e-9, u, u + 1e-9], rows=True).rows.numpy()[i]
            assert np.abs(np.diff(r)).max() <= 1e-8 * scale
    # NaN rows, valid, rows=False, units, T = 0
    sc = fc.twcrps(torch.from_numpy(y), [1.0, float("nan")])
    assert sc.rows is None and sc.valid.item() == ok.sum() and torch.isnan(sc.mean[1])
    mm = fc.twcrps(torch.from_numpy(y), [10.0], unit="mm")
    assert mm.thresholds.item() == math.log(10.01)
    assert torch.equal(mm.mean, fc.twcrps(torch.from_numpy(y), [math.log(10.01)]).mean)
    none = fc.twcrps(torch.from_numpy(y), [], rows=True)
    assert none.mean.shape == (0,) and none.rows.shape == (N, 0) and none.valid.item() == ok.sum()
    gone = fc.twcrps(torch.full((N,), float("nan")), [1.0], rows=True)
    assert gone.valid.item() == 0 and torch.isnan(gone.mean).all() and torch.isnan(gone.rows).all()


@pytest.mark.parametrize("n,M", [(1, 1), (5, 2), (40, 11), (9, 65)])
def test_ensemble_matches_the_double_sum(n, M):
    mem, y, ref = TC.ensemble_case(n, M)
    worst = TC.check_ensemble(EC.raw_on(mem, CPU), y, ref)
    print(f"N={n} M={M}: {worst:.1e} abs")


def test_ensemble_ties_at_c_and_missing_members():
    nan, c = float("nan"), float(EC.C_F32)
    mem = np.array([[nan] * 5, [nan, nan, 0.5, nan, nan], [c, c, 1.0, c, 2.0], [c] * 5,
                    [0.0, nan, 2.0, 3.0, nan]], dtype=np.float32)
    y = np.array([0.0, -0.25, c, 1.5, nan], dtype=np.float32)
    ref = TC.ensemble_reference(mem.astype(np.float64), y)
    TC.check_ensemble(EC.raw_on(mem, CPU), y, ref)
    sc = RawEnsemble(torch.from_numpy(mem)).twcrps(torch.from_numpy(y), [c, 0.75])
    assert torch.isnan(sc.rows[[0, 4]]).all() and torch.isnan(sc.fair_rows[[0, 1, 4]]).all()
    assert sc.valid.item() == 3
    # at t = -inf it is the plain score
    plain = RawEnsemble(torch.from_numpy(mem)).score(torch.from_numpy(y))
    tw = RawEnsemble(torch.from_numpy(mem)).twcrps(torch.from_numpy(y), [-np.inf])
    assert np.allclose(tw.rows[:, 0].numpy(), plain.crps_rows.numpy(), rtol=0, atol=1e-13,
                       equal_nan=True)


# ------------------------------------------------------------------------------------- the loss
LOSSES = [("normal", None, "NormalCRPS", "False"), ("mixed_normal", None, "MixedNormalCRPS", "False"),
          ("mixed", 0.5, "MixedLoss", "False"), ("mixed", 0.2, "MixedLoss", "False"),
          ("mixed_u", 0.5, "MixedLoss", "True"), ("mixed_u", 0.8, "MixedLoss", "True")]


def _loss(name, grad_u, xi, **tw):
    return make_loss(name, grad_u, FC.U_FIXED, 0.5 if xi is None else xi, **tw)[0]


@pytest.mark.parametrize("kind,xi,name,grad_u", LOSSES)
def test_loss_weight_zero_is_the_plain_loss(kind, xi, name, grad_u):
    P, y = torch.from_numpy(FC.make_params(kind, N)), torch.from_numpy(FC.make_targets(N))
    outs = []
    for tw in ({}, dict(tw_threshold=1.0, tw_weight=0.0), dict(tw_threshold=None, tw_weight=0.5)):
        p = P.clone().requires_grad_(True)
        v = _loss(name, grad_u, xi, **tw).crps(p, y)
        v.backward()
        outs.append((v.detach(), p.grad))
    for v, g in outs[1:]:  # the same bits (the plain torch formulation's NaN gradients of
        # masked rows at xi != 0.5 included: pow of a negative base behind a where)
        assert v.dtype == outs[0][0].dtype and torch.equal(v, outs[0][0])
        assert torch.equal(g.view(torch.int32), outs[0][1].view(torch.int32))


@pytest.mark.parametrize("t", [-1.0, 1.0, FC.U_FIXED, 2.5])
@pytest.mark.parametrize("kind,xi,name,grad_u", LOSSES)
def test_loss_gradient_matches_finite_differences_of_the_oracle(kind, xi, name, grad_u, t):
    """tw_weight = 1: the mean twCRPS of the rows with a target.  Autograd of the torch
    formulation against central differences (h = 1e-6: truncation ~1e-12, rounding ~1e-10 of
    the value) of the oracle's closed forms in fp64; 1e-6 of the largest component."""
    P = FC.make_params(kind, N).astype(np.float64)
    y = FC.make_targets(N)
    ok = ~np.isnan(y)
    u = FC.U_FIXED if kind == "mixed" else None
    xi32 = None if xi is None else float(np.float32(xi))  # the loss rounds xi to fp32

    def oracle(Q):
        return TO.closed_rows(Dist(kind, Q, u=u, xi=xi32), y.astype(np.float64), t)[ok].mean()

    p = torch.from_numpy(P).requires_grad_(True)
    v = _loss(name, grad_u, xi, tw_threshold=t, tw_weight=1.0).crps(p, torch.from_numpy(y))
    v.backward()
    want = oracle(P)
    assert abs(v.item() - want) <= (1e-6 if kind == "normal" else 1e-12) * abs(want)  # fp32 result
    h, fd = 1e-6, np.zeros_like(P)
    for i in np.flatnonzero(ok):
        for k in range(P.shape[1]):
            hi, lo = P.copy(), P.copy()
            hi[i, k] += h
            lo[i, k] -= h
            fd[i, k] = (oracle(hi) - oracle(lo)) / (2 * h)
    g = p.grad.numpy()
    assert np.all(g[~ok] == 0.0)
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print(f"{kind} xi={xi} t={t}: value {abs(v.item() - want) / abs(want):.1e}, gradient {err:.1e}")
    assert err <= 1e-6, err


@pytest.mark.parametrize("kind,xi,name,grad_u", LOSSES)
def test_loss_is_the_weighted_sum_of_its_two_terms(kind, xi, name, grad_u):
    P = torch.from_numpy(FC.make_params(kind, N)).double()
    y = torch.from_numpy(FC.make_targets(N))
    plain = _loss(name, grad_u, xi).crps(P, y).double()
    tw = _loss(name, grad_u, xi, tw_threshold=1.0, tw_weight=1.0).crps(P, y).double()
    mix = _loss(name, grad_u, xi, tw_threshold=1.0, tw_weight=0.3).crps(P, y).double()
    tol = 1e-6 if kind == "normal" else 1e-13  # NormalCRPS returns fp32
    assert abs(mix - (0.7 * plain + 0.3 * tw)) <= tol * abs(plain)
    if name != "NormalCRPS":  # reduce=False keeps the reference's shape: the rows with a target
        kw = dict(grad_u=True, xi=xi) if grad_u == "True" else dict(grad_u=False, u=FC.U_FIXED, xi=xi)
        cls = MixedLoss if name == "MixedLoss" else MixedNormalCRPS
        rows = cls(reduce=False, tw_threshold=1.0, tw_weight=0.3,
                   **(kw if cls is MixedLoss else {})).crps(P, y)
        assert rows.shape == (int((~torch.isnan(y)).sum()), 1)
        assert abs(rows.mean() - mix) <= 1e-13 * abs(mix)


def test_constructor_errors_and_plumbing(tmp_path):
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            NormalCRPS(tw_threshold=1.0, tw_weight=bad)
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError):
            MixedLoss(grad_u=False, u=1.71, xi=0.5, tw_threshold=bad, tw_weight=0.5)
        with pytest.raises(ValueError):
            MixedNormalCRPS(tw_threshold=bad, tw_weight=0.5)
    with pytest.raises(TypeError):
        MixedNormalCRPS(True, np.log(0.01), 1.0, 0.5)  # keyword-only
    fn, k = make_loss("MixedLoss", "True", 1.71, 0.5, tw_threshold=2.0, tw_weight=0.25)
    assert (k, fn.tw_threshold, fn.tw_weight, fn.tw_on) == (5, 2.0, 0.25, True)
    assert not make_loss("MixedLoss", "False", 1.71, 0.5)[0].tw_on
    assert tw_threshold_from_mm(10.0) == math.log(10.01)
    plain = GNN(35, 16, 16, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)
    tw = GNN(35, 16, 16, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5, tw_threshold=2.0,
             tw_weight=0.5)
    assert tw.loss_fn.tw_on and not plain.loss_fn.tw_on
    assert list(tw.state_dict()) == list(plain.state_dict())
    from raincast_gnn import dropin
    from raincast_gnn.params import EXPERIMENTS, load_params, tw_from_params
    d = dropin.GNN(35, 16, 16, 2, loss="NormalCRPS", tw_threshold=1.0, tw_weight=0.5)
    assert d.loss_fn.tw_on and d.loss_fn.fused is False
    cfg = dict(EXPERIMENTS["24h_mixed"])
    assert tw_from_params(cfg) == (None, 0.0)
    assert not gnn_from_params(cfg).loss_fn.tw_on
    cfg.update(tw_threshold_mm=10.0, tw_weight=0.4)
    path = tmp_path / "params.json"
    path.write_text(json.dumps(cfg))
    m = gnn_from_params(load_params(str(path)))
    assert (m.loss_fn.tw_threshold, m.loss_fn.tw_weight) == (math.log(10.01), 0.4)
    assert dropin.reference_struct_from_params(cfg).loss_fn.tw_threshold == math.log(10.01)
    for bad in (dict(tw_weight=2.0), dict(tw_threshold_mm=-1.0), dict(tw_threshold_mm=None,
                                                                      tw_weight=0.5)):
        with pytest.raises(ValueError):
            tw_from_params(dict(cfg, **bad))


def test_verify_tw_on_the_cpu():
    from raincast_gnn.evaluate import verify_tw
    from raincast_gnn.ensemble import skill
    from raincast_gnn.forecast import Forecast
    mem, y, _ = TC.ensemble_case(40, 11)
    model = GNN(35, 16, 16, 1, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)
    preds = torch.from_numpy(FC.make_params("mixed", 40))
    raw, yt = EC.raw_on(mem, CPU), torch.from_numpy(np.array(y))
    out = verify_tw(model, preds, yt, raw, [0.0, 1.0, 10.0])
    assert out.model.shape == out.ensemble.shape == out.skill.shape == (3,)
    assert torch.equal(out.skill, skill(out.model, out.ensemble))
    assert torch.equal(out.thresholds, torch.log(torch.tensor([0.0, 1.0, 10.0]).double() + 0.01))
    a = Forecast.from_model(model, preds).twcrps(yt, out.thresholds, rows=True).rows
    b = raw.twcrps(yt, out.thresholds).rows
    both = ~torch.isnan(a) & ~torch.isnan(b)
    assert torch.equal(out.valid, both.sum(0).double())
    for t in range(3):
        assert abs(out.model[t] - a[both[:, t], t].mean()) <= 1e-14
        assert abs(out.ensemble[t] - b[both[:, t], t].mean()) <= 1e-14
