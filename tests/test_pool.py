"""CPU: raincast_gnn.pool's fp64 torch formulation (the path of CPU tensors and of pools with
more than 32 members) against tests/pool_oracle.py and the mpmath fixture
tests/golden/pool_crps_rows.npz; the C ABI of the four gine_pool_* entry points and their host
validation without a device; the Gauss-Jacobi rule; evaluate.predict_ensemble(stack=True) and
evaluate.verify_pool.  Bounds in tests/pool_cases.py; tests/test_gpu_pool.py runs the same
checks on the kernels.

Measured (this path, worst over the fixture, printed with -s): CRPS rows 2.7e-16 of the
largest row of their case (bound 1e-11); Golub-Welsch against scipy: nodes 2.2e-16, weights
1.1e-15.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import forecast_cases as FC
import pool_cases as PC
from conftest import ROOT
from raincast_gnn import _lib, pool
from raincast_gnn.forecast import Forecast
from raincast_gnn.pool import ForecastPool

NAMES = ("gine_pool_prob", "gine_pool_quantile", "gine_pool_score_partials", "gine_pool_score")


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
@pytest.mark.parametrize("M", [2, 3, 7])
def test_torch_path_matches_the_oracle(kind, xi, M):
    n = 13
    params = PC.members(kind, n, M)
    pl, orc = PC.build(kind, xi, params, "cpu")
    worst = np.zeros(7)
    for T in (1, 5, 33):
        x = PC.thresholds(kind, params, T)
        worst[0:2] = np.maximum(worst[0:2], PC.check_prob(pl, orc, x))
        worst[2:4] = np.maximum(worst[2:4], PC.check_quantile(pl, orc, T))
        worst[4:7] = np.maximum(worst[4:7], PC.check_score(pl, orc, FC.make_targets(n, seed=T), x))
    print(f"{kind} xi={xi} M={M}: F {worst[0]:.1e} abs, upper {worst[1]:.1e} rel, "
          f"F(Q(q))-q {worst[2]:.1e}, sf(Q(s))/s-1 {worst[3]:.1e}, member crps {worst[4]:.1e} of "
          f"scale, pit {worst[5]:.1e}, brier {worst[6]:.1e}")


def test_crps_matches_the_mpmath_fixture():
    print(f"torch path, worst over the fixture: {PC.check_fixture('cpu'):.2e} of max |row|")


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
@pytest.mark.parametrize("copies", [1, 2, 4])
def test_copies_of_one_member_are_that_forecast(kind, xi, copies):
    PC.check_copies(kind, xi, 11, copies, "cpu")


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
def test_score_bookkeeping(kind, xi):
    """All targets NaN; T = 0; N = 0; equal members under different targets; two calls."""
    n, M = 9, 3
    params = PC.members(kind, n, M)
    pl, orc = PC.build(kind, xi, params, "cpu")
    x = PC.thresholds(kind, params, 5)
    PC.check_score(pl, orc, np.full(n, np.nan, dtype=np.float32), x)
    PC.check_score(pl, orc, FC.make_targets(n, seed=9), np.zeros(0))
    y = torch.from_numpy(FC.make_targets(n, seed=9))
    a, b = pl.score(y, x), pl.score(y, x)
    for name in ("crps_rows", "member_crps_rows", "diversity_rows", "pit_lo", "pit_hi", "brier",
                 "valid"):
        assert PC.same_bits(getattr(a, name), getattr(b, name)), name
    empty = ForecastPool(pl.preds[:, :0], pl.kind, u=pl.u, xi=pl.xi)
    assert empty.cdf(x).shape == (0, 5) and empty.quantile([0.5]).shape == (0, 1)
    sc = empty.score(y[:0], x)
    assert torch.isnan(sc.brier).all() and float(sc.valid[0]) == 0.0
    assert sc.diversity_rows.shape == (0,) and pl.cdf(np.zeros(0)).shape == (n, 0)
    twice = np.concatenate([params[:, :1], params[:, :1]], axis=1)
    pl2, _ = PC.build(kind, xi, twice, "cpu")
    v = pl2.score(torch.tensor([0.3, 4.0])).diversity_rows
    assert PC.same_bits(v[0:1], v[1:2]) and float(v[0]) > 0.0


@pytest.mark.parametrize("kind,xi", [("normal", None), ("mixed_normal", None), ("mixed", 0.5),
                                     ("mixed_u", 0.2)])
def test_weights(kind, xi):
    PC.check_weights(kind, xi, "cpu")


def test_constructor_validates():
    p = torch.from_numpy(PC.members("mixed", 4, 2))
    with pytest.raises(ValueError):
        ForecastPool(p[0], "mixed", u=FC.U_FIXED, xi=0.5)          # not [M, N, K]
    with pytest.raises(ValueError):
        ForecastPool(p, "mixed_u", xi=0.5)                         # width 4 is not mixed_u's 5
    with pytest.raises(ValueError):
        ForecastPool(p, "mixed", u=FC.U_FIXED)                     # no xi
    with pytest.raises(ValueError):
        ForecastPool(p[:0], "mixed", u=FC.U_FIXED, xi=0.5)         # no member
    pl = ForecastPool(p, "mixed", u=FC.U_FIXED, xi=0.5)
    assert len(pl.members()) == 2 and isinstance(pl.members()[1], Forecast)
    assert torch.equal(pl.members()[1].pred, p[1])
    with pytest.raises(ValueError):
        pl.quantile(np.zeros((3, 2)))                              # per-row levels need N rows
    with pytest.raises(ValueError):
        pl.score(torch.zeros(3))


def test_reliability_and_ecc_take_the_pool():
    from raincast_gnn.ensemble import RawEnsemble
    n, M = 40, 3
    params = PC.members("mixed", n, M)
    pl, orc = PC.build("mixed", 0.5, params, "cpu")
    y = torch.from_numpy(FC.make_targets(n, seed=2))
    rel = pl.reliability(y, [0.0, 1.0], unit="mm")
    ref = Forecast(torch.from_numpy(params[0]), "mixed", u=FC.U_FIXED, xi=0.5) \
        .reliability(y, [0.0, 1.0], unit="mm")
    assert type(rel) is type(ref)
    r = np.random.default_rng(0)
    mem = r.normal(0.0, 2.0, (n, 6)).astype(np.float32)
    mem[3, 2] = np.nan
    raw = RawEnsemble(torch.from_numpy(mem))
    out = pl.ecc(raw, "uniform")
    lv = raw._levels_torch("uniform")
    assert out.shape == (n, 6) and torch.isnan(out[3, 2]) and not torch.isnan(out[3, 3])
    assert PC.same_bits(out, pl.quantile(lv))
    free = (lv.numpy() > orc.P_c * (1 + 1e-12)) & ~np.isnan(lv.numpy())
    got = orc.cdf(np.nan_to_num(out.numpy(), nan=0.0))
    assert np.abs(got - lv.numpy())[free].max() <= 1e-12
    # the rank structure of the raw ensemble survives
    order = np.argsort(mem[0], kind="stable")
    assert np.array_equal(np.sort(out[0].numpy()), out[0].numpy()[order])


# ---------------------------------------------------------------------------------------
# ABI and host validation
# ---------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_pool_entry_points():
    import raincast_gnn
    assert raincast_gnn.ForecastPool is ForecastPool and raincast_gnn.PoolScore is pool.PoolScore
    text = open(os.path.join(ROOT, "include", "gine_hip.h")).read()
    assert re.search(r"#define GINE_ABI_VERSION 10\b", text)
    lib = _lib.load()
    assert lib.gine_abi_version() == 10 and _lib.ABI_VERSION == 10
    for name in NAMES:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, re.M)
        assert m, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name]) == m.group(1).count(",") + 1, name


def test_pool_entry_points_validate_without_a_device():
    """Every rejection comes before any HIP call; N = 0 is ok and launches nothing."""
    lib = _lib.load()
    MIXED, c, u, xi = _lib.LOSS_MIXED, FC.C, FC.U_FIXED, 0.5
    one = ctypes.c_void_p(8)  # never dereferenced on these paths

    def prob(M=3, N=0, kind=MIXED, u=u, xi=xi, T=2, flags=0):
        return lib.gine_pool_prob(one, M, N, kind, u, xi, c, one, one, T, flags, one, None)

    def quant(M=3, N=0, T=2, stride=0, flags=0):
        return lib.gine_pool_quantile(one, M, N, MIXED, u, xi, c, one, one, T, stride, flags,
                                      one, None)

    def score(M=3, N=0, kind=MIXED, xi=xi, T=2):
        return lib.gine_pool_score(one, one, M, N, kind, u, xi, c, one, one, T, one, one,
                                   *([one] * 9), None)

    for f in (prob, quant, score):
        assert f() == _lib.GINE_OK
        for M in (0, -1, 33):
            assert f(M=M) == _lib.GINE_ERR_INVALID, (f.__name__, M)
        assert f(M=1) == _lib.GINE_OK and f(M=32) == _lib.GINE_OK
        assert f(N=-1) == _lib.GINE_ERR_INVALID
        assert f(T=-1) == _lib.GINE_ERR_INVALID
        assert f(T=0) == _lib.GINE_OK
        assert f(N=2 ** 31) == _lib.GINE_ERR_TOO_LARGE
    assert prob(kind=9) == _lib.GINE_ERR_INVALID and score(kind=-1) == _lib.GINE_ERR_INVALID
    assert prob(xi=1.0) == _lib.GINE_ERR_INVALID and score(xi=0.0) == _lib.GINE_ERR_INVALID
    assert prob(u=c) == _lib.GINE_ERR_INVALID
    assert prob(flags=2) == _lib.GINE_ERR_INVALID and quant(flags=4) == _lib.GINE_ERR_INVALID
    assert quant(stride=1) == _lib.GINE_ERR_INVALID and quant(stride=-1) == _lib.GINE_ERR_INVALID
    assert quant(stride=2) == _lib.GINE_OK
    count = ctypes.c_size_t(0)
    assert lib.gine_pool_score_partials(130, 5, ctypes.byref(count)) == _lib.GINE_OK
    assert count.value == 130 * 6
    assert lib.gine_pool_score_partials(0, 5, ctypes.byref(count)) == _lib.GINE_OK
    assert count.value == 6
    assert lib.gine_pool_score_partials(-1, 5, ctypes.byref(count)) == _lib.GINE_ERR_INVALID
    assert lib.gine_pool_score_partials(1, -1, ctypes.byref(count)) == _lib.GINE_ERR_INVALID
    assert lib.gine_pool_score_partials(1, 1, None) == _lib.GINE_ERR_INVALID


@pytest.mark.parametrize("xi", [0.2, 0.5, 0.8])
def test_golub_welsch_rule_matches_scipy(xi):
    from scipy.special import roots_jacobi
    alpha = 2.0 / xi - 2.0
    t, lam = roots_jacobi(pool.GJ_NODES, 0.0, alpha)
    nodes, weights = pool.tail_rule(xi)
    assert nodes.shape == weights.shape == (32,)
    err_n = np.abs(nodes - (1.0 + t) / 2.0).max()
    err_w = np.abs(weights - lam / 2.0 ** (alpha + 1.0)).max()
    print(f"xi={xi}: nodes {err_n:.1e}, weights {err_w:.1e}")
    assert err_n <= 1e-13 and err_w <= 1e-13
    assert abs(weights.sum() - 1.0 / (alpha + 1.0)) <= 1e-14   # int_0^1 w^alpha dw
    assert pool.tail_rule(xi)[0] is nodes                       # cached per xi


# ---------------------------------------------------------------------------------------
# evaluate
# ---------------------------------------------------------------------------------------
def _toy():
    from oracle import gine_cpu as O
    return O.OracleGNN(35, 32, 1, "MixedLoss", "False", 1.71, 0.5)


def _toy_states(batches, seeds=(1, 2, 3)):
    out = []
    for seed in seeds:
        torch.manual_seed(seed)
        m = _toy().train()
        with torch.no_grad():
            for b in batches:
                m(b)
        out.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    return out


def test_predict_ensemble_stack_and_verify_pool():
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.evaluate import predict_ensemble, verify, verify_pool
    batches = [synthetic_batch(20, 2, k=4, seed=s) for s in (3, 4)]
    states = _toy_states(batches)
    default = predict_ensemble(_toy, states, batches, "cpu")
    stacked = predict_ensemble(_toy, states, batches, "cpu", stack=True)
    assert stacked.shape == (3,) + tuple(default.shape)
    assert torch.equal(stacked.mean(dim=0), default)
    one = predict_ensemble(_toy, states[:1], batches, "cpu", stack=True)
    assert one.shape == (1,) + tuple(default.shape)
    from types import SimpleNamespace
    model = SimpleNamespace(loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)  # a params.json
    targets = torch.cat([b.y for b in batches]).float().reshape(-1)
    targets[5] = float("nan")
    v = verify_pool(model, stacked, targets, [0.0, 1.0, 10.0])
    want = verify(model, default, targets, [0.0, 1.0, 10.0])
    assert PC.same_bits(v.average.crps_rows, want.crps_rows)
    assert float(v.pool.valid[0]) == targets.numel() - 1
    assert abs(float(v.pool_crps) - (float(v.member_crps) - float(v.diversity))) <= 1e-13
    assert float(v.diversity) > 0.0 and float(v.pool_crps) < float(v.member_crps)
    assert v.pool.brier.shape == (3,) and torch.isfinite(v.pool.brier).all()
