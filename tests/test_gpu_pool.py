"""GPU: the pool kernels (csrc/gine_pool.hip: gine_pool_prob / _quantile / _score) against
tests/pool_oracle.py, the mpmath fixture tests/golden/pool_crps_rows.npz, Forecast's kernels
(a pool of copies of one member: the same bits) and the package's fp64 torch formulation on the
CPU; bounds in tests/pool_cases.py.

Shapes: N in {1, 65, 130} (one row, one row past a 64-row tile, a partial third tile), M in
{1, 2, 3, 7, 32} (the cap with its 386 breakpoints and 16 rows per workgroup of the point
kernel; 3 and 7 divide nothing), T and Q in {1, 5, 33}, every kind, xi in {0.2, 0.5, 0.8}.

Measured on MI355X, worst over all cases (each test prints its own with -s): Fbar 4.4e-16
absolute; sfbar 2.1e-13 relative; quantiles |Fbar(Q(q)) - q| 1.2e-15 and |sfbar(Q(s)) - s| / s
4.6e-14; member CRPS 7.1e-16 of the largest row, PIT 3.3e-16, Brier 2.8e-16; CRPS rows against the
mpmath fixture 2.7e-16 of the largest row of a case (bound 1e-11); kernels against the torch path
on the CPU: CRPS 2.2e-16 and diversity 4.2e-17 of the largest row, Fbar 3.3e-16.
"""
import numpy as np
import pytest
import torch

import forecast_cases as FC
import pool_cases as PC
from raincast_gnn import forecast
from raincast_gnn.pool import ForecastPool

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
@pytest.mark.parametrize("M", [1, 2, 3, 7, 32])
@pytest.mark.parametrize("n", [1, 65, 130])
def test_kernels_match_the_oracle(kind, xi, n, M):
    params = PC.members(kind, n, M)
    pl, orc = PC.build(kind, xi, params, DEV)
    assert pl.on_kernel
    worst = np.zeros(7)
    for T in (1, 5, 33):
        x = PC.thresholds(kind, params, T)
        worst[0:2] = np.maximum(worst[0:2], PC.check_prob(pl, orc, x))
        worst[2:4] = np.maximum(worst[2:4], PC.check_quantile(pl, orc, T))
        worst[4:7] = np.maximum(worst[4:7], PC.check_score(pl, orc, FC.make_targets(n, seed=T), x))
    print(f"{kind} xi={xi} N={n} M={M}: F {worst[0]:.1e} abs, upper {worst[1]:.1e} rel, "
          f"F(Q(q))-q {worst[2]:.1e}, sf(Q(s))/s-1 {worst[3]:.1e}, member crps {worst[4]:.1e} of "
          f"scale, pit {worst[5]:.1e}, brier {worst[6]:.1e}")


def test_crps_matches_the_mpmath_fixture():
    print(f"kernels, worst over the fixture: {PC.check_fixture(DEV):.2e} of max |row|")


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
@pytest.mark.parametrize("copies", [1, 2, 4])
def test_copies_of_one_member_are_that_forecast(kind, xi, copies):
    PC.check_copies(kind, xi, 130, copies, DEV)


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
def test_score_bookkeeping(kind, xi):
    """All targets NaN; T = 0; N = 0; equal members under different targets; two calls: the
    same bits, and the ticket back at 0."""
    n, M = 130, 3
    params = PC.members(kind, n, M)
    pl, orc = PC.build(kind, xi, params, DEV)
    x = PC.thresholds(kind, params, 5)
    PC.check_score(pl, orc, np.full(n, np.nan, dtype=np.float32), x)
    PC.check_score(pl, orc, FC.make_targets(n, seed=9), np.zeros(0))
    y = torch.from_numpy(FC.make_targets(n, seed=9)).to(DEV)
    a, b = pl.score(y, x), pl.score(y, x)
    for name in ("crps_rows", "member_crps_rows", "diversity_rows", "pit_lo", "pit_hi", "brier",
                 "valid"):
        assert PC.same_bits(getattr(a, name), getattr(b, name)), name
    assert int(forecast._ticket(DEV).item()) == 0
    empty = ForecastPool(pl.preds[:, :0], pl.kind, u=pl.u, xi=pl.xi)
    assert empty.cdf(x).shape == (0, 5) and empty.quantile([0.5]).shape == (0, 1)
    sc = empty.score(y[:0], x)
    assert torch.isnan(sc.brier).all() and float(sc.valid[0]) == 0.0
    assert pl.cdf(np.zeros(0)).shape == (n, 0)
    twice = np.concatenate([params[:, :1], params[:, :1]], axis=1)
    pl2, _ = PC.build(kind, xi, twice, DEV)
    v = pl2.score(torch.tensor([0.3, 4.0])).diversity_rows
    assert PC.same_bits(v[0:1], v[1:2]) and float(v[0]) > 0.0


@pytest.mark.parametrize("kind,xi", [("normal", None), ("mixed_normal", None), ("mixed", 0.5),
                                     ("mixed_u", 0.2)])
def test_weights(kind, xi):
    PC.check_weights(kind, xi, DEV)


@pytest.mark.parametrize("kind,xi", PC.KIND_XI)
@pytest.mark.parametrize("M", [3, 7])
def test_kernels_match_the_torch_path(kind, xi, M):
    """The kernels against the package's torch formulation on the CPU, same inputs: crps and
    diversity within 1e-12 x the largest |crps row|; probabilities at forecast_cases' bounds;
    quantiles in probability space (each path ends on adjacent doubles of its own Fbar)."""
    n = 65
    params = PC.members(kind, n, M)
    gpu, orc = PC.build(kind, xi, params, DEV)
    cpu, _ = PC.build(kind, xi, params, "cpu")
    x = PC.thresholds(kind, params, 9)
    y = FC.make_targets(n, seed=6)
    a, b = gpu.score(torch.from_numpy(y), x), cpu.score(torch.from_numpy(y), x)
    ok = ~np.isnan(y)
    scale = np.abs(b.crps_rows.numpy()[ok]).max()
    err_c = np.abs(a.crps_rows.cpu().numpy() - b.crps_rows.numpy())[ok].max() / scale
    err_v = np.abs(a.diversity_rows.cpu().numpy() - b.diversity_rows.numpy()).max() / scale
    err_f = (gpu.cdf(x).cpu() - cpu.cdf(x)).abs().max().item()
    print(f"{kind} xi={xi} M={M}: crps {err_c:.1e}, diversity {err_v:.1e} of scale, F {err_f:.1e}")
    assert err_c <= 1e-12 and err_v <= 1e-12 and err_f <= 1e-13
    q = np.linspace(0.05, 0.95, 7)
    free = q[None, :] > orc.P_c * (1 + 1e-12) if orc.atom else np.ones((n, 7), dtype=bool)
    for pl in (gpu, cpu):
        assert np.abs(orc.cdf(pl.quantile(q).cpu().numpy()) - q[None, :])[free].max() <= 1e-12


def test_more_than_32_members_take_the_torch_formulation_on_the_device():
    params = PC.members("mixed", 5, 33)
    pl, orc = PC.build("mixed", 0.5, params, DEV)
    assert not pl.on_kernel
    x = PC.thresholds("mixed", params, 5)
    PC.check_prob(pl, orc, x)
    PC.check_score(pl, orc, FC.make_targets(5, seed=1), x)
