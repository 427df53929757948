"""CPU: fitting the pool's weights.  ``ForecastPool.pair_sums`` on the package's
fp64 torch path against the mpmath fixture tests/golden/pool_pair_rows.npz and the shipped
``score`` (checks and bounds in tests/pool_fit_cases.py; tests/test_gpu_pool_fit.py runs the
same on the kernel); the host solver ``solve_pool_weights``; ``fit_weights`` with its
cross-validation, ``reweighted``, ``evaluate.fit_pool``; the C ABI of ``gine_pool_pairs`` /
``gine_pool_pairs_partials`` and their host validation without a device.

Measured (this path, printed with -s): pair distances against the fixture 4.4e-16 of a case's
largest entry (bound 1e-11); the identity c . w - 1/2 w' D w against ``score`` 1.5e-16 of count x
the largest row (bound 1e-11); the solver's Frank-Wolfe gap over the 300 random cases at most
7.4e-16 max|c| (it stops at 1e-12), 9 steps at the most.
"""
import ctypes
import os
import re
from math import erf

import numpy as np
import pytest
import torch

import forecast_cases as FC
import pool_cases as PC
import pool_fit_cases as PF
from conftest import ROOT
from raincast_gnn import _lib, pool
from raincast_gnn.pool import ForecastPool, solve_pool_weights

NAMES = ("gine_pool_pairs_partials", "gine_pool_pairs")


def objective(c, D, w):
    return float(c @ w - 0.5 * (w @ (D @ w)))


# ---------------------------------------------------------------------------------------
# pair_sums, the torch path
# ---------------------------------------------------------------------------------------
def test_pair_distances_match_the_mpmath_fixture():
    print(f"torch path, worst over the fixture: {PF.check_fixture('cpu'):.2e}")


@pytest.mark.parametrize("kind,xi", PF.KIND_XI)
@pytest.mark.parametrize("M", [1, 3, 7])
def test_identity_with_the_shipped_score(kind, xi, M):
    print(f"{kind} xi={xi} M={M}: {PF.check_identity(kind, xi, 13, M, 'cpu'):.2e} of count x row")


@pytest.mark.parametrize("kind,xi", PF.KIND_XI)
def test_exact_zeros_symmetry_and_permutations(kind, xi):
    PF.check_zeros_and_symmetry(kind, xi, 13, 5, "cpu")


@pytest.mark.parametrize("kind,xi", [("normal", None), ("mixed", 0.5), ("mixed_u", 0.2)])
@pytest.mark.parametrize("n", [1, 70])
def test_segments(kind, xi, n):
    print(f"{kind} xi={xi} n={n}: segments against one {PF.check_segments(kind, xi, n, 3, 'cpu'):.2e}")


def test_missing_targets_and_determinism():
    PF.check_missing("mixed_u", 0.5, 9, 3, "cpu")
    PF.check_determinism("mixed_u", 0.5, 70, 3, "cpu")


def test_diversity_is_unchanged_by_the_shared_nodes():
    """diversity() reads the nodes that pair_sums reads: V = 1/2 w' D w row by row."""
    params = PC.members("mixed", 6, 4)
    pl = PF.make_pool("mixed", 0.5, params, "cpu", weights=[0.4, 0.3, 0.2, 0.1])
    V = pl.diversity().numpy()
    ps = pl.pair_sums(torch.zeros(6), np.arange(7))
    w = pl.weights.numpy()
    quad = 0.5 * np.einsum("m,gml,l->g", w, ps.distance.numpy(), w)
    assert np.abs(quad - V).max() <= 1e-13 * np.abs(V).max()


def test_folds_are_validated():
    pl = PF.make_pool("normal", None, PC.members("normal", 10, 2), "cpu")
    y = torch.zeros(10)
    for bad in ([1, 10], [0, 6, 4, 10], [0, 5, 9], [0], 0, -2, [0.0, 10.0], np.zeros((2, 2), int),
                torch.tensor([0, 10], dtype=torch.int32)):
        with pytest.raises(ValueError):
            pl.pair_sums(y, bad)
    with pytest.raises(ValueError):
        pl.pair_sums(torch.zeros(9))
    assert pl.pair_sums(y, [0, 10]).count.tolist() == [10.0]
    assert pl.pair_sums(y, 4).count.tolist() == [3.0, 3.0, 3.0, 1.0]   # ceil(10 / 4) = 3
    assert pl.pair_sums(y, 7).count.tolist() == [2.0] * 5 + [0.0, 0.0]  # the last ones empty


# ---------------------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------------------
def test_solver_small_cases():
    w, info = solve_pool_weights([3.0], [[0.0]])
    assert w.tolist() == [1.0] and info["support"] == [0] and info["gap"] == 0.0
    for c1, c2, d in ((1.0, 1.2, 0.5), (1.0, 1.2, 0.1), (2.0, 1.0, 0.3), (1.0, 1.0, 0.4)):
        w, info = solve_pool_weights([c1, c2], [[0.0, d], [d, 0.0]])
        # weight of the first member: d/dw of c1 w + c2 (1 - w) - d w (1 - w)
        want = min(max(0.5 + (c2 - c1) / (2.0 * d), 0.0), 1.0)
        # d (w - want)^2 is the objective above its minimum, which the gap bounds; and the
        # method ends on an exact solve of a system of condition <= 1e3: 1e3 x 2^-52 < 1e-12
        assert abs(w[0] - want) <= np.sqrt(info["gap"] / d) + 1e-15, (w, want)
        assert abs(w[0] - want) <= 1e-12, (w, want)
        assert objective(np.array([c1, c2]), np.array([[0.0, d], [d, 0.0]]), w) - \
            (c1 * want + c2 * (1 - want) - d * want * (1 - want)) <= 1e-15 * max(c1, c2)
        assert abs(w.sum() - 1.0) <= 1e-15 and (w >= 0.0).all()
    # a dominated member: far from both others and worse than either
    c = np.array([1.0, 1.1, 5.0])
    D = np.array([[0.0, 0.4, 0.5], [0.4, 0.0, 0.5], [0.5, 0.5, 0.0]])
    w, info = solve_pool_weights(c, D)
    assert w[2] == 0.0 and info["support"] == [0, 1]
    assert abs(w[0] - 0.625) <= np.sqrt(info["gap"] / 0.4) + 1e-15 and abs(w[0] - 0.625) <= 1e-12
    # duplicated members: a singular system on the support
    c = np.array([1.0, 1.1, 1.0, 1.1])
    D = np.array([[0.0, 0.4, 0.0, 0.4], [0.4, 0.0, 0.4, 0.0], [0.0, 0.4, 0.0, 0.4],
                  [0.4, 0.0, 0.4, 0.0]])
    w, info = solve_pool_weights(c, D)
    assert info["gap"] <= 1e-12 * 1.1 and (w >= 0.0).all() and abs(w.sum() - 1.0) <= 1e-15
    assert abs(w[0] + w[2] - 0.625) <= np.sqrt(info["gap"] / 0.4) + 1e-15
    assert abs(w[0] + w[2] - 0.625) <= 1e-12
    with pytest.raises(ValueError):
        solve_pool_weights([1.0, np.nan], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        solve_pool_weights([], np.zeros((0, 0)))


def _random_case(seed):
    """c and D of M normal members at n targets, integrated on a grid; every third case has a
    duplicated member."""
    r = np.random.default_rng(seed)
    M, n = int(r.integers(1, 33)), 12
    x = np.linspace(-12.0, 12.0, 801)
    mu, sg = r.normal(0.0, 1.0, (M, n)), np.exp(r.normal(0.0, 0.4, (M, n)))
    if seed % 3 == 0 and M > 1:
        k = int(r.integers(1, M))
        mu[k], sg[k] = mu[0], sg[0]
    y = r.normal(0.0, 1.5, n)
    F = 0.5 * (1.0 + np.vectorize(erf)((x - mu[..., None]) / sg[..., None] / np.sqrt(2.0)))
    H = (x >= y[None, :, None]).astype(np.float64)
    dx = x[1] - x[0]
    return ((F - H) ** 2).sum((1, 2)) * dx, ((F[:, None] - F[None]) ** 2).sum((2, 3)) * dx


def test_solver_random_cases():
    worst, steps = 0.0, 0
    for seed in range(300):
        c, D = _random_case(seed)
        M = c.size
        w, info = solve_pool_weights(c, D)
        again, _ = solve_pool_weights(c, D)
        assert np.array_equal(w, again)
        assert (w >= 0.0).all() and abs(w.sum() - 1.0) <= 1e-15
        assert info["support"] == [int(i) for i in np.flatnonzero(w > 0)]
        g = c - D @ w
        gap = float(g @ w - g.min())
        assert info["gap"] == gap and gap <= 1e-12 * np.abs(c).max(), (seed, gap)
        o = objective(c, D, w)
        assert o <= objective(c, D, np.full(M, 1.0 / M)) and o <= c.min()   # every vertex
        worst, steps = max(worst, gap / np.abs(c).max()), max(steps, info["iterations"])
    print(f"300 cases: worst gap {worst:.2e} max|c|, at most {steps} steps")


def test_solver_close_members_under_a_large_common_score():
    """Checkpoints of one run: a common CRPS far above the distances between them (a season of
    rows: c about 1e3 times the entries of D).  The step is solved from the gradient, so the
    solve's rounding, which scales with |c|, does not limit the gap."""
    for seed in range(40):
        c, D = _random_case(seed)
        c = c + 2000.0 * max(float(D.max()), 1.0)
        w, info = solve_pool_weights(c, D)
        assert info["gap"] <= 1e-12 * np.abs(c).max(), (seed, info)
        assert (w >= 0.0).all() and abs(w.sum() - 1.0) <= 1e-15


# ---------------------------------------------------------------------------------------
# fit_weights, reweighted
# ---------------------------------------------------------------------------------------
def _close_members(kind, n, M, seed=0):
    """Checkpoints a few tenths of sigma around one forecast: pools that do mix."""
    base = FC.make_params(kind, n, seed=seed).astype(np.float64)
    r = np.random.default_rng(900 + seed)
    out = np.repeat(base[None], M, 0)
    out[:, :, 0] += 0.5 * r.normal(0.0, 1.0, (M, n)) * base[None, :, 1]
    out[:, :, 1] *= np.exp(0.3 * r.normal(0.0, 1.0, (M, n)))
    return out.astype(np.float32)


@pytest.mark.parametrize("kind,xi", [("normal", None), ("mixed", 0.5), ("mixed_u", 0.8)])
def test_fit_weights(kind, xi):
    n, M = 60, 5
    params = _close_members(kind, n, M)
    y = FC.make_targets(n, seed=21)
    pl = PF.make_pool(kind, xi, params, "cpu")
    fit = pl.fit_weights(torch.from_numpy(y))
    assert fit.cv_weights is None and fit.cv_crps is None
    assert fit.count == (~np.isnan(y)).sum()
    assert (fit.weights >= 0.0).all() and abs(fit.weights.sum() - 1.0) <= 1e-15
    assert fit.crps <= fit.crps_equal and fit.crps <= fit.crps_members.min()
    assert fit.gap <= 1e-12 * np.abs(fit.crps_members).max() * fit.count
    assert fit.distance.shape == (M, M) and fit.crps_members.shape == (M,)
    assert len(fit.support) >= 2, "the case should mix members"
    fitted = pl.reweighted(fit.weights)
    assert fitted.num_members == len(fit.support)
    sc = fitted.score(torch.from_numpy(y))
    rows = sc.crps_rows.numpy()[~np.isnan(y)]
    err = abs(float(sc.crps) - fit.crps) / np.abs(rows).max()
    print(f"{kind}: weights {np.round(fit.weights, 4)}, crps {fit.crps:.6f} (1/M "
          f"{fit.crps_equal:.6f}), refit score {err:.1e} of the largest row")
    assert err <= 1e-11
    with pytest.raises(ValueError):
        pl.reweighted([1.0, 0.0])
    with pytest.raises(ValueError):
        pl.reweighted([0.5, 0.6, -0.1, 0.0, 0.0])
    with pytest.raises(ValueError):
        pl.reweighted(np.zeros(M))
    one = pl.reweighted([0.0, 0.0, 2.0, 0.0, 0.0])
    assert one.num_members == 1 and torch.equal(one.preds[0], pl.preds[2])


@pytest.mark.parametrize("kind,xi", [("mixed_normal", None), ("mixed", 0.5)])
def test_cross_validation(kind, xi):
    n, M, K = 90, 4, 3
    params = _close_members(kind, n, M, seed=1)
    y = FC.make_targets(n, seed=22)
    ok = ~np.isnan(y)
    pl = PF.make_pool(kind, xi, params, "cpu")
    fit = pl.fit_weights(torch.from_numpy(y), folds=K)
    plain = pl.fit_weights(torch.from_numpy(y))
    assert abs(fit.crps - plain.crps) <= (fit.gap + plain.gap) / fit.count + 1e-13 * fit.crps
    assert fit.cv_weights.shape == (K, M)
    size = n // K
    held = 0.0
    scale = 0.0
    for g in range(K):
        rest = np.r_[0:g * size, (g + 1) * size:n]
        sub = PF.make_pool(kind, xi, params[:, rest], "cpu")
        ref = sub.fit_weights(torch.from_numpy(y[rest]))
        ps = sub.pair_sums(torch.from_numpy(y[rest]))
        c, D = ps.member_crps[0].numpy(), ps.distance[0].numpy()
        wg = fit.cv_weights[g]
        gg = c - D @ wg
        gap_g = float(gg @ wg - gg.min())                    # cv_weights[g] on the explicit rows
        assert abs(objective(c, D, wg) - objective(c, D, ref.weights)) <= gap_g + ref.gap + \
            1e-13 * np.abs(c).max()
        fold = slice(g * size, (g + 1) * size)
        sc = PF.make_pool(kind, xi, params[:, fold], "cpu").reweighted(wg) \
            .score(torch.from_numpy(y[fold]))
        rows = sc.crps_rows.numpy()[ok[fold]]
        held += rows.sum()
        scale = max(scale, np.abs(rows).max())
    assert fit.cv_crps >= fit.crps
    err = abs(held / fit.count - fit.cv_crps) / scale
    print(f"{kind}: crps {fit.crps:.6f}, held out {fit.cv_crps:.6f} (1/M {fit.cv_crps_equal:.6f}); "
          f"against per-fold scores {err:.1e} of the largest row")
    assert err <= 1e-11
    assert abs(fit.cv_crps_equal - fit.crps_equal) <= 1e-13 * fit.crps_equal
    # a fold whose complement has no target
    lone = np.full(n, np.nan, dtype=np.float32)
    lone[3] = 0.5
    with pytest.raises(ValueError):
        pl.fit_weights(torch.from_numpy(lone), folds=K)
    assert pl.fit_weights(torch.from_numpy(lone)).count == 1.0


# ---------------------------------------------------------------------------------------
# ABI and host validation
# ---------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_pair_entry_points():
    import raincast_gnn
    assert raincast_gnn.PoolFit is pool.PoolFit and raincast_gnn.PairSums is pool.PairSums
    text = open(os.path.join(ROOT, "include", "gine_hip.h")).read()
    assert re.search(r"#define GINE_ABI_VERSION 10\b", text)
    lib = _lib.load()
    assert lib.gine_abi_version() == 10 and _lib.ABI_VERSION == 10
    for name in NAMES:
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, text, re.M)
        assert m, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name]) == m.group(1).count(",") + 1, name


def test_pair_entry_points_validate_without_a_device():
    """Every rejection comes before any HIP call; N = 0 is ok and launches nothing."""
    lib = _lib.load()
    MIXED, c, u = _lib.LOSS_MIXED, FC.C, FC.U_FIXED
    one = ctypes.c_void_p(8)  # never dereferenced on these paths

    def pairs(M=3, N=0, kind=MIXED, u=u, xi=0.5, G=1):
        return lib.gine_pool_pairs(one, one, M, N, kind, u, xi, c, one, one, one, G,
                                   *([one] * 5), None)

    assert pairs() == _lib.GINE_OK
    for M in (0, -1, 33):
        assert pairs(M=M) == _lib.GINE_ERR_INVALID, M
    assert pairs(M=1) == _lib.GINE_OK and pairs(M=32) == _lib.GINE_OK
    for G in (0, -1):
        assert pairs(G=G) == _lib.GINE_ERR_INVALID, G
    assert pairs(G=7) == _lib.GINE_OK
    assert pairs(N=-1) == _lib.GINE_ERR_INVALID
    assert pairs(N=2 ** 31) == _lib.GINE_ERR_TOO_LARGE
    assert pairs(G=2 ** 31) == _lib.GINE_ERR_TOO_LARGE
    assert pairs(kind=9) == _lib.GINE_ERR_INVALID and pairs(kind=-1) == _lib.GINE_ERR_INVALID
    assert pairs(xi=1.0) == _lib.GINE_ERR_INVALID and pairs(xi=0.0) == _lib.GINE_ERR_INVALID
    assert pairs(u=c) == _lib.GINE_ERR_INVALID
    assert pairs(kind=_lib.LOSS_MIXED_U, u=c) == _lib.GINE_OK  # u is per row there
    count = ctypes.c_size_t(0)
    size = lib.gine_pool_pairs_partials
    assert size(130, 3, 4, ctypes.byref(count)) == _lib.GINE_OK
    assert count.value == (130 // 64 + 4) * (1 + 3 + 3)       # a record per tile
    assert size(89060, 32, 1, ctypes.byref(count)) == _lib.GINE_OK
    assert count.value == (89060 // 64 + 1) * 529              # nothing per row
    assert size(0, 1, 1, ctypes.byref(count)) == _lib.GINE_OK and count.value == 2
    for bad in ((-1, 3, 1), (5, 0, 1), (5, 33, 1), (5, 3, 0)):
        assert size(*bad, ctypes.byref(count)) == _lib.GINE_ERR_INVALID, bad
    assert size(5, 3, 1, None) == _lib.GINE_ERR_INVALID
    assert size(2 ** 31, 3, 1, ctypes.byref(count)) == _lib.GINE_ERR_TOO_LARGE


# ---------------------------------------------------------------------------------------
# evaluate
# ---------------------------------------------------------------------------------------
def test_evaluate_fit_pool():
    from types import SimpleNamespace

    from oracle import gine_cpu as O
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.evaluate import fit_pool, predict_ensemble, verify_pool

    def toy():
        return O.OracleGNN(35, 32, 2, "MixedLoss", "False", 1.71, 0.5)

    batches = [synthetic_batch(20, 2, k=4, seed=s) for s in (3, 4)]
    torch.manual_seed(1)
    base = {k: v.detach().clone() for k, v in toy().state_dict().items()}
    states = []
    for seed in (1, 2, 3):                                   # three perturbed checkpoints
        g = torch.Generator().manual_seed(seed)
        states.append({k: v + 0.05 * torch.randn(v.shape, generator=g) * v.abs()
                       if v.is_floating_point() else v.clone() for k, v in base.items()})
    stacked = predict_ensemble(toy, states, batches, "cpu", stack=True)
    model = SimpleNamespace(loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)  # a params.json
    targets = torch.cat([b.y for b in batches]).float().reshape(-1)
    targets[5] = float("nan")
    fit, fitted = fit_pool(model, stacked, targets, folds=4)
    assert isinstance(fit, pool.PoolFit) and isinstance(fitted, ForecastPool)
    assert fit.cv_weights.shape == (4, 3) and fitted.num_members == len(fit.support)
    v = verify_pool(model, stacked, targets, [1.0])
    assert abs(fit.crps_equal - float(v.pool_crps)) <= 1e-12 * float(v.pool_crps)
    assert float(fitted.score(targets).crps) <= float(v.pool_crps)
    assert fit.cv_crps >= fit.crps
