"""Seeded score grids and the checks of raincast_gnn.compare against tests/compare_oracle.py,
shared by the CPU tests (the package's numpy formulation) and the GPU tests (the kernels): the
same properties at the same bounds on either device.

Scores are positive and gamma-like (a CRPS in model space), b a noisy copy of a so that skills
are of either sign.  RAGGED is T = 37 days x S = 70 stations: a is 7 % missing and b 5 %,
station 5 is entirely missing in a and day 11 entirely missing.  WIDE(T) is the same recipe at
130 stations (three wavefronts of stations, the last partial) for T in {1, 2, 37}; narrower
cases are its leading columns and fewer replicates its leading rows, which the contract makes
the same bits (all stations of a replicate see the same days; row i is replicate rep_first + i).

Bounds: replicate sums, station sums, n, dbar and var bit for bit (the contract fixes every
operation); diff, skill and stat within 4 * 2^-52 relative (two or three correctly rounded
operations on equal inputs); p within 1e-11 relative where the oracle's p >= 1e-300 and
<= 1e-300 otherwise (tests/forecast_cases.py's bound for erfc-built probabilities: erfc's
relative condition number |x erfc'(x) / erfc(x)| ~ 2 x^2 reaches ~1400 at p = 1e-300, times a
few ulps of the argument and of erfc itself); day sums within (S - 1) * 2^-53 * sum|x| of
math.fsum, which holds for any order of S adds.
"""
import functools

import numpy as np
import torch

import compare_oracle as CO

SEED = 7            # generator seed of the tested replicates
R = 257             # replicates of a reference: one past the kernel's replicate tile of 256
BLOCK_LENS = (1, 5, 36, 37)
LAGS = (0, 1, 4, 36)
REL = 4.0 * 2.0 ** -52
P_REL, P_TINY = 1e-11, 1e-300


def make_grid(T, S, rng_seed):
    r = np.random.default_rng(rng_seed)
    a = r.gamma(2.0, 0.4, (T, S)) + 0.05
    b = a * np.exp(r.normal(0.05, 0.3, (T, S))) + 0.3 * r.gamma(1.0, 0.2, (T, S))
    a[r.random((T, S)) < 0.07] = np.nan
    b[r.random((T, S)) < 0.05] = np.nan
    if S > 5:
        a[:, 5] = np.nan
    if T > 11:
        a[11, :] = np.nan
        b[11, :] = np.nan
    for v in (a, b):
        v.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def ragged():
    return make_grid(37, 70, 3)


@functools.lru_cache(maxsize=None)
def wide(T):
    return make_grid(T, 130, 4 + T)


def grid(name):
    """'ragged' or ('wide', T) -> (a, b)."""
    return ragged() if name == "ragged" else wide(name[1])


@functools.lru_cache(maxsize=None)
def reference(name, L, rep_first=0, replicates=R):
    """The oracle's replicate sums of a whole grid, computed once (read-only)."""
    a, b = grid(name)
    ref = CO.bootstrap(a, b, None, L, SEED, rep_first, replicates)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def dm_reference(name, h):
    a, b = grid(name)
    ref = CO.dm(a, b, h)
    ref.setflags(write=False)
    return ref


def _check_design():
    """RAGGED at the tested (seed, R, L): no replicate leaves a station other than 5 without a
    valid pair (so NaN replicates come from station 5 alone), and some block wraps past the
    last day (so the circular step is exercised)."""
    a, b = ragged()
    T = a.shape[0]
    ok = CO.valid(a, b).astype(np.int64)
    assert not ok[:, 5].any() and not ok[11].any()
    for L in BLOCK_LENS:
        wraps = False
        for r in range(R):
            days = CO.draws(SEED, r, T, L)
            counts = ok[days].sum(0)
            assert (np.delete(counts, 5) > 0).all(), (L, r)
            nb = CO.num_blocks(T, L)
            wraps |= any(CO.start(SEED, r, j, T, L) + min(L, T - j * L) > T for j in range(nb))
        assert wraps or L == 1, L  # a block of one day cannot wrap


_check_design()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(got, ref):
    """Equal bit patterns; a NaN matches any NaN (0 / 0 has the sign bit set on x86 only)."""
    got, ref = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(ref))
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return False
    keep = ~np.isnan(ref)
    return np.array_equal(got[keep].view(np.int64), ref[keep].view(np.int64))


def assert_close(got, ref, rel, what):
    """NaN and infinities in the same places, the rest within `rel` relative."""
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin] - ref[fin])
    worst = float((err / np.maximum(np.abs(ref[fin]), 1e-300)).max()) if err.size else 0.0
    print(f"  {what}: worst relative error {worst:.2e} (bound {rel:.2e})")
    assert np.all(err <= rel * np.abs(ref[fin])), (what, worst)


def check_sums(got, ref, rows=slice(None), cols=slice(None)):
    """Replicate results (a dict by field, [R', S']) against rows / cols of the oracle's."""
    for k in ("sum_a", "sum_b", "sum_w"):
        if k in got:
            assert same_bits(got[k], ref[k][rows, cols]), k
    for k in ("diff", "skill"):
        if k in got:
            assert_close(got[k], ref[k][rows, cols], REL, k)


def check_dm(got, ref, cols=slice(None)):
    """DM results (a dict by field, [S']) against the oracle's [5, S]."""
    n, dbar, var, stat, p = (ref[i][cols] for i in range(5))
    assert same_bits(got["n"], n)
    for k, v in (("mean_d", dbar), ("var", var)):
        g = _np(got[k])
        assert np.array_equal(np.isnan(g), np.isnan(v)), k
        assert same_bits(g[~np.isnan(v)], v[~np.isnan(v)]), k
    assert_close(got["stat"], stat, REL, "stat")
    gp = _np(got["pvalue"])
    assert np.array_equal(np.isnan(gp), np.isnan(p))
    big = p >= P_TINY  # False for NaN
    assert np.all(np.abs(gp[big] - p[big]) <= P_REL * p[big]), "p"
    small = ~np.isnan(p) & ~big
    assert np.all(gp[small] <= P_TINY), "tiny p"


def check_marginals(got, a, b):
    """Station sums bit for bit against the sequential oracle, day sums against math.fsum."""
    S = a.shape[1]
    st = CO.station_sums(a, b)
    for i, k in enumerate(("station_a", "station_b", "station_n")):
        assert same_bits(got[k], st[i]), k
    da, db, dn, abs_a, abs_b = CO.day_sums_exact(a, b)
    assert same_bits(got["day_n"], dn)
    for k, exact, mag in (("day_a", da, abs_a), ("day_b", db, abs_b)):
        err = np.abs(_np(got[k]) - exact)
        assert np.all(err <= (S - 1) * 2.0 ** -53 * mag), (k, float(err.max()))


def on(device, *arrays):
    return [None if v is None else torch.from_numpy(np.array(v)).to(device) for v in arrays]
