"""Seeded inputs and checks shared by tests/test_reliability.py (CPU, the numpy formulation) and
tests/test_gpu_reliability.py (the kernels of csrc/gine_reliability.hip), held to
tests/reliability_oracle.py.

Bounds.  The contract fixes every operation, so every field is held to the
oracle bit for bit: the integers (counts, blocks, block ids, number of blocks, A2, e*) and the
fp64 fields (v, cal, S, S_cal, UNC, MCB, DSC, AUC, cal*, S*, S*_cal, MCB*, p_value); NaN
positions must agree (a NaN's own bits are not part of the contract).  Two checks are bounds
rather than equalities and carry their derivation where they are made: S against the Brier
score of the unquantised p (1/q), and S against MCB - DSC + UNC and the exact sum (8 * 2^-52
relative).

Shapes: N in {0, 1, 63, 64, 65, 300, 1031} (below, at and past a wavefront, past a workgroup
round of 256 rows, no multiple of anything), T in {1, 3}, q in {1, 11, 64, 100, 4096}; the
ordered cases have 144, 4,225 (more than one workgroup of the counts kernel) and 10,201 rows.
"""
import functools

import numpy as np
import torch

import reliability_oracle as RO

SEED = 20211
REP_FIRST = 7  # the second call's odd offset

# name -> (N, T, q, seed)
MIXED = {
    "n0_t1_q11": (0, 1, 11, 1), "n0_t3_q1": (0, 3, 1, 2), "n1_t1_q1": (1, 1, 1, 3),
    "n1_t3_q4096": (1, 3, 4096, 4), "n63_t3_q11": (63, 3, 11, 5), "n64_t1_q64": (64, 1, 64, 6),
    "n65_t3_q100": (65, 3, 100, 7), "n300_t3_q11": (300, 3, 11, 8),
    "n300_t1_q4096": (300, 1, 4096, 9), "n1031_t3_q64": (1031, 3, 64, 10),
    "n1031_t3_q100": (1031, 3, 100, 11), "n1031_t1_q1": (1031, 1, 1, 12),
    "n1031_t3_q4096": (1031, 3, 4096, 13),
}
ORDERED = ("no_events", "all_events", "all_tied", "monotone_q11", "anti_q11", "monotone_q64",
           "anti_q64", "anti_q100")
NAMES = tuple(MIXED) + ORDERED

# the design check: 3,000 rows, p ~ Beta(0.6, 2), q = 100, R = 199; the seeds were chosen so
# that the oracle alone gives p_value >= 0.05 for the outcomes drawn from p and 1 / (R + 1) for
# the same outcomes against sqrt(p).  Data seeds 11, 12 and 13 with resampling seed 0 gave the
# oracle 0.8, 0.565 and 0.145 for the first and 0.005 for the second every time; 11 is kept.
DESIGN = dict(rows=3000, q=100, R=199, data_seed=11, seed=0)
DESIGN_P = (0.8, 0.005)  # the oracle's two p-values (160 / 200 and 1 / 200)


def mixed(N: int, T: int, q: int, seed: int):
    """Probabilities on and off the lattice: exact 0 and 1, the half-way points (k + 0.5) / q,
    NaN, -0.1 and 1.5; outcomes with NaN; with T = 3 one NaN threshold (even seeds) or one
    column entirely invalid (odd seeds), and columns of differing valid counts."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, q + 1, (N, T))
    p = k / np.float64(q)
    kind = rng.random((N, T))
    half = (np.minimum(k, q - 1) + 0.5) / np.float64(q)
    p = np.where(kind < 0.25, half, p)
    p = np.where((kind >= 0.25) & (kind < 0.45), rng.random((N, T)), p)
    p = np.where((kind >= 0.45) & (kind < 0.50), 0.0, p)
    p = np.where((kind >= 0.50) & (kind < 0.55), 1.0, p)
    p = np.where((kind >= 0.55) & (kind < 0.58), np.nan, p)
    p = np.where((kind >= 0.58) & (kind < 0.61), -0.1, p)
    p = np.where((kind >= 0.61) & (kind < 0.64), 1.5, p)
    y = rng.normal(0.3, 1.0, N).astype(np.float32)
    y[rng.random(N) < 0.1] = np.nan
    x = np.array([0.25, 0.5, 1.0][:T], dtype=np.float64)
    if T == 3:
        p[:, 2] = np.where(rng.random(N) < 0.4, np.nan, p[:, 2])  # fewer valid cells
        if seed % 2 == 0:
            x[1] = np.nan
        else:
            p[:, 1] = np.where(rng.random(N) < 0.5, np.nan, 2.0)
    return np.ascontiguousarray(p, dtype=np.float64), y, x


def ordered(name: str):
    """Outcomes in a chosen order against probabilities k / q, one column, threshold 0."""
    x = np.array([0.0])
    if name in ("no_events", "all_events", "all_tied"):
        rng = np.random.default_rng(31)
        q, N = 11, 300
        p = rng.integers(0, q + 1, (N, 1)) / np.float64(q)
        y = np.full(N, 1.0 if name == "all_events" else -1.0, dtype=np.float32)
        if name == "all_tied":
            p[:] = 0.3
            y = np.where(rng.random(N) < 0.3, 1.0, -1.0).astype(np.float32)
        return p, y, x, q
    q = int(name.split("_q")[1])
    K = q + 1
    # level k has K cells, k of them events (monotone: K strictly increasing means, no merge,
    # K blocks) or q - k (anti: strictly decreasing, everything merges: the deepest pop chain)
    lev = np.repeat(np.arange(K), K)
    within = np.tile(np.arange(K), K)
    events = lev if name.startswith("monotone") else q - lev
    y = np.where(within < events, 1.0, -1.0).astype(np.float32)
    order = np.random.default_rng(q).permutation(K * K)
    return (lev[order] / np.float64(q)).reshape(-1, 1), y[order], x, q


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (p [N, T] float64, y [N] float32, x [T] float64, q)."""
    if name in MIXED:
        N, T, q, seed = MIXED[name]
        return (*mixed(N, T, q, seed), q)
    return ordered(name)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The oracle's counts and fits of a case: (n_k, e_k, level, fits [T])."""
    p, y, x, q = case(name)
    n_k, e_k, level = RO.counts(p, y, x, q)
    return n_k, e_k, level, [RO.fit(n_k[t], e_k[t], q) for t in range(p.shape[1])]


@functools.lru_cache(maxsize=None)
def reference_replicates(name: str, rep_first: int, R: int):
    """-> (e_rep [R][T][K], fits [R][T])."""
    n_k, _, level, _ = reference(name)
    q = case(name)[3]
    return RO.resample(level, n_k, q, SEED, rep_first, R)


@functools.lru_cache(maxsize=None)
def design_inputs():
    """-> (p [N, 1], sqrt(p), y, x): outcomes drawn from p."""
    rng = np.random.default_rng(DESIGN["data_seed"])
    N = DESIGN["rows"]
    p = rng.beta(0.6, 2.0, (N, 1))
    y = np.where(rng.random(N) < p[:, 0], 1.0, -1.0).astype(np.float32)
    return p, np.sqrt(p), y, np.array([0.0])


@functools.lru_cache(maxsize=None)
def design_reference(which: int):
    """The oracle's (MCB, MCB* [R], p_value) of the reliable (0) or the sqrt (1) forecast."""
    inputs = design_inputs()
    p, y, x = inputs[which], inputs[2], inputs[3]
    q, R = DESIGN["q"], DESIGN["R"]
    n_k, e_k, level = RO.counts(p, y, x, q)
    f = RO.fit(n_k[0], e_k[0], q)
    _, fits = RO.resample(level, n_k, q, DESIGN["seed"], 0, R)
    mcb_rep = [fits[r][0]["MCB"] for r in range(R)]
    return f["MCB"], mcb_rep, RO.p_value(f["MCB"], mcb_rep)


# ---------------------------------------------------------------------------------- checks
def on(device, p, y, x):
    return (torch.from_numpy(p).to(device), torch.from_numpy(y).to(device),
            torch.from_numpy(x).to(device))


def same_bits(got, want) -> bool:
    """Equal shapes, NaN at the same places and the same bits everywhere else."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, dtype=got.dtype).reshape(got.shape) if np.size(want) == got.size \
        else np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(got)
        if not np.array_equal(nan, np.isnan(want)):
            return False
        return np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))
    return np.array_equal(got, want)


def check_counts(counts, name: str, columns=slice(None)):
    n_k, e_k, level, _ = reference(name)
    got_n, got_e, got_level = counts
    assert got_n.dtype == torch.int32 and got_level.dtype == torch.int16
    K = case(name)[3] + 1
    N = case(name)[0].shape[0]
    assert same_bits(got_n, np.array(n_k[columns], dtype=np.int32).reshape(-1, K)), name
    assert same_bits(got_e, np.array(e_k[columns], dtype=np.int32).reshape(-1, K)), name
    assert same_bits(got_level, np.array(level[columns], dtype=np.int16).reshape(len(level[columns]), N)), name


def check_fit(fit, name: str, columns=slice(None)):
    fits = reference(name)[3][columns]
    q = case(name)[3]
    K = q + 1
    T = len(fits)
    assert fit.cal.shape == (T, K) and fit.stats.shape == (T, 8)
    assert same_bits(fit.v, [RO.value(k, q) for k in range(K)])
    for t, f in enumerate(fits):
        where = f"{name} column {t}"
        assert same_bits(fit.cal[t], f["cal"]), where
        assert same_bits(fit.block_id[t], np.array(f["block_id"], dtype=np.int32)), where
        nb = len(f["blocks"])
        assert int(fit.num_blocks[t]) == nb, where
        be = [b[0] for b in f["blocks"]] + [0] * (K - nb)
        bn = [b[1] for b in f["blocks"]] + [0] * (K - nb)
        assert same_bits(fit.block_e[t], np.array(be, dtype=np.int32)), where
        assert same_bits(fit.block_n[t], np.array(bn, dtype=np.int32)), where
        assert int(fit.a2[t]) == f["a2"], where
        got = fit.stats[t].cpu().numpy()
        for j, field in enumerate(("n", "E", "S", "S_cal", "UNC", "MCB", "DSC", "AUC")):
            assert same_bits(got[j:j + 1], [f["stats"][j]]), (where, field, got[j], f[field])
        assert same_bits(getattr(fit, "MCB")[t:t + 1], [f["MCB"]])


def check_replicates(got, name: str, rep_first: int, rows=slice(None), columns=slice(None),
                     R: int | None = None):
    """``got = (cal_rep, stats_rep, e_rep)`` against rows ``rows`` and columns ``columns`` of the
    oracle's ``R`` replicates from ``rep_first``."""
    cal, stats, e_rep = got
    R = cal.shape[0] if R is None else R
    ref_e, ref_fits = reference_replicates(name, rep_first, R)
    ref_e, ref_fits = ref_e[rows], ref_fits[rows]
    K = case(name)[3] + 1
    assert cal.shape[0] == len(ref_fits) and cal.shape[2] == K
    for r, row in enumerate(ref_fits):
        row = row[columns]
        assert cal.shape[1] == len(row)
        for t, f in enumerate(row):
            where = f"{name} replicate {rep_first}+{r} column {t}"
            assert same_bits(e_rep[r, t], np.array(ref_e[r][columns][t], dtype=np.int32)), where
            assert same_bits(cal[r, t], f["cal"]), where
            assert same_bits(stats[r, t], [f["S"], f["S_cal"], f["MCB"]]), where


def check_identity(fit, name: str):
    """S against MCB - DSC + UNC and against the exact sum (v - o)^2 / n.

    Bound, 8 * 2^-52 relative to the exact value: S is a sum of at most K non-negative terms,
    each formed with 5 roundings (relative 2.5 * 2^-52 of the term at most) and added
    sequentially, and one division; MCB - DSC + UNC adds four roundings of quantities no larger
    than max(S, 1/4).  The sequential sum's first-order bound is (m - 1) * 2^-53 for m
    non-empty levels; the cases' observed errors are far below it, and 8 * 2^-52 is the figure
    the design sets."""
    p, y, x, q = case(name)
    s = fit.stats.cpu().numpy()
    for t in range(p.shape[1]):
        exact = RO.direct_brier(p, y, x, q, t)
        if exact is None:
            assert np.isnan(s[t, 2])
            continue
        S, UNC, MCB, DSC = s[t, 2], s[t, 4], s[t, 5], s[t, 6]
        bound = 8 * 2.0 ** -52 * float(exact)
        print(f"{name} column {t}: S - exact = {float(S) - float(exact):.3e}, identity - exact = "
              f"{float(MCB - DSC + UNC) - float(exact):.3e}, bound {bound:.3e}")
        assert abs(RO.Fraction(float(S)) - exact) <= RO.Fraction(bound), (name, t)
        assert abs(RO.Fraction(float(MCB - DSC + UNC)) - exact) <= RO.Fraction(bound), (name, t)
