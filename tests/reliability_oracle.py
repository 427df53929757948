"""The contract of DESIGN.md 6k (reliability diagrams) restated on Python integers,
``fractions.Fraction`` and scalar ``numpy.float64`` operations in the stated order.

Nothing here is imported from the package: the generator is copied, the counts are plain loops
and the isotonic fit is the min-max formula ``cal_k = max_{a<=k} min_{b>=k} mean(a..b)`` in exact
fractions, not a stack.  Above 64 non-empty levels a stack version stands in, which
:func:`self_test` holds to the min-max form.
"""
from fractions import Fraction

import numpy as np

F = np.float64
MASK = (1 << 64) - 1
MINMAX_LEVELS = 64
NAN = float("nan")


def mix(seed: int, i: int) -> int:
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix_rows(seed: int, first: int, count: int) -> np.ndarray:
    """``mix(seed, first + j)`` for ``j < count`` as uint64 (the same definition in numpy's
    wrapping arithmetic; :func:`self_test` holds it to :func:`mix`)."""
    with np.errstate(over="ignore"):
        i = np.uint64(first & MASK) + np.arange(count, dtype=np.uint64)
        z = np.uint64(seed & MASK) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def value(k: int, q: int) -> np.float64:
    return F(k) / F(q)


def counts(p, y, x, q: int):
    """p [N, T] float64, y [N] float32, x [T] float64 -> (n_k, e_k) lists [T][K] of ints and
    level [T][N] (-1: invalid)."""
    N, T = p.shape
    K = q + 1
    n_k = [[0] * K for _ in range(T)]
    e_k = [[0] * K for _ in range(T)]
    level = [[-1] * N for _ in range(T)]
    for t in range(T):
        xt = F(x[t])
        for i in range(N):
            yi, pi = F(y[i]), F(p[i, t])
            if yi != yi or xt != xt or not (pi >= 0.0 and pi <= 1.0):
                continue
            k = int(np.rint(pi * F(q)))
            level[t][i] = k
            n_k[t][k] += 1
            if yi > xt:
                e_k[t][k] += 1
    return n_k, e_k, level


def isotonic_minmax(e, n):
    """Means of the isotonic fit of the groups (e_j events of n_j cells, n_j > 0), as exact
    fractions: ``max_{a<=j} min_{b>=j} mean(a..b)``."""
    m = len(e)
    pe, pn = [0], [0]
    for a, b in zip(e, n):
        pe.append(pe[-1] + a)
        pn.append(pn[-1] + b)
    # low[a][j] = min over b >= j of mean(a..b)
    low = [[None] * m for _ in range(m)]
    for a in range(m):
        best = None
        for b in range(m - 1, a - 1, -1):
            mean = Fraction(pe[b + 1] - pe[a], pn[b + 1] - pn[a])
            best = mean if best is None or mean < best else best
            low[a][b] = best
    return [max(low[a][j] for a in range(j + 1)) for j in range(m)]


def blocks_from_means(means, e, n):
    """Consecutive groups of equal fitted mean -> blocks [E_b, N_b, first group]."""
    blocks = []
    for j, mean in enumerate(means):
        if blocks and means[blocks[-1][2]] == mean:
            blocks[-1][0] += e[j]
            blocks[-1][1] += n[j]
        else:
            blocks.append([e[j], n[j], j])
    return blocks


def blocks_stack(e, n):
    """The same blocks by pool-adjacent-violators with exact integer comparisons."""
    blocks = []
    for j, (a, b) in enumerate(zip(e, n)):
        cur = [a, b, j]
        while blocks and blocks[-1][0] * cur[1] >= cur[0] * blocks[-1][1]:
            prev = blocks.pop()
            cur = [cur[0] + prev[0], cur[1] + prev[1], prev[2]]
        blocks.append(cur)
    return blocks


def fit_blocks(e, n):
    if len(e) <= MINMAX_LEVELS:
        return blocks_from_means(isotonic_minmax(e, n), e, n)
    return blocks_stack(e, n)


def fit(n_col, e_col, q: int) -> dict:
    """One column: counts [K] -> cal [K] (NaN at empty levels), block_id [K] (-1 there), blocks
    [(E_b, N_b)], a2 and the statistics as numpy.float64 scalars."""
    K = q + 1
    levels = [k for k in range(K) if n_col[k] > 0]
    e = [e_col[k] for k in levels]
    n = [n_col[k] for k in levels]
    blocks = fit_blocks(e, n)
    cal = [NAN] * K
    block_id = [-1] * K
    for b, (Eb, Nb, first) in enumerate(blocks):
        last = blocks[b + 1][2] if b + 1 < len(blocks) else len(levels)
        for j in range(first, last):
            cal[levels[j]] = F(Eb) / F(Nb)
            block_id[levels[j]] = b
    total = F(0.0)
    a2 = below = 0
    for k, ek, nk in zip(levels, e, n):
        v = value(k, q)
        w = F(1.0) - v
        total = total + (F(nk - ek) * (v * v) + F(ek) * (w * w))
        a2 += ek * (2 * below + (nk - ek))
        below += nk - ek
    nn, EE = sum(n), sum(e)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = total / F(nn)
        cs = F(0.0)
        for Eb, Nb, _ in blocks:
            cs = cs + F(Eb) * (F(Nb - Eb) / F(Nb))
        S_cal = cs / F(nn)
        UNC = F(EE) * (F(nn - EE) / F(nn)) / F(nn)
        AUC = F(a2) / ((F(2.0) * F(EE)) * F(nn - EE))
    return dict(cal=cal, block_id=block_id, blocks=[(b[0], b[1]) for b in blocks], a2=a2,
                n=nn, E=EE, S=S, S_cal=S_cal, UNC=UNC, MCB=S - S_cal, DSC=UNC - S_cal, AUC=AUC,
                stats=[F(nn), F(EE), S, S_cal, UNC, S - S_cal, UNC - S_cal, AUC])


def thresholds53(q: int):
    return [int(np.floor(value(k, q) * F(9007199254740992.0))) for k in range(q + 1)]


def resample_counts(level, q: int, seed: int, rep_first: int, R: int):
    """level [T][N] -> e_rep [R][T][K] ints."""
    T = len(level)
    N = len(level[0]) if T else 0
    K = q + 1
    thr = np.array(thresholds53(q), dtype=np.uint64)
    lv = np.array(level, dtype=np.int64).reshape(T, N)
    out = []
    for j in range(R):
        r = (rep_first + j) & MASK
        U = mix_rows(seed, (r * N) & MASK, N) >> np.uint64(11)
        rows = []
        for t in range(T):
            ok = lv[t] >= 0
            fire = ok & (U < thr[np.where(ok, lv[t], 0)])
            rows.append([int(c) for c in np.bincount(lv[t][fire], minlength=K)])
        out.append(rows)
    return out


def resample(level, n_k, q: int, seed: int, rep_first: int, R: int):
    """-> (e_rep [R][T][K], fits [R][T]: the dicts of :func:`fit` with e* for e)."""
    e_rep = resample_counts(level, q, seed, rep_first, R)
    fits = [[fit(n_k[t], e_rep[j][t], q) for t in range(len(n_k))] for j in range(R)]
    return e_rep, fits


def p_value(mcb, mcb_rep) -> np.float64:
    """``(1 + #{r : MCB*_r >= MCB}) / (R + 1)``; NaN where MCB is."""
    if mcb != mcb:
        return F(NAN)
    count = sum(1 for m in mcb_rep if m >= mcb)
    return F(1 + count) / F(len(mcb_rep) + 1)


def direct_brier(p, y, x, q: int, t: int) -> Fraction:
    """``sum (v - o)^2 / n`` of column ``t`` over its valid cells, exactly (v = k / q)."""
    total, n = Fraction(0), 0
    for i in range(p.shape[0]):
        yi, pi, xt = F(y[i]), F(p[i, t]), F(x[t])
        if yi != yi or xt != xt or not (pi >= 0.0 and pi <= 1.0):
            continue
        k = int(np.rint(pi * F(q)))
        o = 1 if yi > xt else 0
        total += (Fraction(k, q) - o) ** 2
        n += 1
    return total / n if n else None


def self_test(rounds: int = 300, seed: int = 5) -> None:
    """The stack blocks equal the min-max blocks on random and adversarial groups, and the
    numpy generator equals the integer one."""
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        m = int(rng.integers(1, 24))
        n = [int(v) for v in rng.integers(1, 6, m)]
        e = [int(rng.integers(0, b + 1)) for b in n]
        assert blocks_stack(e, n) == blocks_from_means(isotonic_minmax(e, n), e, n), (e, n)
    for m in (1, 2, 17, 64):
        n = [m + 1] * m
        for e in (list(range(m)), list(range(m, 0, -1)), [1] * m, [0] * m):
            assert blocks_stack(e, n) == blocks_from_means(isotonic_minmax(e, n), e, n)
    for s, first in ((0, 0), (12345, 7), (MASK, MASK - 2)):
        got = mix_rows(s, first, 5)
        assert [int(v) for v in got] == [mix(s, (first + j) & MASK) for j in range(5)]
