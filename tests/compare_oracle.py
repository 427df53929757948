"""Independent restatement of the paired-comparison definitions (include/gine_hip.h, DESIGN.md
6j): the generator on Python integers masked to 64 bits, every sum an explicit sequential loop
of fp64 scalars (numpy float64, or Python floats in the replicate loop, which is the long one),
Diebold-Mariano with math.sqrt and math.erfc.  Imports nothing from the package."""
import math

import numpy as np

M64 = (1 << 64) - 1
F = np.float64


def mix(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def num_blocks(T, L):
    return -(-T // L)


def start(seed, r, j, T, L):
    return ((mix(seed, (r * num_blocks(T, L) + j) & M64) >> 32) * T) >> 32


def draws(seed, r, T, L):
    """The T days of global replicate r, in order."""
    out = []
    for j in range(num_blocks(T, L)):
        s = start(seed, r, j, T, L)
        for i in range(L):
            if len(out) < T:
                out.append((s + i) % T)
    return out


def valid(a, b):
    return ~np.isnan(a) & ~np.isnan(b)


def bootstrap(a, b, w, L, seed, rep_first, R):
    """-> dict of sum_a, sum_b, sum_w, diff, skill, each [R, S]."""
    T, S = a.shape
    ok = valid(a, b)
    A = np.zeros((R, S))
    B = np.zeros((R, S))
    W = np.zeros((R, S))
    # per station, the valid days' (a, b, w) as Python floats (IEEE fp64; one add per step)
    cols = []
    for s in range(S):
        ws = [1.0] * T if w is None else w[:, s].tolist()
        cols.append([(x, y, v) if good else None
                     for x, y, v, good in zip(a[:, s].tolist(), b[:, s].tolist(), ws,
                                              ok[:, s].tolist())])
    for i in range(R):
        days = draws(seed, rep_first + i, T, L)
        for s in range(S):
            col = cols[s]
            xa, xb, xw = 0.0, 0.0, 0.0
            for t in days:
                e = col[t]
                if e is not None:
                    xa = xa + e[0]
                    xb = xb + e[1]
                    xw = xw + e[2]
            A[i, s], B[i, s], W[i, s] = xa, xb, xw
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"sum_a": A, "sum_b": B, "sum_w": W, "diff": (A - B) / W, "skill": 1.0 - A / B}


def station_sums(a, b):
    T, S = a.shape
    ok = valid(a, b)
    out = np.zeros((3, S))
    for s in range(S):
        xa, xb, n = F(0.0), F(0.0), F(0.0)
        for t in range(T):
            if ok[t, s]:
                xa, xb, n = xa + F(a[t, s]), xb + F(b[t, s]), n + F(1.0)
        out[:, s] = xa, xb, n
    return out


def day_sums_exact(a, b):
    """-> (day_a, day_b, day_n, abs_a, abs_b): math.fsum over a day's valid stations, and the
    sums of absolute values the error bound is stated in."""
    T, S = a.shape
    ok = valid(a, b)
    out = np.zeros((5, T))
    for t in range(T):
        xs = [float(a[t, s]) for s in range(S) if ok[t, s]]
        ys = [float(b[t, s]) for s in range(S) if ok[t, s]]
        out[:, t] = (math.fsum(xs), math.fsum(ys), len(xs), math.fsum(map(abs, xs)),
                     math.fsum(map(abs, ys)))
    return out


def dm_column(a, b, h):
    """One column -> (n, dbar, var, stat, p)."""
    T = len(a)
    ok = [not math.isnan(a[t]) and not math.isnan(b[t]) for t in range(T)]
    total, n = F(0.0), 0
    for t in range(T):
        if ok[t]:
            total = total + (F(a[t]) - F(b[t]))
            n += 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = F(n)
        dbar = total / nf
        v = F(0.0)
        for k in range(h + 1):
            g = F(0.0)
            for t in range(T - k):
                if ok[t] and ok[t + k]:
                    x = (F(a[t]) - F(b[t])) - dbar
                    y = (F(a[t + k]) - F(b[t + k])) - dbar
                    g = g + x * y
            g = g / nf
            v = g if k == 0 else v + F(2.0 * (1.0 - k / (h + 1.0))) * g
        var = v / nf
    if n < 2 or not (var > 0.0) or math.isinf(var):
        return float(n), float(dbar), float(var), math.nan, math.nan
    stat = float(dbar) / math.sqrt(float(var))
    return float(n), float(dbar), float(var), stat, math.erfc(abs(stat) * 0.70710678118654752440)


def dm(a, b, h):
    """-> [5, S]: n, dbar, var, stat, p per station."""
    return np.array([dm_column(a[:, s], b[:, s], h) for s in range(a.shape[1])]).T


def benjamini_hochberg(p, fdr):
    p = np.asarray(p, dtype=np.float64)
    finite = [i for i in range(len(p)) if math.isfinite(p[i])]
    finite.sort(key=lambda i: p[i])
    m = len(finite)
    last = 0
    for rank, i in enumerate(finite, 1):
        if p[i] <= rank * fdr / m:
            last = rank
    out = np.zeros(len(p), dtype=bool)
    for rank, i in enumerate(finite, 1):
        out[i] = rank <= last
    return out
