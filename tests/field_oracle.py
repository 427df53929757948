"""Independent oracle of the per-graph field scores, written from the definitions
with plain loops over graphs, pairs and members; it shares no code with raincast_gnn.fields.
Every sum is accumulated with math.fsum (exactly rounded), so the oracle is the more exact side.

For each score the oracle also returns the sum of the absolute values of the terms it added,
the scale a rounding error is measured against:
  es_abs   = (1/m) sum_i |X_i - y| + (1/(2 m^2)) sum_ij |X_i - X_j|   (both sums positive)
  vs_abs   = sum_{a<b} (|y_a - y_b|^p + mean_i |X_ai - X_bi|^p)^2
  crps_abs = (1/m) sum_i |A_i - obs| + (1/(2 m^2)) sum_ij |A_i - A_j|
(es_fair_abs and crps_fair_abs: the same with 1/(2 m (m - 1))).

x [N, M] float64 member values in model space (NaN = missing), y [N] targets (NaN = missing),
ptr [G + 1].  Results are dicts of [G] float64 arrays ("members" is [G, M]).
"""
import math

import numpy as np

MM_OFFSET = 0.01
NAN = float("nan")


def values(members, scale=1.0, shift=0.0):
    """shift + scale * members in float64 (one product, one sum: two roundings)."""
    return np.float64(shift) + np.float64(scale) * np.asarray(members, dtype=np.float64)


def valid_sets(x, y):
    """-> (rows of S, members of V) of one graph's x [n, M], y [n]."""
    n, M = x.shape
    rows = [r for r in range(n) if not math.isnan(y[r])
            and any(not math.isnan(x[r, i]) for i in range(M))]
    mem = [i for i in range(M) if all(not math.isnan(x[r, i]) for r in rows)]
    return rows, mem


def power(d, p):
    if p == 0.5:
        return math.sqrt(d)
    if p == 1.0:
        return d
    if p == 2.0:
        return d * d
    return d ** p


def to_mm(v):
    return max(math.exp(v) - MM_OFFSET, 0.0)


def norm(u):
    return math.sqrt(math.fsum((u * u).tolist()))  # the squares one rounding each, as in a loop


def energy(X, y):
    """X [n, m] (S x V), y [n] -> es, es_fair, es_abs, es_fair_abs."""
    m = X.shape[1]
    to_obs = math.fsum(norm(X[:, i] - y) for i in range(m))
    # sum over all (i, j): the diagonal is 0 and (i, j), (j, i) are equal, so twice j < i, exactly
    between = 2.0 * math.fsum(norm(X[:, i] - X[:, j]) for i in range(m) for j in range(i))
    es = to_obs / m - between / (2.0 * m * m)
    fair = to_obs / m - between / (2.0 * m * (m - 1)) if m > 1 else NAN
    fair_abs = to_obs / m + between / (2.0 * m * (m - 1)) if m > 1 else NAN
    return es, fair, to_obs / m + between / (2.0 * m * m), fair_abs


def variogram(X, y, p):
    """Plain loops over the pairs a < b and the members -> vs, vs_abs."""
    n, m = X.shape
    terms, mags = [], []
    rows = [[float(v) for v in X[a]] for a in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            ra, rb = rows[a], rows[b]
            mean = math.fsum(power(abs(ra[i] - rb[i]), p) for i in range(m)) / m
            w = power(abs(float(y[a]) - float(y[b])), p)
            terms.append((w - mean) ** 2)
            mags.append((w + mean) ** 2)
    return math.fsum(terms), math.fsum(mags)


def variogram_by_rows(X, y, p):
    """The same sum with the members and b-rows of one a-row vectorised (large graphs): the
    member mean is numpy's pairwise sum, the sum over pairs still math.fsum."""
    n, m = X.shape
    pw = {0.5: np.sqrt, 1.0: lambda d: d, 2.0: np.square}.get(p, lambda d: d ** p)
    terms, mags = [], []
    for a in range(n - 1):
        mean = pw(np.abs(X[a + 1:] - X[a])).sum(1) / m
        w = pw(np.abs(y[a + 1:] - y[a]))
        terms.extend(((w - mean) ** 2).tolist())
        mags.extend(((w + mean) ** 2).tolist())
    return math.fsum(terms), math.fsum(mags)


def area(X, y, stat):
    """-> A [m], obs, crps, crps_fair, rank_lo, rank_hi, crps_abs, crps_fair_abs."""
    n, m = X.shape
    if stat == "max":
        A = [max(to_mm(X[r, i]) for r in range(n)) for i in range(m)]
        obs = max(to_mm(v) for v in y)
    else:
        A = [math.fsum(to_mm(X[r, i]) for r in range(n)) / n for i in range(m)]
        obs = math.fsum(to_mm(v) for v in y) / n
    to_obs = math.fsum(abs(a - obs) for a in A)
    between = math.fsum(abs(a - b) for a in A for b in A)
    crps = to_obs / m - between / (2.0 * m * m)
    fair = to_obs / m - between / (2.0 * m * (m - 1)) if m > 1 else NAN
    lo = float(sum(a < obs for a in A))
    hi = float(sum(a <= obs for a in A))
    fair_abs = to_obs / m + between / (2.0 * m * (m - 1)) if m > 1 else NAN
    return A, obs, crps, fair, lo, hi, to_obs / m + between / (2.0 * m * m), fair_abs


FIELDS = ("es", "es_fair", "es_abs", "es_fair_abs", "vs", "vs_abs", "pairs", "obs", "crps",
          "crps_fair", "crps_abs", "crps_fair_abs", "rank_lo", "rank_hi", "members_valid",
          "rows_valid")
PARTS = ("energy", "variogram", "area")


def score(x, y, ptr, p=0.5, stat="max", by_rows=False, parts=PARTS):
    """Every score of every graph; `parts` leaves the others at NaN (the counts always come)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    G, M = len(ptr) - 1, x.shape[1]
    out = {k: np.full(G, NAN) for k in FIELDS}
    out["members"] = np.full((G, M), NAN)
    for g in range(G):
        xg, yg = x[ptr[g]:ptr[g + 1]], y[ptr[g]:ptr[g + 1]]
        rows, mem = valid_sets(xg, yg)
        n, m = len(rows), len(mem)
        out["rows_valid"][g], out["members_valid"][g] = n, m
        out["pairs"][g] = n * (n - 1) // 2
        if n == 0 or m == 0:
            continue
        X, ys = xg[np.ix_(rows, mem)], yg[rows]
        if "energy" in parts:
            (out["es"][g], out["es_fair"][g], out["es_abs"][g],
             out["es_fair_abs"][g]) = energy(X, ys)
        if "variogram" in parts:
            vario = variogram_by_rows if by_rows else variogram
            out["vs"][g], out["vs_abs"][g] = vario(X, ys, p)
        if "area" not in parts:
            continue
        A, obs, crps, fair, lo, hi, mag, fair_mag = area(X, ys, stat)
        out["members"][g, mem] = A
        for k, v in (("obs", obs), ("crps", crps), ("crps_fair", fair), ("rank_lo", lo),
                     ("rank_hi", hi), ("crps_abs", mag), ("crps_fair_abs", fair_mag)):
            out[k][g] = v
    return out
