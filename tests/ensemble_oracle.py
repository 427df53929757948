"""Independent fp64 numpy oracle of the raw-ensemble scores and the ECC levels, written from
the definitions and sharing no code with the package: ranks by explicit
counting, the CRPS pair term as the O(M^2) double sum.

A member is ``x = shift + scale * raw`` (fp64; one product, one sum); NaN = missing; ``m`` = the
row's valid count.
  r_i       = 1 + #{j valid : x_j < x_i or (x_j == x_i and j < i)}
  crps      = (1/m) sum |x_i - y| - (1/(2 m^2)) sum_i sum_j |x_i - x_j|
  crps_fair = the same with 1/(2 m (m - 1)); NaN for m < 2
  rank_lo   = #{x_i < y},  rank_hi = #{x_i <= y}
  prob[t]   = #{x_i > x_t} / m
Row scores NaN for a NaN target or m = 0; prob NaN for m = 0.
"""
import numpy as np


def values(raw, scale=1.0, shift=0.0):
    return np.float64(shift) + np.float64(scale) * np.asarray(raw, dtype=np.float64)


def ranks(x):
    """x [N, M] -> (r [N, M] int64, 0 where the member is missing; m [N] int64)."""
    N, M = x.shape
    r = np.zeros((N, M), dtype=np.int64)
    m = np.zeros(N, dtype=np.int64)
    for n in range(N):
        row = x[n].tolist()  # Python floats: the counting loops stay plain and quick
        for i in range(M):
            if row[i] != row[i]:
                continue
            m[n] += 1
            count = 0
            for j in range(M):
                if row[j] < row[i] or (row[j] == row[i] and j < i):  # NaN: neither
                    count += 1
            r[n, i] = 1 + count
    return r, m


def score_rows(x, y):
    """-> dict of crps, crps_fair, rank_lo, rank_hi, m, each [N] fp64."""
    N = x.shape[0]
    out = {k: np.full(N, np.nan) for k in ("crps", "crps_fair", "rank_lo", "rank_hi")}
    out["m"] = np.zeros(N)
    for n in range(N):
        v = x[n][~np.isnan(x[n])]
        m = len(v)
        out["m"][n] = m
        if m == 0 or np.isnan(y[n]):
            continue
        yy = np.float64(y[n])
        first = np.abs(v - yy).sum() / m
        pairs = 0.0
        vl = v.tolist()
        for i in range(m):
            for j in range(m):
                pairs += abs(vl[i] - vl[j])
        out["crps"][n] = first - pairs / (2.0 * m * m)
        if m > 1:
            out["crps_fair"][n] = first - pairs / (2.0 * m * (m - 1))
        out["rank_lo"][n] = np.sum(v < yy)
        out["rank_hi"][n] = np.sum(v <= yy)
    return out


def prob(x, thresholds):
    """-> [N, T] exceedance probabilities (NaN for a row without members)."""
    N, T = x.shape[0], len(thresholds)
    out = np.full((N, T), np.nan)
    for n in range(N):
        v = x[n][~np.isnan(x[n])]
        if len(v) == 0:
            continue
        for t in range(T):
            out[n, t] = np.float64(np.sum(v > thresholds[t])) / np.float64(len(v))
    return out


def brier(p, y, thresholds, crps):
    """-> (brier [T], valid): over rows with a score (target and members present)."""
    ok = ~np.isnan(crps)
    valid = int(ok.sum())
    out = np.full(len(thresholds), np.nan)
    if valid:
        for t in range(len(thresholds)):
            d = p[ok, t] - (y[ok].astype(np.float64) > thresholds[t])
            out[t] = np.sum(d * d) / valid
    return out, valid


def ecc_levels(x, rule):
    """-> [N, M] fp64: r / (m + 1) ("uniform") or (r - 0.5) / m ("midpoint"), NaN where the
    member is missing; each one IEEE division of exact operands."""
    r, m = ranks(x)
    lv = np.full(x.shape, np.nan)
    for n in range(x.shape[0]):
        for i in range(x.shape[1]):
            if r[n, i] == 0:
                continue
            if rule == "uniform":
                lv[n, i] = np.float64(r[n, i]) / np.float64(m[n] + 1)
            else:
                lv[n, i] = (np.float64(r[n, i]) - 0.5) / np.float64(m[n])
    return lv
