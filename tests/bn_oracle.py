"""Exact oracle of train-mode BatchNorm1d statistics and of the BatchNorm-backward coefficients,
independent of raincast_gnn (numpy, fractions, mpmath only).

Its inputs are the arrays a kernel itself read or wrote -- the fp32 a1 the producer launch
stored, and for the backward the fp32 dbn it stored and the fp32 bn_save it was given -- never
the values a test intended, so nothing here depends on a matrix product being exact.

Arithmetic: an fp32 number is m * 2^e with an integer |m| <= 2^24, so column sums of fp32
values and of products of two fp32 values are sums of integers per exponent (column_dots:
numpy adds the integers of one exponent, each total far below 2^53 and therefore exact, and
Python integers combine the exponents).  Every sum is exact, returned as fractions.Fraction;
mean, var and the coefficients follow in exact rational arithmetic; sqrt goes through mpmath
at 50 digits (MP), the only rounding of the oracle (1e-50 relative).

Forward, per channel (a1 [N, D]):
  mean = sum a / N, var = sum a^2 / N - mean^2 (biased), invstd = 1 / sqrt(var + eps32),
  alpha = gamma * invstd, shift = beta - mean * alpha, A = sum |a|, Q = sum a^2;
  running(): f * mean + (1 - f) * running_mean and f * unbiased + (1 - f) * running_var with
  unbiased = var * N / (N - 1), and var itself at N = 1.
N = 1: torch.nn.functional.batch_norm refuses a single row in training mode; the project's
rule (csrc/gine_bnacc.hpp bn_finish_channel, gine_mlp.hip k_bn_fwd_finalize / BnFwdFin) is
var = 0 for the batch and the biased var, 0, into the running variance.  That deviation from
torch is the project's documented behaviour and what running() returns.

Backward, per channel (dbn, a1 [N, D]; mean32, invstd32 the saved fp32 statistics, exact):
  xhat = (a1 - mean32) * invstd32, sd = sum dbn, sx = sum dbn * xhat,
  c1 = gamma * invstd32, c2 = -c1 * sx / N, c3 = -c1 * sd / N,
  SD = sum |dbn|, SX = sum |dbn * xhat|.
"""
from fractions import Fraction

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50

_MASK24 = (1 << 24) - 1


def _decompose(x):
    """fp32 array -> (m, e) int64 arrays with x = m * 2^e exactly, |m| <= 2^24."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and np.isfinite(x).all()
    f, e = np.frexp(x.astype(np.float64))
    m = np.ldexp(f, 24)
    assert (m == np.rint(m)).all()
    return m.astype(np.int64), e.astype(np.int64) - 24


def column_dots(x, y=None):
    """Exact column sums of x (y None) or of x * y; x, y fp32 [N, D].  List of D Fractions."""
    mx, ex = _decompose(x)
    if y is None:
        p, e = mx, ex
    else:
        my, ey = _decompose(y)
        assert my.shape == mx.shape
        p, e = mx * my, ex + ey          # |p| <= 2^48
    N, D = p.shape
    assert N < (1 << 28)                  # per-exponent totals stay below 2^53
    hi, lo = p >> 24, p & _MASK24         # p = hi * 2^24 + lo (floor), |hi| <= 2^24, 0 <= lo < 2^24
    emin = int(e.min())
    span = int(e.max()) - emin + 1
    idx = ((e - emin) * D + np.arange(D, dtype=np.int64)).ravel()
    H = np.bincount(idx, weights=hi.ravel().astype(np.float64), minlength=span * D)
    L = np.bincount(idx, weights=lo.ravel().astype(np.float64), minlength=span * D)
    H, L = H.reshape(span, D), L.reshape(span, D)
    scale = Fraction(2) ** emin
    out = []
    for c in range(D):
        tot = 0
        for k in np.nonzero((H[:, c] != 0) | (L[:, c] != 0))[0]:
            tot += ((int(H[k, c]) << 24) + int(L[k, c])) << int(k)
        out.append(Fraction(tot) * scale)
    return out


def frac(x):
    """Exact Fraction of a binary floating-point scalar."""
    return Fraction(float(x))


def mpf(q):
    """Fraction (or number) -> MP.mpf, rounded once at 50 digits."""
    if isinstance(q, Fraction):
        return MP.mpf(q.numerator) / MP.mpf(q.denominator)
    return MP.mpf(q)


def invstd(var, eps32):
    """1 / sqrt(var + eps32) at 50 digits (var, eps32 exact rationals or mpf)."""
    return 1 / MP.sqrt(mpf(var) + mpf(eps32))


def forward_sums(a1):
    """The exact sums of one a1: {N, s1, q, a} with per-channel lists of Fractions."""
    a1 = np.asarray(a1)
    return {"N": a1.shape[0], "s1": column_dots(a1), "q": column_dots(a1, a1),
            "a": column_dots(np.abs(a1))}


def forward_channel(sums, c, gamma, beta, eps32):
    """Channel c: exact mean, var, A, Q (Fractions) and invstd, alpha, shift (mpf).  gamma,
    beta: the fp32 values the kernel read (1 and 0 for a BatchNorm without affine)."""
    N = sums["N"]
    mean = sums["s1"][c] / N
    var = sums["q"][c] / N - mean * mean
    assert var >= 0
    inv = invstd(var, frac(eps32))
    alpha = mpf(frac(gamma)) * inv
    return {"mean": mean, "var": var, "A": sums["a"][c], "Q": sums["q"][c], "invstd": inv,
            "alpha": alpha, "shift": mpf(frac(beta)) - mpf(mean) * alpha}


def running(mean, var, N, f, rm_old, rv_old):
    """New running mean and var (Fractions) for the factor f (a double: the momentum as the
    kernel widens it, or 1 / num_batches_tracked) from the fp32 buffers the kernel read."""
    f = frac(f)
    unbiased = var * N / (N - 1) if N > 1 else var
    return (f * mean + (1 - f) * frac(rm_old), f * unbiased + (1 - f) * frac(rv_old), unbiased)


def backward_sums(dbn, a1, mean, inv):
    """Exact per-channel sd, sx, SD, SX (lists of Fractions).  mean, inv: per-channel binary
    floating-point statistics, taken exactly (the saved fp32 mean32 / invstd32)."""
    dbn, a1 = np.asarray(dbn), np.asarray(a1)
    D = dbn.shape[1]
    mean64 = np.asarray(mean, dtype=np.float64)
    # sum dbn * xhat = inv * (sum dbn * a1 - mean * sum dbn); the magnitudes the same way with
    # w = |dbn| * sign(a1 - mean), an fp32 array (the sign of a rounded difference is exact)
    w = (np.abs(dbn) * np.sign(a1.astype(np.float64) - mean64)).astype(np.float32)
    sd, da = column_dots(dbn), column_dots(dbn, a1)
    sw, wa = column_dots(w), column_dots(w, a1)
    out = {"sd": sd, "SD": column_dots(np.abs(dbn)), "sx": [], "SX": []}
    for c in range(D):
        m, i = frac(mean[c]), frac(inv[c])
        out["sx"].append(i * (da[c] - m * sd[c]))
        out["SX"].append(i * (wa[c] - m * sw[c]))
        assert out["SX"][c] >= 0
    return out


def coef(sums, c, gamma, inv, N, training=True):
    """Channel c: exact c1, c2, c3 (Fractions); c2 = c3 = 0 without batch statistics."""
    c1 = frac(gamma) * frac(inv)
    if not training:
        return c1, Fraction(0), Fraction(0)
    return c1, -c1 * sums["sx"][c] / N, -c1 * sums["sd"][c] / N


def fl32(q):
    """The correctly rounded fp32 of a Fraction that is exact in fp64 (a 24 x 24 bit product)."""
    d = float(q)
    assert Fraction(d) == q
    return np.float32(d)
