"""Independent fp64 oracle of the threshold-weighted CRPS, weight 1{x >= t} (numpy + scipy +
math only; shares no code with the package):

    twCRPS_t(F, y) = int_{t'}^inf (F(x) - 1{x >= y'})^2 dx,   t' = max(t, c) (t for "normal"),
                                                             y' = max(y, t')

(a) ``quad_rows``: that integral by scipy.integrate.quad, split at u and y' (and into windows of the row's scales above
    the last of them), with quad's own error estimate.  Its scalar F is written here from the definition in forecast_oracle's
    docstring (math.erfc; quad evaluates it point by point) and agrees with ``Dist.cdf``.
(b) ``closed_rows``: the closed forms, a second route: CRPS of F censored at t' below u; above
    u what is left of the Pareto tail.
The raw ensemble: ``ensemble_rows``, the double-sum definition on clamped values.
A threshold of -inf: the CRPS at max(y, c) (at y for "normal"); NaN: NaN.
"""
import math

import numpy as np
from scipy.integrate import quad
from scipy.special import erfcx, ndtr

SQRT2 = math.sqrt(2.0)


def _t_eff(dist, t):
    return max(t, dist.c) if dist.atom else t


# ------------------------------------------------------------------------------- (a) quadrature
def _row_cdf(dist, i):
    """Scalar F and 1 - F of row i, from the definition."""
    mu, sigma, p = float(dist.mu[i, 0]), float(dist.sigma[i, 0]), float(dist.p[i, 0])
    c, atom, tail = dist.c, dist.atom, dist.tail
    if tail:
        u, su, xi = float(dist.u[i, 0]), float(dist.su[i, 0]), float(dist.xi)
        zu = (u - mu) / sigma
        m_u = p + (1 - p) * 0.5 * math.erfc(-zu / SQRT2)
        om_u = (1 - p) * 0.5 * math.erfc(zu / SQRT2)

    def F(x):
        if atom and x < c:
            return 0.0
        if tail and x >= u:
            return m_u + om_u * (1.0 - (1.0 + xi * (x - u) / su) ** (-1.0 / xi))
        return p + (1 - p) * 0.5 * math.erfc(-(x - mu) / sigma / SQRT2)

    def S(x):  # 1 - F without the subtraction (1 - F is 0 in fp64 from 1e-16 down)
        if atom and x < c:
            return 1.0
        if tail and x >= u:
            return om_u * (1.0 + xi * (x - u) / su) ** (-1.0 / xi)
        return (1 - p) * 0.5 * math.erfc((x - mu) / sigma / SQRT2)

    return F, S


def quad_rows(dist, y, t):
    """-> (values [N], quad's error estimates [N]) at one threshold t; NaN rows for NaN y or t."""
    y = np.asarray(y, dtype=np.float64)
    val, est = np.full(len(y), np.nan), np.full(len(y), np.nan)
    if math.isnan(t):
        return val, est
    tp = _t_eff(dist, t)
    for i, yi in enumerate(y):
        if math.isnan(yi):
            continue
        F, S = _row_cdf(dist, i)
        yp = max(float(yi), tp)
        cuts = {tp, yp, math.inf}
        if dist.tail and float(dist.u[i, 0]) > tp:
            cuts.add(float(dist.u[i, 0]))
        # the infinite last piece in windows of the row's own scales: far up the tail the
        # integrand is a spike next to its lower limit that quad's first panel can miss whole
        last = max(v for v in cuts if v != math.inf)
        for scale in (float(dist.sigma[i, 0]),) + ((float(dist.su[i, 0]),) if dist.tail else ()):
            cuts.update(last + k * scale for k in (0.05, 1.0, 10.0))
        cuts = sorted(cuts)
        v = e = 0.0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            f = S if lo >= yp else F  # the indicator is constant on the piece: (F - 1)^2 = S^2
            r = quad(lambda x: f(x) ** 2, lo, hi, epsabs=1e-14, epsrel=1e-13, limit=200)
            v, e = v + r[0], e + r[1]
        val[i], est[i] = v, e
    return val, est


# ----------------------------------------------------------------------------- (b) closed forms
def _pdf(v):
    return np.exp(-v * v / 2) / np.sqrt(2 * np.pi)


def _censored(mu, s, p, y, c):
    """CRPS at y >= c of p + (1 - p) N(mu, s^2) censored at c, in upper probabilities
    S(x) = (1 - p) Phi(-z):  (y - c) - 2 int_c^y S + int_c^inf S^2, with
    int Phi(-z) dz = z Phi(-z) - pdf(z) and
    int_a^inf Phi(-z)^2 dz = -a Phi(-a)^2 + 2 pdf(a) Phi(-a) - Phi(-sqrt2 a) / sqrt(pi)."""
    yt, ct = (y - mu) / s, (c - mu) / s
    q = 1 - p
    up = lambda z: ndtr(-z)  # noqa: E731
    one = (yt * up(yt) - _pdf(yt)) - (ct * up(ct) - _pdf(ct))
    two = -ct * up(ct) ** 2 + 2 * _pdf(ct) * up(ct) - up(np.sqrt(2) * ct) / np.sqrt(np.pi)
    # far up (a >= 3) the same integral with the Mills ratio R(z) = Phi(-z) / pdf(z) factored
    # out, pdf(a)^2 (2 R(a) - a R(a)^2 - sqrt2 R(sqrt2 a)): the three terms above are products of
    # exp() whose argument rounding (a^2 eps / 2) their difference magnifies 2 a^2 times
    a = np.maximum(ct, 3.0)
    R = lambda z: np.sqrt(np.pi / 2) * erfcx(z / np.sqrt(2))  # noqa: E731
    far = _pdf(a) ** 2 * (2 * R(a) - a * R(a) ** 2 - np.sqrt(2) * R(np.sqrt(2) * a))
    two = np.where(ct >= 3.0, far, two)
    return (y - c) - 2 * s * q * one + s * q * q * two


def closed_rows(dist, y, t):
    """-> values [N] at one threshold t."""
    y = np.asarray(y, dtype=np.float64)[:, None]
    if math.isnan(t):
        return np.full(len(y), np.nan)
    tp = _t_eff(dist, t)
    mu, s, p = dist.mu, dist.sigma, dist.p
    with np.errstate(all="ignore"):
        if tp == -math.inf:  # "normal" only: the plain CRPS
            z = (y - mu) / s
            return (s * (z * (2 * ndtr(z) - 1) + 2 * _pdf(z) - 1 / np.sqrt(np.pi)))[:, 0]
        yp = np.maximum(y, tp)
        if not dist.tail:
            return _censored(mu, s, p, yp, tp)[:, 0]
        u, su, xi, a = dist.u, dist.su, dist.xi, dist.om_u
        w = lambda x: 1 + xi * np.maximum(x - u, 0.0) / su  # noqa: E731
        e1, e2 = -(1 - xi) / xi, -(2 - xi) / xi
        # t' >= u: the tail above t'
        tl = (yp - tp) + 2 * a * su / (1 - xi) * (w(yp) ** e1 - w(tp) ** e1) \
            + a * a * su / (2 - xi) * w(tp) ** e2
        # t' < u: the body censored at t' up to u, then the whole tail
        ct, ut, yt = (tp - mu) / s, (u - mu) / s, (np.minimum(yp, u) - mu) / s
        q = 1 - p
        P_c = p + q * ndtr(ct)
        t2 = -ct * P_c ** 2 + ut * a ** 2
        t3 = -2 * q * _pdf(ct) * P_c - 2 * q * _pdf(ut) * a
        t5 = -q ** 2 / np.sqrt(np.pi) * (ndtr(np.sqrt(2) * ut) - ndtr(np.sqrt(2) * ct))
        below = s * (yt * (2 * (p + q * ndtr(yt)) - 1) + t2 + t3 + 2 * q * _pdf(yt) + t5) \
            + a * a * su / (2 - xi)
        above = s * (ut + t2 + t3 - 2 * (-q * _pdf(ut) + ut * a) + t5) \
            + (yp - u) + 2 * a * su / (1 - xi) * (w(yp) ** e1 - 1) + a * a * su / (2 - xi)
        body = np.where(yp < u, below, above)
        return np.where(tp >= u, tl, body)[:, 0]


# --------------------------------------------------------------------------------- the ensemble
def ensemble_rows(x, y, t):
    """x [N, M] fp64 members (NaN missing), y [N], one threshold -> (crps [N], fair [N])."""
    n = x.shape[0]
    crps, fair = np.full(n, np.nan), np.full(n, np.nan)
    if math.isnan(t):
        return crps, fair
    for i in range(n):
        v = x[i][~np.isnan(x[i])]
        m = len(v)
        if m == 0 or np.isnan(y[i]):
            continue
        v = np.maximum(v, t)
        yc = max(float(y[i]), t)
        a = np.abs(v - yc).sum() / m
        pair = np.abs(v[:, None] - v[None, :]).sum()
        crps[i] = a - pair / (2.0 * m * m)
        if m > 1:
            fair[i] = a - pair / (2.0 * m * (m - 1))
    return crps, fair
