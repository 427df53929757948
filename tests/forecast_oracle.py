"""Independent fp64 oracle of the predictive distribution (numpy + scipy only).

Written from the definition, sharing no code with the package:
  c = censoring point, z(x) = (x - mu) / sigma, Phi = scipy.special.ndtr
  normal        F(x) = Phi(z)
  mixed_normal  F(x) = 0 (x < c), p + (1 - p) Phi(z) (x >= c); atom P_c = F(c)
  mixed(_u)     as mixed_normal below u; x >= u: m_u + (1 - m_u) G((x - u) / sigma_u),
                m_u = p + (1 - p) Phi(z(u)), G(t) = 1 - (1 + xi t)^(-1/xi)
``params``: [N, K] float64 rows (K = 2, 3, 4, 5); ``u``: the fixed threshold of "mixed".
Targets at or below c are the atom for ``pit`` and ``brier`` (a censored variable has no value
below c); ``crps_rows`` takes y as it is, as the losses do.
"""
import numpy as np
from scipy.special import erfc, ndtr, ndtri

C = float(np.log(0.01))


class Dist:
    def __init__(self, kind, params, u=None, xi=None, c=C):
        P = np.asarray(params, dtype=np.float64)
        self.kind, self.c, self.xi = kind, float(c), xi
        self.mu, self.sigma = P[:, 0:1], P[:, 1:2]
        self.atom = kind != "normal"
        self.tail = kind in ("mixed", "mixed_u")
        self.p = P[:, 2:3] if self.atom else np.zeros_like(self.mu)
        if self.tail:
            self.su = P[:, 3:4]
            self.u = P[:, 4:5] if kind == "mixed_u" else np.full_like(self.mu, float(u))
            zu = (self.u - self.mu) / self.sigma
            self.m_u = self.p + (1 - self.p) * ndtr(zu)
            self.om_u = (1 - self.p) * ndtr(-zu)          # 1 - m_u without cancellation
        if self.atom:
            zc = (self.c - self.mu) / self.sigma
            self.P_c = self.p + (1 - self.p) * ndtr(zc)
            self.S_c = (1 - self.p) * ndtr(-zc)

    def _z(self, x):
        return (x - self.mu) / self.sigma

    def _gpd_sf(self, x):
        t = np.maximum((x - self.u) / self.su, 0.0)
        return (1 + self.xi * t) ** (-1 / self.xi)

    def cdf(self, x):
        """F at x [T] (or [N, T]) -> [N, T]."""
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        x = x[None, :] if x.ndim == 1 else x
        with np.errstate(all="ignore"):
            F = self.p + (1 - self.p) * ndtr(self._z(x))
            if self.tail:
                F = np.where(x >= self.u, self.m_u + self.om_u * (1 - self._gpd_sf(x)), F)
            if self.atom:
                F = np.where(x < self.c, 0.0, F)
        return F

    def sf(self, x):
        """P(Y > x), from the upper normal tail and the tail power."""
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        x = x[None, :] if x.ndim == 1 else x
        with np.errstate(all="ignore"):
            S = (1 - self.p) * 0.5 * erfc(self._z(x) / np.sqrt(2.0))
            if self.tail:
                S = np.where(x >= self.u, self.om_u * self._gpd_sf(x), S)
            if self.atom:
                S = np.where(x < self.c, 1.0, S)
        return S

    def quantile(self, level, upper=False):
        """inf{x : F(x) >= q} for q = level (upper: level = 1 - q) -> [N, T]."""
        lv = np.asarray(level, dtype=np.float64)[None, :] + np.zeros_like(self.mu)
        q1 = 1 - self.p
        with np.errstate(all="ignore"):
            s = lv if upper else 1 - lv
            below = (1 - s / q1) if upper else (lv - self.p) / q1
            x_lo = self.mu + self.sigma * ndtri(below)
            x_hi = self.mu - self.sigma * ndtri(s / q1)
            x = np.where(below > 0.5, x_hi, x_lo)
            if self.tail:
                in_tail = (lv < self.om_u) if upper else (lv > self.m_u)
                xt = self.u + self.su / self.xi * ((s / self.om_u) ** (-self.xi) - 1)
                x = np.where(in_tail, xt, x)
            if self.atom:
                x = np.where((lv >= self.S_c) if upper else (lv <= self.P_c), self.c, x)
            else:
                x = np.where(s == 1, -np.inf, x)
            x = np.where(s == 0, np.inf, x)
            x = np.where((lv >= 0) & (lv <= 1), x, np.nan)
        return x

    # closed-form CRPS of the reference's losses, in float64 throughout
    def crps_rows(self, y):
        y = np.asarray(y, dtype=np.float64)[:, None]
        mu, s, p = self.mu, self.sigma, self.p
        pdf = lambda v: np.exp(-v * v / 2) / np.sqrt(2 * np.pi)  # noqa: E731
        yt = (y - mu) / s
        with np.errstate(all="ignore"):
            if not self.atom:
                out = s * (yt * (2 * ndtr(yt) - 1) + 2 * pdf(yt) - 1 / np.sqrt(np.pi))
                return out[:, 0]
            ct = (self.c - mu) / s
            P_c = p + (1 - p) * ndtr(ct)
            t1 = yt * (2 * (p + (1 - p) * ndtr(yt)) - 1)
            t4 = 2 * (1 - p) * pdf(yt)
            if not self.tail:
                t2 = -ct * P_c ** 2
                t3 = -2 * (1 - p) * pdf(ct) * P_c
                t5 = -(1 - p) ** 2 / np.sqrt(np.pi) * (1 - ndtr(np.sqrt(2) * ct))
                return (s * (t1 + t2 + t3 + t4 + t5))[:, 0]
            u, su, xi = self.u, self.su, self.xi
            ut = (u - mu) / s
            P_u = (1 - p) * (1 - ndtr(ut))
            t2 = -ct * P_c ** 2 + ut * P_u ** 2
            t3 = -2 * (1 - p) * pdf(ct) * P_c - 2 * (1 - p) * pdf(ut) * P_u
            t5 = -(1 - p) ** 2 / np.sqrt(np.pi) * (ndtr(np.sqrt(2) * ut) - ndtr(np.sqrt(2) * ct))

            def pareto(yy):
                t = (yy - u) / su
                G = np.where(t <= 0, 0.0, 1 - (1 + xi * np.maximum(t, 0)) ** (-1 / xi))
                return su * (np.abs(t) - 2 * (1 - self.m_u) / (1 - xi) * (1 - (1 - G) ** (1 - xi))
                             + (1 - self.m_u) ** 2 / (2 - xi))

            loss1 = s * (t1 + t2 + t3 + t4 + t5) + pareto(u)
            upper = s * (ut + t2 + t3 - 2 * (-(1 - p) * pdf(ut) + ut * P_u) + t5)
            return np.where(y < u, loss1, pareto(y) + upper)[:, 0]

    def _y_eff(self, y):
        y = np.asarray(y, dtype=np.float64)
        return np.maximum(y, self.c) if self.atom else y  # NaN stays NaN

    def pit(self, y):
        """[F(y-), F(y)] per row; NaN for NaN targets."""
        ye = self._y_eff(y)
        hi = self.cdf(ye[:, None])[:, 0]
        lo = np.where(ye == self.c, 0.0, hi) if self.atom else hi.copy()
        bad = np.isnan(ye)
        lo[bad], hi[bad] = np.nan, np.nan
        return lo, hi

    def brier(self, y, x):
        """mean over valid rows of (P(Y > x_t) - 1{y > x_t})^2 -> ([T], count)."""
        ye = self._y_eff(y)
        ok = ~np.isnan(ye)
        x = np.asarray(x, dtype=np.float64)
        d = self.sf(x)[ok] - (ye[ok, None] > x[None, :])
        with np.errstate(all="ignore"):
            return (d * d).sum(0) / ok.sum(), int(ok.sum())
