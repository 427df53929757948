"""Independent fp64 oracle of the linear pool (numpy + scipy only): the member distributions
of tests/forecast_oracle.py, summed with the weights.

``params``: [M, N, K]; ``weights``: [M], summing to 1 (default 1 / M).  ``cdf`` / ``sf`` are
``sum_m w_m F_m`` / ``sum_m w_m sf_m``; ``P_c`` / ``S_c`` the pooled atom and the mass above
it; ``pit`` / ``brier`` as ``Dist``'s from the pooled probabilities; ``member_crps_rows`` the
weighted mean of the members' closed-form CRPS.  The pool's own CRPS has no closed form: its
reference is tests/golden/pool_crps_rows.npz (direct integrals by mpmath).
"""
import numpy as np

from forecast_oracle import C, Dist


class PoolDist:
    def __init__(self, kind, params, u=None, xi=None, weights=None, c=C):
        P = np.asarray(params, dtype=np.float64)
        self.members = [Dist(kind, P[m], u=u, xi=xi, c=c) for m in range(P.shape[0])]
        M = len(self.members)
        self.w = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, dtype=np.float64)
        self.kind, self.c = kind, float(c)
        self.atom, self.tail = self.members[0].atom, self.members[0].tail
        if self.atom:
            self.P_c = sum(w * d.P_c for w, d in zip(self.w, self.members))
            self.S_c = sum(w * d.S_c for w, d in zip(self.w, self.members))

    def cdf(self, x):
        return sum(w * d.cdf(x) for w, d in zip(self.w, self.members))

    def sf(self, x):
        return sum(w * d.sf(x) for w, d in zip(self.w, self.members))

    def member_crps_rows(self, y):
        return sum(w * d.crps_rows(y) for w, d in zip(self.w, self.members))

    def _y_eff(self, y):
        y = np.asarray(y, dtype=np.float64)
        return np.maximum(y, self.c) if self.atom else y  # NaN stays NaN

    def pit(self, y):
        ye = self._y_eff(y)
        hi = self.cdf(ye[:, None])[:, 0]
        lo = np.where(ye == self.c, 0.0, hi) if self.atom else hi.copy()
        bad = np.isnan(ye)
        lo[bad], hi[bad] = np.nan, np.nan
        return lo, hi

    def brier(self, y, x):
        ye = self._y_eff(y)
        ok = ~np.isnan(ye)
        x = np.asarray(x, dtype=np.float64)
        d = self.sf(x)[ok] - (ye[ok, None] > x[None, :])
        with np.errstate(all="ignore"):
            return (d * d).sum(0) / ok.sum(), int(ok.sum())
