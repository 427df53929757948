"""The linear pool of several checkpoints' forecasts: one distribution out of ``M``.

A run directory holds several checkpoints.  Averaging their parameter rows ``[mu, sigma, p,
sigma_u, u]`` (what ``evaluate.predict_ensemble`` returns by default) yields a distribution
that no checkpoint predicted: the mean of the no-rain masses is no no-rain probability, the
mean of the thresholds no threshold.  The linear pool combines the forecasts themselves,

    Fbar(x) = sum_m w_m F_m(x),     sfbar(x) = sum_m w_m sf_m(x),

``F_m`` / ``sf_m`` being :class:`raincast_gnn.forecast.Forecast`'s ``cdf`` / ``exceedance`` of
member ``m``'s rows of ``preds [M, N, K]`` (``torch.stack`` of ``predict_model`` outputs; one
``kind``, ``xi``, ``c`` and fixed ``u`` for all) and ``w`` positive weights that sum to 1
(default ``1 / M``).  Members are always summed in index order, as ``w_max sum_m (w_m /
w_max) t_m``; below ``c`` the atom kinds return exactly 0 and 1.

* Quantiles / return levels are ``inf{x : Fbar(x) >= q}``: ``c`` up to the pooled atom
  ``sum_m w_m P_c,m``; otherwise the root lies between the smallest and the largest member
  quantile, is that value itself where the two agree, and else the upper end of a bracket of
  two adjacent doubles (the upper form solves ``sfbar(x) = s``, so a tiny ``s`` keeps its
  relative accuracy).
* ``crps_pool(y) = sum_m w_m crps_m(y) - V`` with the diversity ``V = int sum_m w_m (F_m -
  Fbar)^2 dx >= 0``, which depends on no target.  The first term is the members' closed forms;
  ``V`` has none for censored-normal + Pareto members and is integrated by a fixed rule
  (:meth:`ForecastPool.diversity` is its torch form): 16-point Gauss-Legendre panels
  between the sorted breakpoints ``c``, every ``u_m`` and ``mu_m + k sigma_m`` (``k`` = 0, +-1,
  +-2, +-3, +-5, +-8), and for the tail kinds one 32-point Gauss-Jacobi panel over ``[U, inf)``,
  ``U = max_m u_m``, under ``x = U + (S / xi)(1 - w) / w`` (``S = max_m sigma_u,m``), where the
  integrand is ``w^(2 / xi - 2)`` times a function analytic at ``w = 0``.
* PIT interval ``[Fbar(y-), Fbar(y)]`` and Brier scores from ``sfbar``, with ``Forecast``'s
  conventions (a target at or below ``c`` is the atom).

* The weights of minimum mean CRPS.  Summed over rows with a target, the pool's
  CRPS is the quadratic ``c . w - 1/2 w' D w``: ``c_m`` the sum of member ``m``'s CRPS, ``D_ml``
  the sum of ``int (F_m - F_l)^2 dx`` by the rule above (pointwise ``sum_m w_m (F_m - Fbar)^2 =
  1/2 sum_ml w_m w_l (F_m - F_l)^2``).  :meth:`ForecastPool.pair_sums` gives ``c`` and ``D``
  per segment of rows, :func:`solve_pool_weights` minimises over the simplex on the host, and
  :meth:`ForecastPool.fit_weights` adds K-fold cross-validation over contiguous blocks of rows
  (a fold's complement is the totals minus the fold); :meth:`ForecastPool.reweighted` is the
  pool under such weights.

HIP tensors with ``M <= 32`` go to the kernels of csrc/gine_pool.hip (``gine_pool_prob`` /
``_quantile`` / ``_score`` / ``_pairs``: one launch each); CPU tensors, and HIP tensors with more members,
take the fp64 torch formulation of the same definitions and the same rule below.  A pool of
one member, or of 2 or 4 copies of one member, returns ``Forecast``'s bits on either path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .forecast import C_DEFAULT, KINDS, _WIDTH, Forecast, ForecastScore, _ticket

MAX_KERNEL_MEMBERS = 32
GL_NODES = 16
GJ_NODES = 32
BREAK_K = (-8.0, -5.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 5.0, 8.0)
_CHUNK_NODES = 1 << 22  # evaluation points per pass of the torch rule

_jacobi_cache: dict = {}
_jacobi_device: dict = {}


def gauss_jacobi_01(alpha: float, n: int = GJ_NODES):
    """Nodes and weights of the ``n``-point Gauss rule on [0, 1] for the weight ``w^alpha``
    (``alpha > -1``) by Golub-Welsch: the eigenvalues of the Jacobi matrix of the monic Jacobi
    polynomials ``P^(0, alpha)`` on [-1, 1] and the squared first components of its
    eigenvectors, mapped by ``w = (1 + t) / 2``."""
    k = np.arange(n, dtype=np.float64)
    s = 2.0 * k + alpha
    diag = np.empty(n)
    diag[0] = alpha / (alpha + 2.0)
    diag[1:] = alpha * alpha / (s[1:] * (s[1:] + 2.0))
    j = k[1:]
    off = np.sqrt(4.0 * j * j * (j + alpha) * (j + alpha)
                  / (s[1:] * s[1:] * (s[1:] + 1.0) * (s[1:] - 1.0)))
    t, v = np.linalg.eigh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
    return (1.0 + t) / 2.0, v[0] ** 2 / (alpha + 1.0)


def tail_rule(xi: float):
    """The tail panel's nodes and weights (numpy, cached per ``xi``)."""
    r = _jacobi_cache.get(xi)
    if r is None:
        r = _jacobi_cache[xi] = gauss_jacobi_01(2.0 / xi - 2.0)
    return r


def _tail_rule_on(xi: float, device):
    key = (xi, str(device))
    r = _jacobi_device.get(key)
    if r is None:
        n, w = tail_rule(xi)
        r = _jacobi_device[key] = (torch.from_numpy(n).to(device), torch.from_numpy(w).to(device))
    return r


@dataclass
class PoolScore(ForecastScore):
    """:class:`ForecastScore` of the pool, and its decomposition ``crps_rows =
    member_crps_rows - diversity_rows``: the weighted mean of the members' CRPS (NaN where the
    target is NaN) and the diversity ``V`` of the row's members (no target needed)."""
    member_crps_rows: torch.Tensor = None
    diversity_rows: torch.Tensor = None


@dataclass
class PairSums:
    """:meth:`ForecastPool.pair_sums`: per segment, over its rows with a target, their number
    ``count [G]``, the members' summed CRPS ``member_crps [G, M]`` and the summed pairwise
    Cramer distances ``distance [G, M, M]`` (``int (F_m - F_l)^2 dx``; symmetric, the diagonal
    exactly 0).  The pool's summed CRPS under weights ``w`` is ``member_crps . w - 1/2 w'
    distance w``.  fp64 on the pool's device."""
    count: torch.Tensor
    member_crps: torch.Tensor
    distance: torch.Tensor


@dataclass
class PoolFit:
    """:meth:`ForecastPool.fit_weights` (numpy fp64, host).  ``weights [M]``: the weights of
    minimum mean CRPS over the ``count`` rows with a target; ``crps`` the mean CRPS there,
    ``crps_equal`` that of ``1 / M``, ``crps_members [M]`` the members' own, ``distance [M,
    M]`` the mean pairwise Cramer distances; ``support``, ``gap``, ``iterations`` as
    :func:`solve_pool_weights` reports them.  With folds: ``cv_weights [G, M]`` fitted on all
    rows but fold ``g``'s, and ``cv_crps`` / ``cv_crps_equal``: every fold scored under the
    weights fitted without it (under ``1 / M``), summed and divided by ``count``."""
    weights: np.ndarray
    crps: float
    crps_equal: float
    crps_members: np.ndarray
    distance: np.ndarray
    count: float
    support: list
    gap: float
    iterations: int
    cv_weights: np.ndarray = None
    cv_crps: float = None
    cv_crps_equal: float = None


def _objective(c, D, w) -> float:
    return float(c @ w - 0.5 * (w @ (D @ w)))


def solve_pool_weights(c, D):
    """Minimise ``c . w - 1/2 w' D w`` over ``{w >= 0, sum w = 1}`` (numpy fp64, host) ->
    ``(w, info)``.  ``D``: symmetric, zero diagonal, pairwise Cramer distances, which makes
    the objective convex on the simplex.

    A deterministic active-set method.  Start at the best single member (the lowest index
    among equals).  Each pass takes the gradient ``g = c - D w`` and stops when the
    Frank-Wolfe gap ``g . w - min_m g_m <= 1e-12 max|c|``, which bounds ``objective(w) -
    optimum``; otherwise the member of smallest ``g_m`` joins the support if it is outside, and the
    equality-constrained problem on the support is solved for the step from ``w`` (least
    squares, so duplicated members are no obstacle; from the gradient at ``w``, so every pass
    refines the last).  The step towards that solution is the exact line minimiser, cut
    at the first weight to reach zero; members that reach it leave the support and the solve
    is repeated.  Where the solve gives no descent direction the step goes towards the best
    vertex instead.  ``w`` is exactly ``>= 0`` and sums to 1 within 1e-15 after every step.
    ``info``: ``gap``, ``iterations`` (steps taken), ``support`` (indices with ``w > 0``).
    Raises ``RuntimeError`` after ``100 + 50 M`` steps."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    M = c.size
    D = np.asarray(D, dtype=np.float64).reshape(M, M)
    if M < 1 or not (np.isfinite(c).all() and np.isfinite(D).all()):
        raise ValueError("c [M >= 1] and D [M, M] must be finite")
    tol = 1e-12 * float(np.abs(c).max())
    w = np.zeros(M)
    w[int(np.argmin(c))] = 1.0
    cap = 100 + 50 * M
    steps = 0
    joined = False
    while True:
        g = c - D @ w
        j = int(np.argmin(g))
        gap = float(g @ w - g[j])
        if gap <= tol:
            break
        if steps >= cap:
            raise RuntimeError(f"solve_pool_weights: gap {gap:.3e} > {tol:.3e} after {cap} steps")
        support = w > 0
        if not support[j] and not joined:
            support[j] = True
        joined = False
        idx = np.flatnonzero(support)
        k = idx.size
        # the step p on the support that makes the gradient constant there: D_SS p_S + mu 1 =
        # g_S, 1' p_S = 0.  Solved for the step, not for the weights, from the gradient at w:
        # every pass refines the one before, so the solve's own rounding does not limit the gap
        A = np.zeros((k + 1, k + 1))
        A[:k, :k] = D[np.ix_(idx, idx)]
        A[:k, k] = 1.0
        A[k, :k] = 1.0
        rhs = np.append(g[idx] - g[idx].mean(), 0.0)
        p = np.zeros(M)
        p[idx] = np.linalg.lstsq(A, rhs, rcond=None)[0][:k]
        slope = float(g @ p)
        if not slope < 0.0:  # no descent on this support: towards the best vertex
            p = -w
            p[j] += 1.0
            slope = -gap
        curve = -float(p @ (D @ p))
        alpha = -slope / curve if curve > 0.0 else np.inf
        neg = p < 0.0
        bound = float((w[neg] / -p[neg]).min()) if neg.any() else np.inf
        if not np.isfinite(min(alpha, bound)):
            alpha = 1.0
        if alpha >= bound:  # the first weights to reach zero leave the support
            hit = neg & (w / np.where(neg, -p, 1.0) <= bound)
            alpha = bound
        else:
            hit = np.zeros(M, dtype=bool)
        w = w + alpha * p
        w[hit | (w < 0.0) | ~(support | (p > 0.0))] = 0.0
        w = w / w.sum()
        steps += 1
        joined = bool(hit.any())  # solve again on the smaller support before anyone joins
    return w, {"gap": gap, "iterations": steps, "support": [int(i) for i in np.flatnonzero(w > 0)]}


def _tree_sum(t: torch.Tensor, dim: int) -> torch.Tensor:
    """Sum over ``dim`` as a tree of elementwise additions over the axis padded with zeros to
    a power of two: every output depends on its own line alone, whatever the other sizes."""
    t = t.movedim(dim, -1)
    n = t.size(-1)
    size = 1 if n == 0 else 1 << (n - 1).bit_length()
    if size != n:
        t = torch.cat([t, t.new_zeros(t.shape[:-1] + (size - n,))], -1)
    while size > 1:
        size //= 2
        t = t[..., :size] + t[..., size:]
    return t[..., 0]


def _ordered(x: torch.Tensor) -> torch.Tensor:
    """Finite doubles as int64 in their own order (its own inverse)."""
    k = x.contiguous().view(torch.int64)
    return torch.where(k < 0, torch.iinfo(torch.int64).min - k, k)


def _from_ordered(k: torch.Tensor) -> torch.Tensor:
    return torch.where(k < 0, torch.iinfo(torch.int64).min - k, k).view(torch.float64)


class ForecastPool:
    """The linear pool of ``preds [M, N, K]`` (``M`` checkpoints' post-processed outputs).
    ``kind``, ``u``, ``xi``, ``c`` as :class:`Forecast`; ``weights``: ``M`` positive numbers,
    normalised to sum 1 (default ``1 / M`` each).  Results are fp64 on the predictions'
    device."""

    def __init__(self, preds: torch.Tensor, kind, u=None, xi=None, c: float = C_DEFAULT,
                 weights=None):
        k = KINDS[kind] if isinstance(kind, str) else int(kind)
        if k not in _WIDTH:
            raise ValueError(f"unknown kind {kind!r}")
        if preds.dim() != 3 or preds.size(0) < 1 or preds.size(2) != _WIDTH[k]:
            raise ValueError(f"preds must be [M >= 1, N, {_WIDTH[k]}] for this kind, got "
                             f"{tuple(preds.shape)}")
        self.preds = preds.detach().float().contiguous()
        M = self.preds.size(0)
        self._members = [Forecast(self.preds[m], k, u=u, xi=xi, c=c) for m in range(M)]
        f = self._members[0]
        self.kind, self.u, self.xi, self.c = f.kind, f.u, f.xi, f.c
        self.atom = self.kind != _lib.LOSS_NORMAL
        self.tail = self.kind in (_lib.LOSS_MIXED, _lib.LOSS_MIXED_U)
        if weights is None:
            w = np.full(M, 1.0 / M)
        else:
            w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights,
                           dtype=np.float64).reshape(-1)
            if w.size != M:
                raise ValueError(f"weights must have {M} entries, got {w.size}")
            if not (np.isfinite(w).all() and (w > 0).all()):
                raise ValueError("weights must be finite and > 0")
            w = w / w.sum()
        self._w = [float(v) for v in w]
        self.weights = torch.tensor(self._w, dtype=torch.float64, device=self.preds.device)
        self._rows_cache = None

    @classmethod
    def from_model(cls, model, stacked: torch.Tensor, weights=None) -> "ForecastPool":
        """The pool of ``stacked [M, N, K]`` (``predict_ensemble(..., stack=True)``) under the
        distribution that ``model`` predicts (``Forecast.from_model``)."""
        f = Forecast.from_model(model, stacked[0])
        tail = f.kind in (_lib.LOSS_MIXED, _lib.LOSS_MIXED_U)
        return cls(stacked, f.kind, u=f.u if f.kind == _lib.LOSS_MIXED else None,
                   xi=f.xi if tail else None, c=f.c, weights=weights)

    # ------------------------------------------------------------------ public
    @property
    def num_members(self) -> int:
        return self.preds.size(0)

    @property
    def on_kernel(self) -> bool:
        return self.preds.is_cuda and self.num_members <= MAX_KERNEL_MEMBERS

    def members(self):
        """The ``M`` member :class:`Forecast` s (views of ``preds``)."""
        return list(self._members)

    def cdf(self, x, unit: str = "model") -> torch.Tensor:
        """``Fbar(x)`` per row and threshold."""
        return self._prob(self._members[0]._thresholds(x, unit), False)

    def exceedance(self, x, unit: str = "model") -> torch.Tensor:
        """``sum_m w_m P_m(Y > x)`` per row and threshold (never ``1 - Fbar``)."""
        return self._prob(self._members[0]._thresholds(x, unit), True)

    def quantile(self, q, unit: str = "model") -> torch.Tensor:
        """``inf{x : Fbar(x) >= q}``; ``q``: ``[T]`` for all rows, or ``[N, T]`` per row."""
        return Forecast._to_unit(self._quantile(self._levels(q), False), unit)

    def return_level(self, s, unit: str = "model") -> torch.Tensor:
        """The value the pool exceeds with probability ``s`` (``[T]`` or ``[N, T]``)."""
        return Forecast._to_unit(self._quantile(self._levels(s), True), unit)

    def score(self, y: torch.Tensor, thresholds=(), unit: str = "model") -> PoolScore:
        """Scores of the targets ``y [N]`` (model space, NaN = missing) under the pool: per-row
        CRPS with its member and diversity parts, PIT interval, Brier score per threshold."""
        x = self._members[0]._thresholds(thresholds, unit)
        y = y.detach().to(self.preds.device).float().reshape(-1).contiguous()
        if y.numel() != self.preds.size(1):
            raise ValueError(f"y must have {self.preds.size(1)} entries, got {y.numel()}")
        return self._score_hip(y, x) if self.on_kernel else self._score_torch(y, x)

    def reliability(self, y: torch.Tensor, thresholds, unit: str = "model", levels: int = 1000):
        """The pool's exceedance probabilities beside the targets as a
        :class:`raincast_gnn.reliability.Reliability` (as ``Forecast.reliability``)."""
        from .reliability import Reliability
        return Reliability(self.exceedance(thresholds, unit), y,
                           self._members[0]._thresholds(thresholds, unit), levels=levels)

    def ecc(self, raw, levels: str = "uniform", unit: str = "model") -> torch.Tensor:
        """ECC-Q members ``[N, M_raw]`` from the pool: member ``i`` of ``raw`` (a
        :class:`raincast_gnn.ensemble.RawEnsemble`) becomes the pool's quantile at the level
        of its stable rank (``Forecast.ecc``); NaN where the raw member is NaN."""
        from .ensemble import LEVELS
        if levels not in LEVELS:
            raise ValueError(f"levels must be 'uniform' or 'midpoint', got {levels!r}")
        if raw.members.size(0) != self.preds.size(1):
            raise ValueError(f"the ensemble has {raw.members.size(0)} rows, the pool "
                             f"{self.preds.size(1)}")
        if raw.members.device != self.preds.device:
            raise ValueError(f"the ensemble is on {raw.members.device}, the pool on "
                             f"{self.preds.device}")
        lv = raw._levels_torch(levels).contiguous()
        return Forecast._to_unit(self._quantile(lv, False), unit)

    # ------------------------------------------------------------------ arguments
    def _levels(self, q) -> torch.Tensor:
        t = torch.as_tensor(q, dtype=torch.float64, device=self.preds.device)
        if t.dim() == 2:
            if t.size(0) != self.preds.size(1):
                raise ValueError(f"per-row levels must be [{self.preds.size(1)}, T], got "
                                 f"{tuple(t.shape)}")
            return t.contiguous()
        if t.dim() > 2:
            raise ValueError("levels must be a scalar, [T] or [N, T]")
        return t.reshape(-1).contiguous()

    # ------------------------------------------------------------------ HIP
    def _prob(self, x: torch.Tensor, upper: bool) -> torch.Tensor:
        if not self.on_kernel:
            return self._prob_torch(x.reshape(1, -1), upper)
        M, N, T = self.preds.size(0), self.preds.size(1), x.numel()
        out = torch.empty(N, T, dtype=torch.float64, device=self.preds.device)
        _lib.call("gine_pool_prob", _lib.ptr(self.preds), M, N, self.kind, self.u, self.xi, self.c,
                  _lib.ptr(self.weights), _lib.ptr(x), T, _lib.FORECAST_UPPER if upper else 0,
                  _lib.ptr(out), _lib.stream_handle(self.preds.device))
        return out

    def _quantile(self, level: torch.Tensor, upper: bool) -> torch.Tensor:
        if not self.on_kernel:
            return self._quantile_torch(level, upper)
        M, N = self.preds.size(0), self.preds.size(1)
        T = level.size(-1)
        out = torch.empty(N, T, dtype=torch.float64, device=self.preds.device)
        _lib.call("gine_pool_quantile", _lib.ptr(self.preds), M, N, self.kind, self.u, self.xi,
                  self.c, _lib.ptr(self.weights), _lib.ptr(level), T,
                  T if level.dim() == 2 else 0, _lib.FORECAST_UPPER if upper else 0,
                  _lib.ptr(out), _lib.stream_handle(self.preds.device))
        return out

    def _score_hip(self, y: torch.Tensor, x: torch.Tensor) -> PoolScore:
        dev = self.preds.device
        M, N, T = self.preds.size(0), self.preds.size(1), x.numel()
        rows = torch.empty(5, N, dtype=torch.float64, device=dev)
        brier = torch.full((T,), float("nan"), dtype=torch.float64, device=dev) if N == 0 \
            else torch.empty(T, dtype=torch.float64, device=dev)
        valid = torch.zeros(1, dtype=torch.float64, device=dev)
        count = ctypes.c_size_t(0)
        _lib.call("gine_pool_score_partials", N, T, ctypes.byref(count))
        partials = torch.empty(count.value, dtype=torch.float64, device=dev)
        gn, gw = _tail_rule_on(self.xi, dev) if self.tail else (None, None)
        _lib.call("gine_pool_score", _lib.ptr(self.preds), _lib.ptr(y), M, N, self.kind, self.u,
                  self.xi, self.c, _lib.ptr(self.weights), _lib.ptr(x), T, _lib.ptr(gn),
                  _lib.ptr(gw), _lib.ptr(rows[0]), _lib.ptr(rows[1]), _lib.ptr(rows[2]),
                  _lib.ptr(rows[3]), _lib.ptr(rows[4]), _lib.ptr(brier), _lib.ptr(valid),
                  _lib.ptr(partials), _lib.ptr(_ticket(dev)), _lib.stream_handle(dev))
        return PoolScore(rows[0], rows[3], rows[4], brier, valid, rows[1], rows[2])

    # ------------------------------------------------------------------ torch (fp64)
    def _rows(self):
        if self._rows_cache is None:
            self._rows_cache = [f._rows() for f in self._members]
        return self._rows_cache

    def _wsum(self, terms):
        """sum_m w_m term_m in index order, formed as w_max sum_m (w_m / w_max) term_m (the
        first term starts the sum): with equal weights the ratios are 1, so 2 or 4 copies of
        one member give that member's bits even where a term is subnormal."""
        wmax = max(self._w)
        acc = None
        for w, t in zip(self._w, terms):
            acc = (w / wmax) * t if acc is None else acc + (w / wmax) * t
        return wmax * acc

    def _prob_torch(self, x: torch.Tensor, upper: bool, rows=None) -> torch.Tensor:
        """Fbar or sfbar at x [N, T] or [1, T]."""
        rs = self._rows() if rows is None else rows
        out = self._wsum(f._prob_rows(r, x, upper) for f, r in zip(self._members, rs))
        if self.atom:  # exactly, whatever the weights round to
            out = torch.where(x < self.c, torch.full_like(out, 1.0 if upper else 0.0), out)
        return out

    def _quantile_torch(self, level: torch.Tensor, upper: bool) -> torch.Tensor:
        N = self.preds.size(1)
        lv = level if level.dim() == 2 else level.reshape(1, -1).expand(N, -1)
        inf = float("inf")
        qs = [f._quantile_cpu(lv, upper) for f in self._members]
        lo, hi = qs[0], qs[0]
        for q in qs[1:]:
            lo, hi = torch.minimum(lo, q), torch.maximum(hi, q)

        def good(x):  # h(x) >= 0, h increasing: Fbar(x) - q, or s - sfbar(x)
            f = self._prob_torch(x, upper)
            return (lv - f >= 0) if upper else (f - lv >= 0)

        # the least x with h(x) >= 0 in [lo, hi]: lo itself if h(lo) >= 0, else bisection
        # between the two in the order of the doubles' bits, to adjacent doubles
        solve = torch.isfinite(lo) & torch.isfinite(hi) & (lo < hi)
        a = _ordered(torch.where(solve, lo, torch.zeros_like(lo)))
        b = _ordered(torch.where(solve, hi, torch.ones_like(hi)))
        solve = solve & ~good(_from_ordered(a))
        for _ in range(64):
            mid = (a >> 1) + (b >> 1) + (a & b & 1)
            g = good(_from_ordered(mid))
            move = solve & (mid != a)
            b = torch.where(move & g, mid, b)
            a = torch.where(move & ~g, mid, a)
        x = torch.where(solve, _from_ordered(b), lo)
        if self.atom:
            rs = self._rows()
            mass = self._wsum(r["Sc" if upper else "Pc"] for r in rs)
            at = (lv >= mass) if upper else (lv <= mass)
            x = torch.where(at, torch.full_like(x, self.c), x)
        else:
            x = torch.where(lv == (1.0 if upper else 0.0), torch.full_like(x, -inf), x)
        x = torch.where(lv == (0.0 if upper else 1.0), torch.full_like(x, inf), x)
        bad = ~((lv >= 0.0) & (lv <= 1.0))
        return torch.where(bad, torch.full_like(x, float("nan")), x)

    def _var_torch(self, rs, x: torch.Tensor, upper: bool) -> torch.Tensor:
        """sum_m w_m (F_m - Fbar)^2 at x [n, P], in two passes (equal members: exactly 0)."""
        fs = [f._prob_rows(r, x, upper) for f, r in zip(self._members, rs)]
        fb = self._wsum(fs)
        return self._wsum((f - fb) * (f - fb) for f in fs)

    def _rule_chunks(self):
        """The rule's nodes, in row chunks of at most ``_CHUNK_NODES`` evaluation points: yields
        ``(sl, rs, xq, wq, xt, S)`` -- the row slice, the members' rows there, the body's
        nodes and weights ``[n, 16 (nb - 1)]`` (an empty panel has weight 0), and for the tail
        kinds the tail panel's nodes ``xt [n, 32]`` and the map's scale ``S [n, 1]``, else
        ``None``."""
        dev = self.preds.device
        N, M = self.preds.size(1), self.preds.size(0)
        nb = len(BREAK_K) * M + (M if self.tail else 0) + (1 if self.atom else 0)
        per_row = GL_NODES * (nb - 1) + GJ_NODES
        step = max(1, _CHUNK_NODES // per_row)
        gx, gw = np.polynomial.legendre.leggauss(GL_NODES)
        gx = torch.from_numpy(gx).to(dev)
        gw = torch.from_numpy(gw).to(dev)
        ks = torch.tensor(BREAK_K, dtype=torch.float64, device=dev)
        for s in range(0, N, step):
            sl = slice(s, min(N, s + step))
            rs = [{k: (v[sl] if torch.is_tensor(v) else v) for k, v in r.items()}
                  for r in self._rows()]
            n = sl.stop - sl.start
            mu = torch.cat([r["mu"] for r in rs], 1)            # [n, M]
            sg = torch.cat([r["sigma"] for r in rs], 1)
            bp = [(mu.unsqueeze(2) + ks * sg.unsqueeze(2)).reshape(n, -1)]
            lo, hi = bp[0].min(1, keepdim=True).values, bp[0].max(1, keepdim=True).values
            if self.tail:
                us = torch.cat([r["u"] for r in rs], 1)
                bp.append(us)
                hi = us.max(1, keepdim=True).values              # U
            if self.atom:
                cc = torch.full((n, 1), self.c, dtype=torch.float64, device=dev)
                bp.append(cc)
                lo = cc
                if not self.tail:
                    hi = torch.maximum(hi, cc)
            bp = torch.minimum(torch.maximum(torch.cat(bp, 1), lo), hi).sort(1).values
            a, b = bp[:, :-1], bp[:, 1:]
            half, mid = 0.5 * (b - a), 0.5 * (a + b)
            xq = (mid.unsqueeze(2) + half.unsqueeze(2) * gx).reshape(n, -1)
            wq = (half.unsqueeze(2) * gw).reshape(n, -1)
            xt = S = None
            if self.tail:
                wn, _ = _tail_rule_on(self.xi, dev)
                S = torch.cat([r["su"] for r in rs], 1).max(1, keepdim=True).values
                xt = hi + (S / self.xi) * ((1.0 - wn) / wn)
            yield sl, rs, xq, wq, xt, S

    def diversity(self) -> torch.Tensor:
        """``V [N]`` by the fixed rule of the module docstring (the torch formulation)."""
        dev = self.preds.device
        out = torch.empty(self.preds.size(1), dtype=torch.float64, device=dev)
        for sl, rs, xq, wq, xt, S in self._rule_chunks():
            V = (wq * self._var_torch(rs, xq, False)).sum(1)
            if self.tail:
                wn, ww = _tail_rule_on(self.xi, dev)
                g = self._var_torch(rs, xt, True) * (S / self.xi) * torch.pow(wn, -2.0 / self.xi)
                V = V + (ww * g).sum(1)
            out[sl] = V
        return out

    # ------------------------------------------------------------------ fitting the weights
    def _segments(self, folds) -> np.ndarray:
        """``folds`` as the int64 row pointer ``[G + 1]`` of contiguous segments."""
        N = self.preds.size(1)
        if folds is None:
            return np.array([0, N], dtype=np.int64)
        if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
            if folds < 1:
                raise ValueError(f"folds must be >= 1, got {folds}")
            size = -(-N // int(folds))
            return np.minimum(np.arange(int(folds) + 1, dtype=np.int64) * size, N)
        if torch.is_tensor(folds):
            if folds.is_cuda or folds.dtype != torch.int64:
                raise ValueError("a folds tensor must be int64 on the CPU")
            ptr = folds.detach().numpy().reshape(-1).copy()
        else:
            ptr = np.asarray(folds)
            if ptr.dtype.kind not in "iu" or ptr.ndim != 1:
                raise ValueError("folds must be None, an int or a sequence of row offsets")
            ptr = ptr.astype(np.int64)
        if ptr.size < 2:
            raise ValueError("a row pointer needs at least one segment")
        if ptr[0] != 0 or ptr[-1] != N:
            raise ValueError(f"a row pointer must start at 0 and end at {N}, got {ptr[0]} and "
                             f"{ptr[-1]}")
        if (np.diff(ptr) < 0).any():
            raise ValueError("a row pointer must not decrease")
        return ptr

    def pair_sums(self, y: torch.Tensor, folds=None) -> "PairSums":
        """What the pool's CRPS needs as a function of the weights (:class:`PairSums`), summed
        over the rows with a target (``y [N]``, model space, NaN = missing) of each segment.
        ``folds``: ``None`` (one segment), an int ``K`` (``K`` contiguous blocks of
        ``ceil(N / K)`` rows, the last shorter or empty), or a row pointer ``[G + 1]`` (a host
        sequence or a CPU int64 tensor: starts at 0, does not decrease, ends at ``N``)."""
        ptr = self._segments(folds)
        y = y.detach().to(self.preds.device).float().reshape(-1).contiguous()
        if y.numel() != self.preds.size(1):
            raise ValueError(f"y must have {self.preds.size(1)} entries, got {y.numel()}")
        if self.on_kernel:
            count, cbar, dist = self._pairs_hip(y, torch.from_numpy(ptr).to(self.preds.device))
        else:
            count, cbar, dist = self._pairs_torch(y, ptr)
        M, G = self.num_members, ptr.size - 1
        D = torch.zeros(G, M, M, dtype=torch.float64, device=self.preds.device)
        if M > 1:
            iu = torch.triu_indices(M, M, 1, device=self.preds.device)  # (0,1), (0,2), ...
            D[:, iu[0], iu[1]] = dist
            D[:, iu[1], iu[0]] = dist
        return PairSums(count, cbar, D)

    def _pairs_hip(self, y: torch.Tensor, ptr: torch.Tensor):
        """One launch of gine_pool_pairs; ``ptr``: the validated row pointer, int64 on the device."""
        dev = self.preds.device
        M, N, G = self.preds.size(0), self.preds.size(1), ptr.numel() - 1
        P = M * (M - 1) // 2
        out = torch.zeros(G * (1 + M + P), dtype=torch.float64, device=dev)
        count, cbar, dist = out[:G], out[G:G + G * M].view(G, M), out[G + G * M:].view(G, P)
        if N == 0:
            return count, cbar, dist
        size = ctypes.c_size_t(0)
        _lib.call("gine_pool_pairs_partials", N, M, G, ctypes.byref(size))
        partials = torch.empty(size.value, dtype=torch.float64, device=dev)
        gn, gw = _tail_rule_on(self.xi, dev) if self.tail else (None, None)
        _lib.call("gine_pool_pairs", _lib.ptr(self.preds), _lib.ptr(y), M, N, self.kind, self.u,
                  self.xi, self.c, _lib.ptr(gn), _lib.ptr(gw), _lib.ptr(ptr), G, _lib.ptr(count),
                  _lib.ptr(cbar), _lib.ptr(dist) if P else None, _lib.ptr(partials),
                  _lib.ptr(_ticket(dev)), _lib.stream_handle(dev))
        return count, cbar, dist

    def _pairs_torch(self, y: torch.Tensor, ptr: np.ndarray):
        """The kernel's definition in torch: per row every pair's ``sum_nodes wq (F_m - F_l)
        (F_m - F_l)`` over the rule's nodes and every member's closed-form CRPS, then the rows
        with a target added per segment.  Every sum is a tree of elementwise additions over a
        zero-padded axis, so a row's values depend on that row alone and a segment's on its own
        rows alone."""
        dev = self.preds.device
        M, N, G = self.preds.size(0), self.preds.size(1), ptr.size - 1
        P = M * (M - 1) // 2
        ok = ~torch.isnan(y)
        y1 = torch.where(ok, y, torch.zeros_like(y)).double().unsqueeze(1)
        rows_c = torch.stack([f._crps_cpu(r, y1).squeeze(1)
                              for f, r in zip(self._members, self._rows())], 1)   # [N, M]
        rows_d = torch.zeros(N, P, dtype=torch.float64, device=dev)
        if P:
            for sl, rs, xq, wq, xt, S in self._rule_chunks():
                fs = [f._prob_rows(r, xq, False) for f, r in zip(self._members, rs)]
                if self.tail:
                    wn, ww = _tail_rule_on(self.xi, dev)
                    ss = [f._prob_rows(r, xt, True) for f, r in zip(self._members, rs)]
                    wt = ww * ((S / self.xi) * torch.pow(wn, -2.0 / self.xi))
                p = 0
                for m in range(M):
                    for l in range(m + 1, M):
                        d = fs[m] - fs[l]
                        v = _tree_sum(wq * d * d, 1)
                        if self.tail:
                            d = ss[m] - ss[l]
                            v = v + _tree_sum(wt * d * d, 1)
                        rows_d[sl, p] = v
                        p += 1
        keep = ok.unsqueeze(1)
        rows_c = torch.where(keep, rows_c, torch.zeros_like(rows_c))
        rows_d = torch.where(keep, rows_d, torch.zeros_like(rows_d))
        count = torch.zeros(G, dtype=torch.float64, device=dev)
        cbar = torch.zeros(G, M, dtype=torch.float64, device=dev)
        dist = torch.zeros(G, P, dtype=torch.float64, device=dev)
        for g in range(G):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b > a:
                count[g] = ok[a:b].sum()
                cbar[g] = _tree_sum(rows_c[a:b], 0)
                dist[g] = _tree_sum(rows_d[a:b], 0)
        return count, cbar, dist

    def fit_weights(self, y: torch.Tensor, folds=None) -> "PoolFit":
        """The weights of minimum mean CRPS over the rows with a target (:class:`PoolFit`), by
        :func:`solve_pool_weights` on :meth:`pair_sums`; with ``folds`` also the weights fitted
        without each fold and the CRPS of every fold under the weights fitted without it."""
        ps = self.pair_sums(y, folds)
        count = ps.count.cpu().numpy()
        cs, Ds = ps.member_crps.cpu().numpy(), ps.distance.cpu().numpy()
        M = self.num_members
        total = float(count.sum())
        if total == 0.0:
            raise ValueError("no row has a target")
        c, D = cs.sum(0), Ds.sum(0)
        equal = np.full(M, 1.0 / M)
        w, info = solve_pool_weights(c, D)
        fit = PoolFit(weights=w, crps=_objective(c, D, w) / total,
                      crps_equal=_objective(c, D, equal) / total, crps_members=c / total,
                      distance=D / total, count=total, support=info["support"],
                      gap=info["gap"], iterations=info["iterations"])
        if folds is None:
            return fit
        G = count.size
        fit.cv_weights = np.zeros((G, M))
        held = held_equal = 0.0
        for g in range(G):
            if total - count[g] == 0.0:
                raise ValueError(f"no row outside fold {g} has a target")
            fit.cv_weights[g], _ = solve_pool_weights(c - cs[g], D - Ds[g])
            held += _objective(cs[g], Ds[g], fit.cv_weights[g])
            held_equal += _objective(cs[g], Ds[g], equal)
        fit.cv_crps, fit.cv_crps_equal = held / total, held_equal / total
        return fit

    def reweighted(self, weights) -> "ForecastPool":
        """The pool of the members with ``weights > 0`` under those weights (the constructor
        takes positive weights only: a member of weight 0 is no member)."""
        w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights,
                       dtype=np.float64).reshape(-1)
        if w.size != self.num_members:
            raise ValueError(f"weights must have {self.num_members} entries, got {w.size}")
        if not (np.isfinite(w).all() and (w >= 0).all() and (w > 0).any()):
            raise ValueError("weights must be finite, >= 0 and not all 0")
        keep = np.flatnonzero(w > 0)
        return ForecastPool(self.preds[torch.from_numpy(keep).to(self.preds.device)], self.kind,
                            u=self.u if self.kind == _lib.LOSS_MIXED else None,
                            xi=self.xi if self.tail else None, c=self.c, weights=w[keep])

    def _score_torch(self, y: torch.Tensor, x: torch.Tensor) -> PoolScore:
        rs = self._rows()
        dev = self.preds.device
        ok = ~torch.isnan(y)
        nan = torch.full((y.numel(),), float("nan"), dtype=torch.float64, device=dev)
        y1 = torch.where(ok, y, torch.zeros_like(y)).double().unsqueeze(1)
        ye = torch.clamp(y1, min=self.c) if self.atom else y1
        V = self.diversity()
        mc = self._wsum(f._crps_cpu(r, y1).squeeze(1) for f, r in zip(self._members, rs))
        hi = self._prob_torch(ye, False).squeeze(1)
        lo = torch.where(ye.squeeze(1) == self.c, torch.zeros_like(hi), hi) if self.atom else hi
        sf = self._prob_torch(x.reshape(1, -1), True)                 # [N, T]
        d = sf - (ye > x.reshape(1, -1)).double()
        valid = ok.sum().double().reshape(1)
        brier = torch.where(ok.unsqueeze(1), d * d, torch.zeros_like(d)).sum(0) / valid
        return PoolScore(torch.where(ok, mc - V, nan), torch.where(ok, lo, nan),
                         torch.where(ok, hi, nan), brier, valid, torch.where(ok, mc, nan), V)
