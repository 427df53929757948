"""The predictive distribution behind a prediction: probabilities, quantiles, scores.

The model's output is the parameter row of a distribution of ``y = log(mm + 0.01)``: the one
whose CRPS the losses of :mod:`raincast_gnn.loss` are (integrating ``(F(x) - 1{x >= y})^2``
reproduces the reference's per-row values, tests/test_forecast.py).  With ``c`` the censoring
point (``log 0.01``, 0 mm), ``z(x) = (x - mu) / sigma`` and ``Phi`` the normal cdf:

* ``normal`` ``[mu, sigma]``: ``F(x) = Phi(z)``;
* ``mixed_normal`` ``[mu, sigma, p]``: ``F(x) = 0`` below ``c`` and ``p + (1 - p) Phi(z)`` from
  ``c`` on, so there is an atom ``P_c = F(c)`` at ``c`` (the probability of no rain);
* ``mixed`` ``[mu, sigma, p, sigma_u]`` (fixed ``u``) and ``mixed_u`` ``[..., u]`` (the row's own
  ``u``): as ``mixed_normal`` below ``u``; for ``x >= u`` ``m_u + (1 - m_u) G((x - u) / sigma_u)``
  with ``m_u = p + (1 - p) Phi(z(u))`` and ``G(t) = 1 - (1 + xi t)^(-1/xi)``.

It is defined for ``c < u`` and ``0 < xi < 1``.  ``F`` is right-continuous (``P(Y <= x)``); the
quantile is the generalised inverse ``inf{x : F(x) >= q}`` (``c`` for every ``q <= P_c``).
For a learned ``u`` the score is the CRPS of this distribution, ``where(y < u, ...)``, not the
sigmoid blend that training uses as its smooth surrogate.

HIP tensors go to the kernels of csrc/gine_forecast.hip (``gine_forecast_prob`` /
``_quantile`` / ``_score``: one launch each, fp64, nothing that a HIP graph could not record
when the thresholds are device tensors already); CPU tensors go to the fp64 torch
formulation of the same formulas below, as :mod:`raincast_gnn.loss` keeps one.

Units: ``unit="model"`` is ``y`` itself, ``unit="mm"`` converts thresholds with
``log(mm + 0.01)`` and quantiles with ``max(exp(y) - 0.01, 0)``.  The two constants are the
reference's target transform (its data pipeline stores ``log(precipitation + 0.01)``, and the
losses' ``c = log(0.01)``); a model trained on another transform needs ``unit="model"``.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

C_DEFAULT = math.log(0.01)
MM_OFFSET = 0.01
KINDS = {"normal": _lib.LOSS_NORMAL, "mixed_normal": _lib.LOSS_MIXED_NORMAL,
         "mixed": _lib.LOSS_MIXED, "mixed_u": _lib.LOSS_MIXED_U}
_WIDTH = {_lib.LOSS_NORMAL: 2, _lib.LOSS_MIXED_NORMAL: 3, _lib.LOSS_MIXED: 4,
          _lib.LOSS_MIXED_U: 5}
_SQRT2 = math.sqrt(2.0)
_LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
_INV_SQRT_PI = 1.0 / math.sqrt(math.pi)

_tickets: dict = {}


def _ticket(device) -> torch.Tensor:
    """Per-device work counter of gine_forecast_score (zeroed once, left at 0 by every call)."""
    key = str(device)
    t = _tickets.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=device)
        _tickets[key] = t
    return t


@dataclass
class ForecastScore:
    """Verification of a set of targets: per row the CRPS and the PIT interval
    ``[F(y-), F(y)]`` (NaN where the target is NaN), per threshold the Brier score over the
    valid rows, and their number ``valid`` (a 1-element fp64 tensor)."""
    crps_rows: torch.Tensor
    pit_lo: torch.Tensor
    pit_hi: torch.Tensor
    brier: torch.Tensor
    valid: torch.Tensor

    @property
    def crps(self) -> torch.Tensor:
        """Mean CRPS over the valid rows (NaN when there is none)."""
        return torch.nansum(self.crps_rows) / self.valid[0]


@dataclass
class TwScore:
    """Threshold-weighted CRPS of a set of targets (:mod:`raincast_gnn.twcrps`): ``mean [T]``
    over the ``valid`` rows (a 1-element fp64 tensor; NaN means when there is none), ``rows
    [N, T]`` (NaN where the target is NaN) when asked for, and the ``thresholds [T]`` in model
    space."""
    mean: torch.Tensor
    valid: torch.Tensor
    rows: torch.Tensor | None
    thresholds: torch.Tensor


def pit_sample(lo: torch.Tensor, hi: torch.Tensor, generator=None) -> torch.Tensor:
    """The randomised PIT ``lo + U (hi - lo)``, ``U`` uniform on [0, 1): uniform under a
    calibrated forecast, atoms included (for a histogram).  NaN rows stay NaN."""
    u = torch.rand(lo.shape, dtype=lo.dtype, device=lo.device, generator=generator)
    return lo + u * (hi - lo)


def _upper_phi(z):
    return 0.5 * torch.special.erfc(z / _SQRT2)


def _lower_phi(z):
    return 0.5 * torch.special.erfc(-z / _SQRT2)


def _Phi(z):  # as the loss writes it
    return 0.5 * (1 + torch.erf(z / _SQRT2))


def _phi(z):
    return torch.exp(-0.5 * z * z - _LOG_SQRT_2PI)


def _upper_phi_inv(v):
    """z with upper_phi(z) = v."""
    return -torch.special.ndtri(v)


class Forecast:
    """The distribution of each row of ``pred [N, K]`` (post-processed model output).

    ``kind``: ``"normal"``, ``"mixed_normal"``, ``"mixed"``, ``"mixed_u"`` or the matching
    ``GINE_LOSS_*`` value.  ``u``: the fixed threshold of ``"mixed"``; ``xi``: the tail shape of
    the two mixed kinds; ``c``: the censoring point.  Results are fp64 tensors on the
    prediction's device, ``[N, T]`` for ``T`` thresholds or levels."""

    def __init__(self, pred: torch.Tensor, kind, u=None, xi=None, c: float = C_DEFAULT):
        self.kind = KINDS[kind] if isinstance(kind, str) else int(kind)
        if self.kind not in _WIDTH:
            raise ValueError(f"unknown kind {kind!r}")
        if pred.dim() != 2 or pred.size(1) != _WIDTH[self.kind]:
            raise ValueError(f"pred must be [N, {_WIDTH[self.kind]}] for this kind, got "
                             f"{tuple(pred.shape)}")
        self.pred = pred.detach().float().contiguous()
        self.c = float(c)
        self.u = 0.0 if u is None else float(u)
        self.xi = 0.5 if xi is None else float(xi)
        if self.kind in (_lib.LOSS_MIXED, _lib.LOSS_MIXED_U):
            if xi is None or not 0.0 < self.xi < 1.0:
                raise ValueError(f"the mixed kinds need 0 < xi < 1, got {xi!r}")
            if self.kind == _lib.LOSS_MIXED and (u is None or not self.u > self.c):
                raise ValueError(f"kind 'mixed' needs a fixed u > c, got {u!r}")
            if self.kind == _lib.LOSS_MIXED_U and not self.c < 0.0:
                raise ValueError("kind 'mixed_u' needs c < 0 (its u lies in (0, 2.12))")

    @classmethod
    def from_model(cls, model, pred: torch.Tensor) -> "Forecast":
        """The distribution that ``model`` (``models.GNN`` or anything with its ``loss``,
        ``grad_u``, ``u``, ``xi`` attributes, as read from a params.json) predicts.  ``grad_u``
        is the params.json string; ``u`` and ``xi`` are rounded to fp32 as the loss rounds them."""
        loss = model.loss
        c = getattr(getattr(model, "loss_fn", None), "c", C_DEFAULT)
        if loss == "NormalCRPS":
            return cls(pred, _lib.LOSS_NORMAL, c=C_DEFAULT)
        if loss == "MixedNormalCRPS":
            return cls(pred, _lib.LOSS_MIXED_NORMAL, c=float(c))
        if loss == "MixedLoss":
            xi = float(np.float32(model.xi))
            if model.grad_u == "True":
                return cls(pred, _lib.LOSS_MIXED_U, xi=xi, c=float(c))
            return cls(pred, _lib.LOSS_MIXED, u=float(np.float32(model.u)), xi=xi, c=float(c))
        raise ValueError(f"unknown loss '{loss}'")

    # ------------------------------------------------------------------ arguments
    def _points(self, x) -> torch.Tensor:
        t = torch.as_tensor(x, dtype=torch.float64, device=self.pred.device)
        if t.dim() > 1:
            raise ValueError("thresholds / levels must be a scalar or one-dimensional")
        return t.reshape(-1).contiguous()

    def _thresholds(self, x, unit: str) -> torch.Tensor:
        t = self._points(x)
        if unit == "mm":  # log(mm + 0.01); at or below -0.01 mm: below every value
            return torch.log(torch.clamp(t + MM_OFFSET, min=0.0))
        if unit != "model":
            raise ValueError(f"unit must be 'model' or 'mm', got {unit!r}")
        return t

    @staticmethod
    def _to_unit(y: torch.Tensor, unit: str) -> torch.Tensor:
        if unit == "mm":
            return torch.clamp(torch.exp(y) - MM_OFFSET, min=0.0)
        if unit != "model":
            raise ValueError(f"unit must be 'model' or 'mm', got {unit!r}")
        return y

    # ------------------------------------------------------------------ public
    def cdf(self, x, unit: str = "model") -> torch.Tensor:
        """``P(Y <= x)`` per row and threshold."""
        return self._prob(self._thresholds(x, unit), False)

    def exceedance(self, x, unit: str = "model") -> torch.Tensor:
        """``P(Y > x)`` per row and threshold, accurate where it is tiny (no ``1 - F``)."""
        return self._prob(self._thresholds(x, unit), True)

    def quantile(self, q, unit: str = "model") -> torch.Tensor:
        """``inf{x : F(x) >= q}`` per row and level; ``c`` (0 mm) up to the atom's mass."""
        return self._to_unit(self._quantile(self._points(q), False), unit)

    def return_level(self, s, unit: str = "model") -> torch.Tensor:
        """The value exceeded with probability ``s`` (the quantile at ``1 - s`` without forming
        ``1 - s``: meaningful down to ``s = 1e-12``)."""
        return self._to_unit(self._quantile(self._points(s), True), unit)

    def score(self, y: torch.Tensor, thresholds=(), unit: str = "model") -> ForecastScore:
        """Scores of the targets ``y [N]`` (model space, NaN = missing): per-row CRPS and PIT
        interval, Brier score of ``P(Y > threshold)`` per threshold (``unit``: the
        thresholds').  For the PIT and the Brier score a target at or below ``c`` is the atom."""
        x = self._thresholds(thresholds, unit)
        y = y.detach().to(self.pred.device).float().reshape(-1).contiguous()
        if y.numel() != self.pred.size(0):
            raise ValueError(f"y must have {self.pred.size(0)} entries, got {y.numel()}")
        if self.pred.is_cuda:
            return self._score_hip(y, x)
        return self._score_cpu(y, x)

    def twcrps(self, y: torch.Tensor, thresholds, unit: str = "model",
               rows: bool = False) -> TwScore:
        """Threshold-weighted CRPS of the targets ``y [N]`` (model space, NaN = missing) at each
        threshold (``unit``: the thresholds'), weight ``1{x >= t}``: the part of the CRPS integral
        above ``t`` (:mod:`raincast_gnn.twcrps`).  ``rows``: also the per-row values."""
        x = self._thresholds(thresholds, unit)
        y = y.detach().to(self.pred.device).float().reshape(-1).contiguous()
        if y.numel() != self.pred.size(0):
            raise ValueError(f"y must have {self.pred.size(0)} entries, got {y.numel()}")
        if self.pred.is_cuda:
            return self._twcrps_hip(y, x, rows)
        return self._twcrps_cpu(y, x, rows)

    def reliability(self, y: torch.Tensor, thresholds, unit: str = "model", levels: int = 1000):
        """The exceedance probabilities at ``thresholds`` (``unit``: theirs) beside the targets
        ``y [N]`` (model space, NaN = missing) as a :class:`raincast_gnn.reliability.Reliability`
        on a lattice of ``levels`` steps: CORP reliability curve, MCB / DSC / UNC, consistency
        bands."""
        from .reliability import Reliability
        return Reliability(self.exceedance(thresholds, unit), y, self._thresholds(thresholds, unit),
                           levels=levels)

    def ecc(self, raw, levels: str = "uniform", unit: str = "model") -> torch.Tensor:
        """Ensemble copula coupling (ECC-Q): the post-processed members ``[N, M]``.  Member
        ``i`` of ``raw`` (a :class:`raincast_gnn.ensemble.RawEnsemble`) is replaced by this
        distribution's quantile at the level of its stable rank ``r`` among the row's ``m``
        valid members, ``r / (m + 1)`` (``"uniform"``) or ``(r - 0.5) / m`` (``"midpoint"``),
        so the members keep the raw ensemble's rank structure across stations; NaN where the
        raw member is NaN."""
        from .ensemble import ecc
        return self._to_unit(ecc(self, raw, levels), unit)

    # ------------------------------------------------------------------ HIP
    def _prob(self, x: torch.Tensor, upper: bool) -> torch.Tensor:
        if not self.pred.is_cuda:
            return self._prob_cpu(x, upper)
        return self._launch_points("gine_forecast_prob", x, upper)

    def _quantile(self, q: torch.Tensor, upper: bool) -> torch.Tensor:
        if not self.pred.is_cuda:
            return self._quantile_cpu(q, upper)
        return self._launch_points("gine_forecast_quantile", q, upper)

    def _launch_points(self, name: str, x: torch.Tensor, upper: bool) -> torch.Tensor:
        N, T = self.pred.size(0), x.numel()
        out = torch.empty(N, T, dtype=torch.float64, device=self.pred.device)
        _lib.call(name, _lib.ptr(self.pred), N, self.kind, self.u, self.xi, self.c, _lib.ptr(x),
                  T, _lib.FORECAST_UPPER if upper else 0, _lib.ptr(out),
                  _lib.stream_handle(self.pred.device))
        return out

    def _score_hip(self, y: torch.Tensor, x: torch.Tensor) -> ForecastScore:
        dev = self.pred.device
        N, T = self.pred.size(0), x.numel()
        rows = torch.empty(3, N, dtype=torch.float64, device=dev)
        brier = torch.full((T,), float("nan"), dtype=torch.float64, device=dev) if N == 0 \
            else torch.empty(T, dtype=torch.float64, device=dev)
        valid = torch.zeros(1, dtype=torch.float64, device=dev)
        count = ctypes.c_size_t(0)
        _lib.call("gine_forecast_score_partials", N, T, ctypes.byref(count))
        partials = torch.empty(count.value, dtype=torch.float64, device=dev)
        _lib.call("gine_forecast_score", _lib.ptr(self.pred), _lib.ptr(y), N, self.kind, self.u,
                  self.xi, self.c, _lib.ptr(x), T, _lib.ptr(rows[0]), _lib.ptr(rows[1]),
                  _lib.ptr(rows[2]), _lib.ptr(brier), _lib.ptr(valid), _lib.ptr(partials),
                  _lib.ptr(_ticket(dev)), _lib.stream_handle(dev))
        return ForecastScore(rows[0], rows[1], rows[2], brier, valid)

    def _twcrps_hip(self, y: torch.Tensor, x: torch.Tensor, rows: bool) -> TwScore:
        dev = self.pred.device
        N, T = self.pred.size(0), x.numel()
        out = torch.empty(N, T, dtype=torch.float64, device=dev) if rows else None
        mean = torch.full((T,), float("nan"), dtype=torch.float64, device=dev) if N == 0 \
            else torch.empty(T, dtype=torch.float64, device=dev)
        valid = torch.zeros(1, dtype=torch.float64, device=dev)
        count = ctypes.c_size_t(0)
        _lib.call("gine_forecast_twcrps_partials", N, T, ctypes.byref(count))
        partials = torch.empty(count.value, dtype=torch.float64, device=dev)
        _lib.call("gine_forecast_twcrps", _lib.ptr(self.pred), _lib.ptr(y), N, self.kind, self.u,
                  self.xi, self.c, _lib.ptr(x), T, _lib.ptr(out), _lib.ptr(mean), _lib.ptr(valid),
                  _lib.ptr(partials), _lib.ptr(_ticket(dev)), _lib.stream_handle(dev))
        return TwScore(mean, valid, out, x)

    # ------------------------------------------------------------------ CPU (fp64 torch)
    def _twcrps_cpu(self, y: torch.Tensor, x: torch.Tensor, rows: bool) -> TwScore:
        from .twcrps import tw_rows_of
        ok = ~torch.isnan(y)
        y1 = torch.where(ok, y, torch.zeros_like(y)).double().unsqueeze(1)
        r = tw_rows_of(self.kind, self.pred, y1, x.reshape(1, -1), self.u, self.c, self.xi)
        valid = ok.sum().double().reshape(1)
        mean = torch.where(ok.unsqueeze(1), r, torch.zeros_like(r)).sum(0) / valid
        out = torch.where(ok.unsqueeze(1), r, torch.full_like(r, float("nan"))) if rows else None
        return TwScore(mean, valid, out, x)

    def _rows(self):
        """Columns [N, 1] in fp64 and the per-row invariants of the kernel's RowP."""
        P = self.pred.double()
        mu, sigma = P[:, 0:1], P[:, 1:2]
        atom = self.kind != _lib.LOSS_NORMAL
        tail = self.kind in (_lib.LOSS_MIXED, _lib.LOSS_MIXED_U)
        p = P[:, 2:3] if atom else torch.zeros_like(mu)
        su = P[:, 3:4] if tail else torch.ones_like(mu)
        u = P[:, 4:5] if self.kind == _lib.LOSS_MIXED_U else torch.full_like(mu, self.u)
        q = 1.0 - p
        r = dict(mu=mu, sigma=sigma, p=p, q=q, su=su, u=u, atom=atom, tail=tail)
        if atom:
            zc = (self.c - mu) / sigma
            r["Pc"], r["Sc"] = p + q * _lower_phi(zc), q * _upper_phi(zc)
        if tail:
            zu = (u - mu) / sigma
            r["mU"], r["omU"] = p + q * _lower_phi(zu), q * _upper_phi(zu)
        return r

    def _gpd_upper(self, r, x):
        t = torch.clamp((x - r["u"]) / r["su"], min=0.0)  # only read where x >= u
        return torch.pow(1.0 + self.xi * t, -1.0 / self.xi)

    def _prob_rows(self, r, x: torch.Tensor, upper: bool) -> torch.Tensor:
        """F or P(Y > .) at x [N, T] or [1, T]."""
        z = (x - r["mu"]) / r["sigma"]
        out = r["q"] * _upper_phi(z) if upper else r["p"] + r["q"] * _lower_phi(z)
        if r["tail"]:
            g = self._gpd_upper(r, x)
            t = r["omU"] * g if upper else r["mU"] + r["omU"] * (1.0 - g)
            out = torch.where(x >= r["u"], t, out)
        if r["atom"]:
            out = torch.where(x < self.c, torch.full_like(out, 1.0 if upper else 0.0), out)
        return out

    def _prob_cpu(self, x: torch.Tensor, upper: bool) -> torch.Tensor:
        return self._prob_rows(self._rows(), x.reshape(1, -1), upper)

    def _quantile_cpu(self, level: torch.Tensor, upper: bool) -> torch.Tensor:
        r = self._rows()
        N = self.pred.size(0)
        # one level vector for all rows, or [N, Q]: each row's own levels (ECC)
        lv = level if level.dim() == 2 else level.reshape(1, -1).expand(N, -1)
        inf = float("inf")
        s = lv if upper else 1.0 - lv
        v = s / r["q"]
        w = 1.0 - v if upper else (lv - r["p"]) / r["q"]
        high = (v <= 0.5) if upper else (w > 0.5)
        arg = torch.where(high, v, w)
        inside = (arg > 0) & (arg < 1)
        z = _upper_phi_inv(torch.where(inside, arg, torch.full_like(arg, 0.5)))
        x = torch.where(high, r["mu"] + r["sigma"] * z, r["mu"] - r["sigma"] * z)
        if r["atom"]:
            x = torch.clamp(x, min=self.c)
        if r["tail"]:
            x = torch.minimum(x, r["u"])
            in_tail = (lv < r["omU"]) if upper else (lv > r["mU"])
            ratio = torch.where(in_tail, s / r["omU"], torch.ones_like(s))
            xt = r["u"] + r["su"] / self.xi * (torch.pow(ratio, -self.xi) - 1.0)
            x = torch.where(in_tail, xt, x)
        if r["atom"]:
            at = (lv >= r["Sc"]) if upper else (lv <= r["Pc"])
            x = torch.where(at, torch.full_like(x, self.c), x)
        else:
            x = torch.where(lv == (1.0 if upper else 0.0), torch.full_like(x, -inf), x)
        x = torch.where(lv == (0.0 if upper else 1.0), torch.full_like(x, inf), x)
        bad = ~((lv >= 0.0) & (lv <= 1.0))
        return torch.where(bad, torch.full_like(x, float("nan")), x)

    def _crps_cpu(self, r, y: torch.Tensor) -> torch.Tensor:
        """Closed-form CRPS of y [N, 1] (fp64), as csrc/gine_forecast.hip restates it."""
        mu, sigma, p, q = r["mu"], r["sigma"], r["p"], r["q"]
        yt = (y - mu) / sigma
        if not r["atom"]:
            return sigma * (yt * (2.0 * _Phi(yt) - 1.0) + 2.0 * _phi(yt) - _INV_SQRT_PI)
        ct = (self.c - mu) / sigma
        Pc = p + q * _Phi(ct)
        t1 = yt * (2.0 * (p + q * _Phi(yt)) - 1.0)
        if not r["tail"]:
            t2 = -(ct * Pc * Pc)
            t3 = -2.0 * (q * _phi(ct) * Pc)
            t5 = -_INV_SQRT_PI * (q * q * (1.0 - _Phi(_SQRT2 * ct)))
            return sigma * (t1 + t2 + t3 + 2.0 * (q * _phi(yt)) + t5)
        u, su, xi = r["u"], r["su"], self.xi
        ut = (u - mu) / sigma
        m_u = p + q * _Phi(ut)
        Pu = q * (1.0 - _Phi(ut))
        t2 = ut * Pu * Pu - ct * Pc * Pc
        t3 = -2.0 * (q * _phi(ct) * Pc + q * _phi(ut) * Pu)
        t5 = -_INV_SQRT_PI * (q * q * (_Phi(_SQRT2 * ut) - _Phi(_SQRT2 * ct)))

        def pareto(yy):
            t = (yy - u) / su
            cdf = torch.where(t <= 0, torch.zeros_like(t),
                              1.0 - torch.pow(1.0 + xi * torch.clamp(t, min=0.0), -1.0 / xi))
            om = 1.0 - m_u
            return su * (torch.abs(t) - 2.0 / (1.0 - xi) * (om * (1.0 - torch.pow(1.0 - cdf,
                                                                                    1.0 - xi)))
                         + om * om / (2.0 - xi))

        loss1 = sigma * (t1 + t2 + t3 + 2.0 * (q * _phi(yt)) + t5) + pareto(u.expand_as(y))
        upper = sigma * (ut + t2 + t3 - 2.0 * (-(q * _phi(ut)) + ut * Pu) + t5)
        return torch.where(y < u, loss1, pareto(y) + upper)

    def _score_cpu(self, y: torch.Tensor, x: torch.Tensor) -> ForecastScore:
        r = self._rows()
        ok = ~torch.isnan(y)
        nan = torch.full((y.numel(),), float("nan"), dtype=torch.float64)
        y1 = torch.where(ok, y, torch.zeros_like(y)).double().unsqueeze(1)
        ye = torch.clamp(y1, min=self.c) if r["atom"] else y1
        crps = torch.where(ok, self._crps_cpu(r, y1).squeeze(1), nan)
        hi = self._prob_rows(r, ye, False).squeeze(1)
        lo = torch.where(ye.squeeze(1) == self.c, torch.zeros_like(hi), hi) if r["atom"] else hi
        sf = self._prob_rows(r, x.reshape(1, -1), True)               # [N, T]
        d = sf - (ye > x.reshape(1, -1)).double()
        valid = ok.sum().double().reshape(1)
        brier = torch.where(ok.unsqueeze(1), d * d, torch.zeros_like(d)).sum(0) / valid
        return ForecastScore(crps, torch.where(ok, lo, nan), torch.where(ok, hi, nan), brier,
                             valid)
