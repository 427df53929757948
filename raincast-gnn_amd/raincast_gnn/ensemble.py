"""The raw ensemble beside the predictive distribution: its scores, and members back out.

Every batch carries the NWP ensemble it post-processes (``batch.ensemble [N, E, F]``; the
precipitation column is one feature).  :class:`RawEnsemble` scores those members as they are
-- the baseline a post-processed CRPS is read against -- and :meth:`Forecast.ecc
<raincast_gnn.forecast.Forecast.ecc>` turns the distribution back into members that keep the
raw ensemble's rank structure (ensemble copula coupling, ECC-Q).

Definitions, per row, with ``x_i = shift + scale * members[n, i]`` in model space
``log(mm + 0.01)``, a NaN member missing and ``m`` the number of valid ones:

* stable rank ``r_i = 1 + #{j valid : x_j < x_i or (x_j == x_i and j < i)}`` (ties go to the
  lower member index: the same input gives the same members, run after run);
* ``crps = (1/m) sum |x_i - y| - (1/(2 m^2)) sum_ij |x_i - x_j|``, the pair term from the sorted
  values as ``(1/m^2) sum_k (2k - m - 1) x_(k)``; ``crps_fair`` with ``1/(2 m (m - 1))`` (NaN for
  ``m < 2``);
* ``rank_lo = #{x_i < y}``, ``rank_hi = #{x_i <= y}``: the observation's verification rank lies
  in ``rank_lo..rank_hi`` of ``0..m`` (the ensemble's ``pit_lo / pit_hi``);
* ``prob[n, t] = #{x_i > x_t} / m``, the ensemble's exceedance probability (no target needed);
* ECC-Q: member ``i`` becomes the predictive quantile at ``r_i / (m + 1)`` (``"uniform"``) or
  ``(r_i - 0.5) / m`` (``"midpoint"``); NaN where the member is missing.

Row scores are NaN for a NaN target or ``m = 0``; ``members_valid`` is ``m`` itself.

HIP tensors with at most 64 members go to ``gine_ensemble_score`` / ``gine_ensemble_ecc``
(csrc/gine_forecast.hip: one wavefront per row, one launch, the members read in place from the
strided view); CPU tensors, and HIP tensors with more members, go to the fp64 torch formulation
of the same definitions below (``torch.sort``), as :mod:`raincast_gnn.forecast` keeps one.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from .forecast import MM_OFFSET, Forecast

LEVELS = {"uniform": 0, "midpoint": _lib.ECC_MIDPOINT}


@dataclass
class EnsembleScore:
    """Verification of the raw ensemble: per row the CRPS, the fair CRPS, the verification
    rank interval and the valid member count; ``prob [N, T]`` the exceedance probabilities,
    ``brier [T]`` their Brier score over the valid rows and ``valid`` the number of those
    (a 1-element fp64 tensor; a row is valid with a target and at least one member)."""
    crps_rows: torch.Tensor
    crps_fair_rows: torch.Tensor
    rank_lo: torch.Tensor
    rank_hi: torch.Tensor
    members_valid: torch.Tensor
    prob: torch.Tensor
    brier: torch.Tensor
    valid: torch.Tensor

    @property
    def crps(self) -> torch.Tensor:
        """Mean CRPS over the valid rows (NaN when there is none)."""
        return torch.nansum(self.crps_rows) / self.valid[0]

    @property
    def crps_fair(self) -> torch.Tensor:
        """Mean fair CRPS over the valid rows with at least two members."""
        return torch.nansum(self.crps_fair_rows) / (~torch.isnan(self.crps_fair_rows)).sum()


@dataclass
class EnsembleTwScore:
    """Threshold-weighted CRPS of the raw ensemble: ``rows`` / ``fair_rows [N, T]`` (NaN where
    :class:`EnsembleScore` has NaN), their means ``mean`` / ``mean_fair [T]`` over the rows that
    have a value, ``valid`` the number of rows with a target and a member (a 1-element fp64
    tensor) and the ``thresholds [T]`` in model space."""
    rows: torch.Tensor
    fair_rows: torch.Tensor
    mean: torch.Tensor
    mean_fair: torch.Tensor
    valid: torch.Tensor
    thresholds: torch.Tensor


def skill(model_crps, ensemble_crps):
    """The CRPSS ``1 - model / ensemble``: positive where the model beats the ensemble."""
    return 1.0 - model_crps / ensemble_crps


def _thresholds(x, unit: str, device) -> torch.Tensor:
    """As ``Forecast._thresholds``: one-dimensional fp64, ``log(mm + 0.01)`` for ``unit="mm"``."""
    t = torch.as_tensor(x, dtype=torch.float64, device=device)
    if t.dim() > 1:
        raise ValueError("thresholds must be a scalar or one-dimensional")
    t = t.reshape(-1).contiguous()
    if unit == "mm":
        return torch.log(torch.clamp(t + MM_OFFSET, min=0.0))
    if unit != "model":
        raise ValueError(f"unit must be 'model' or 'mm', got {unit!r}")
    return t


class RawEnsemble:
    """The members ``[N, M]`` of each row's ensemble (any strides: nothing is copied), in
    model space after ``shift + scale * members``."""

    def __init__(self, members: torch.Tensor, *, scale: float = 1.0, shift: float = 0.0):
        if members.dim() != 2:
            raise ValueError(f"members must be [N, M], got {tuple(members.shape)}")
        if members.size(1) == 0:
            raise ValueError("an ensemble needs at least one member")
        members = members.detach()
        self.members = members if members.dtype == torch.float32 else members.float()
        self.scale, self.shift = float(scale), float(shift)

    @classmethod
    def from_batch(cls, ensemble: torch.Tensor, column: int, mean: float = 0.0,
                   std: float = 1.0) -> "RawEnsemble":
        """Column ``column`` of ``batch.ensemble [N, E, F]`` as a view, with the dataset's
        StandardScaler undone (``value = mean + std * stored``)."""
        if ensemble.dim() != 3:
            raise ValueError(f"ensemble must be [N, E, F], got {tuple(ensemble.shape)}")
        if not -ensemble.size(2) <= column < ensemble.size(2):
            raise ValueError(f"column {column} outside the {ensemble.size(2)} features")
        return cls(ensemble[:, :, column], scale=std, shift=mean)

    # ------------------------------------------------------------------ public
    @property
    def device(self):
        return self.members.device

    @property
    def on_kernel(self) -> bool:
        """Whether the HIP kernels take this ensemble (else the torch formulation)."""
        return self.members.is_cuda and self.members.size(1) <= _lib.ENSEMBLE_MAX_MEMBERS

    def values(self) -> torch.Tensor:
        """The members in model space, fp64 ``[N, M]``."""
        return self.shift + self.scale * self.members.double()

    def score(self, y: torch.Tensor, thresholds=(), unit: str = "model") -> EnsembleScore:
        """Scores of the targets ``y [N]`` (model space, NaN = missing); ``unit``: the
        thresholds'."""
        x = _thresholds(thresholds, unit, self.device)
        y = y.detach().to(self.device).float().reshape(-1).contiguous()
        N = self.members.size(0)
        if y.numel() != N:
            raise ValueError(f"y must have {N} entries, got {y.numel()}")
        rows, prob = self._score_hip(y, x) if self.on_kernel else self._score_torch(y, x)
        crps = rows[0]
        ok = ~torch.isnan(crps)
        valid = ok.sum().double().reshape(1)
        d = prob - (y.double().unsqueeze(1) > x.unsqueeze(0)).double()
        brier = torch.where(ok.unsqueeze(1), d * d, torch.zeros_like(d)).sum(0) / valid
        return EnsembleScore(crps, rows[1], rows[2], rows[3], rows[4], prob, brier, valid)

    def twcrps(self, y: torch.Tensor, thresholds, unit: str = "model") -> EnsembleTwScore:
        """Threshold-weighted CRPS of the targets ``y [N]`` at each threshold, weight
        ``1{x >= t}``: the ``crps`` / ``crps_fair`` formulas on ``max(x_i, t)`` and ``max(y, t)``
        (there is no censoring point here: the ensemble is whatever its members are).  Finite or
        ``-inf`` thresholds; NaN for a NaN threshold."""
        x = _thresholds(thresholds, unit, self.device)
        y = y.detach().to(self.device).float().reshape(-1).contiguous()
        N, T = self.members.size(0), x.numel()
        if y.numel() != N:
            raise ValueError(f"y must have {N} entries, got {y.numel()}")
        rows, fair = self._twcrps_hip(y, x) if self.on_kernel else self._twcrps_torch(y, x)
        ok = ~torch.isnan(y) & ((~torch.isnan(self.members)).sum(1) > 0)
        valid = ok.sum().double().reshape(1)
        mean = torch.where(ok.unsqueeze(1), rows, torch.zeros_like(rows)).sum(0) / valid
        has = ~torch.isnan(fair)
        mean_fair = torch.where(has, fair, torch.zeros_like(fair)).sum(0) / has.sum(0).double()
        mean_fair = torch.where(torch.isnan(x), torch.full_like(mean_fair, float("nan")),
                                mean_fair)
        return EnsembleTwScore(rows, fair, mean, mean_fair, valid, x)

    def exceedance(self, thresholds, unit: str = "model") -> torch.Tensor:
        """``#{x_i > threshold} / m`` per row and threshold (NaN for a row without members)."""
        x = _thresholds(thresholds, unit, self.device)
        if self.on_kernel:
            return self._launch_score(None, x, None)
        return self._score_torch(None, x)[1]

    def reliability(self, y: torch.Tensor, thresholds, unit: str = "model",
                    levels: int | None = None):
        """The ensemble's exceedance frequencies at ``thresholds`` beside the targets ``y [N]``
        as a :class:`raincast_gnn.reliability.Reliability`.  ``levels`` defaults to the number
        of members ``M``: without NaN members every frequency ``k / M`` is on that lattice
        exactly.  A row without members (NaN frequency) is invalid."""
        from .reliability import Reliability
        q = self.members.size(1) if levels is None else levels
        return Reliability(self.exceedance(thresholds, unit), y,
                           _thresholds(thresholds, unit, self.device), levels=q)

    def rank_histogram(self, score: EnsembleScore, generator=None) -> torch.Tensor:
        """Counts ``[M + 1]`` of the verification rank over the valid rows (Talagrand diagram).
        A target tied with members takes a rank drawn uniformly from ``rank_lo..rank_hi``, the
        analogue of :func:`raincast_gnn.forecast.pit_sample`."""
        M = self.members.size(1)
        lo, hi = score.rank_lo, score.rank_hi
        ok = ~torch.isnan(lo)
        u = torch.rand(lo.shape, dtype=torch.float64, device=lo.device, generator=generator)
        lo0, hi0 = torch.nan_to_num(lo), torch.nan_to_num(hi)
        rank = torch.minimum(lo0 + torch.floor(u * (hi0 - lo0 + 1.0)), hi0).long()
        return torch.bincount(rank, weights=ok.double(), minlength=M + 1).round().long()

    # ------------------------------------------------------------------ HIP
    def _launch_score(self, y, x: torch.Tensor, rows):
        mem = self.members
        N, M, T = mem.size(0), mem.size(1), x.numel()
        prob = torch.empty(N, T, dtype=torch.float64, device=mem.device)
        r = [None] * 5 if rows is None else [_lib.ptr(rows[k]) for k in range(5)]
        _lib.call("gine_ensemble_score", _lib.ptr(mem), mem.stride(0), mem.stride(1), M,
                  self.scale, self.shift, _lib.ptr(y), N, _lib.ptr(x), T, *r, _lib.ptr(prob),
                  _lib.stream_handle(mem.device))
        return prob

    def _score_hip(self, y: torch.Tensor, x: torch.Tensor):
        rows = torch.empty(5, self.members.size(0), dtype=torch.float64, device=self.device)
        return rows, self._launch_score(y, x, rows)

    def _twcrps_hip(self, y: torch.Tensor, x: torch.Tensor):
        mem = self.members
        N, T = mem.size(0), x.numel()
        out = torch.empty(2, N, T, dtype=torch.float64, device=self.device)
        _lib.call("gine_ensemble_twcrps", _lib.ptr(mem), mem.stride(0), mem.stride(1),
                  mem.size(1), self.scale, self.shift, _lib.ptr(y), N, _lib.ptr(x), T,
                  _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_handle(self.device))
        return out[0], out[1]

    # ------------------------------------------------------------------ torch (fp64)
    def _ranks(self):
        """-> values [N, M], sorted values (NaN last), stable ranks 1..M as int64 (those of
        missing members lie above m) and m [N]."""
        v = self.values()
        M = v.size(1)
        xs, idx = torch.sort(v, dim=1, stable=True)  # NaN sorts last
        k = torch.arange(1, M + 1, device=v.device).expand_as(idx)
        rank = torch.empty_like(idx).scatter_(1, idx, k)
        return v, xs, rank, (~torch.isnan(v)).sum(1)

    def _score_torch(self, y, x: torch.Tensor):
        v, xs, _, m = self._ranks()
        N, M = v.shape
        dm = m.double()
        nan = torch.full((N,), float("nan"), dtype=torch.float64, device=v.device)
        above = (v.unsqueeze(2) > x.reshape(1, 1, -1)).sum(1).double()  # NaN is never above
        prob = above / dm.unsqueeze(1)
        rows = torch.stack([nan, nan, nan, nan, dm])
        if y is None:
            return rows, prob
        yy = y.double().unsqueeze(1)
        ok = ~torch.isnan(y) & (m > 0)
        miss = torch.isnan(v)
        a = torch.where(miss, torch.zeros_like(v), (v - yy).abs()).sum(1)
        k = torch.arange(1, M + 1, device=v.device, dtype=torch.float64).unsqueeze(0)
        coef = 2.0 * k - dm.unsqueeze(1) - 1.0
        s = torch.where(torch.isnan(xs), torch.zeros_like(xs), coef * xs).sum(1)
        crps = a / dm - s / (dm * dm)
        fair = torch.where(m > 1, a / dm - s / (dm * (dm - 1.0)), nan)
        lo, hi = (v < yy).sum(1).double(), (v <= yy).sum(1).double()
        rows = torch.stack([torch.where(ok, crps, nan), torch.where(ok, fair, nan),
                            torch.where(ok, lo, nan), torch.where(ok, hi, nan), dm])
        return rows, prob

    def _twcrps_torch(self, y: torch.Tensor, x: torch.Tensor):
        v, xs, _, m = self._ranks()
        N, M = v.shape
        dm = m.double().unsqueeze(1)                                       # [N, 1]
        t = x.reshape(1, 1, -1)
        yc = torch.maximum(y.double().reshape(-1, 1, 1), t)                # [N, 1, T]
        miss = torch.isnan(v).unsqueeze(2)
        vc = torch.maximum(torch.nan_to_num(v).unsqueeze(2), t)           # [N, M, T]
        a = torch.where(miss, torch.zeros_like(vc), (vc - yc).abs()).sum(1)
        k = torch.arange(1, M + 1, device=v.device, dtype=torch.float64).reshape(1, -1, 1)
        coef = 2.0 * k - dm.unsqueeze(2) - 1.0
        xc = torch.maximum(torch.nan_to_num(xs).unsqueeze(2), t)          # sorted: NaN last
        s = torch.where(torch.isnan(xs).unsqueeze(2), torch.zeros_like(xc), coef * xc).sum(1)
        nan = torch.full_like(a, float("nan"))
        ok = (~torch.isnan(y) & (m > 0)).unsqueeze(1) & ~torch.isnan(x).unsqueeze(0)
        rows = torch.where(ok, a / dm - s / (dm * dm), nan)
        fair = torch.where(ok & (m > 1).unsqueeze(1), a / dm - s / (dm * (dm - 1.0)), nan)
        return rows, fair

    def _levels_torch(self, levels: str) -> torch.Tensor:
        """The ECC level of every member [N, M] (NaN where it is missing)."""
        v, _, rank, m = self._ranks()
        r, dm = rank.double(), m.double().unsqueeze(1)
        lv = (r - 0.5) / dm if LEVELS[levels] else r / (dm + 1.0)
        return torch.where(torch.isnan(v), torch.full_like(lv, float("nan")), lv)


def ecc(forecast: Forecast, raw: RawEnsemble, levels: str = "uniform") -> torch.Tensor:
    """ECC-Q members ``[N, M]`` in model space (``Forecast.ecc`` is the public entry)."""
    if levels not in LEVELS:
        raise ValueError(f"levels must be 'uniform' or 'midpoint', got {levels!r}")
    pred, mem = forecast.pred, raw.members
    if mem.size(0) != pred.size(0):
        raise ValueError(f"the ensemble has {mem.size(0)} rows, the forecast {pred.size(0)}")
    if mem.device != pred.device:
        raise ValueError(f"the ensemble is on {mem.device}, the forecast on {pred.device}")
    if not raw.on_kernel:  # each row's own levels through the torch formulation
        return forecast._quantile_cpu(raw._levels_torch(levels), False)
    N, M = mem.shape
    out = torch.empty(N, M, dtype=torch.float64, device=pred.device)
    _lib.call("gine_ensemble_ecc", _lib.ptr(pred), N, forecast.kind, forecast.u, forecast.xi,
              forecast.c, _lib.ptr(mem), mem.stride(0), mem.stride(1), M, raw.scale, raw.shift,
              LEVELS[levels], _lib.ptr(out), _lib.stream_handle(pred.device))
    return out
