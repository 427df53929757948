"""Paired score comparison: is A better than B, or is the difference noise?  

Two sets of per-row scores over the same ``[T days, S stations]`` grid -- a model's CRPS rows
beside the raw ensemble's, or run A beside run B -- give skill and mean difference, overall and
per station, with moving-block bootstrap intervals and Diebold-Mariano tests under a
false-discovery correction over the stations.

Definitions (the contract; include/gine_hip.h states the same):

* ``a`` and ``b`` are fp64 grids read in place through their strides; a pair is **valid** when
  both elements are non-NaN.  An optional weight ``w`` (finite, >= 0) is only summed, it never
  multiplies ``a`` or ``b``: day sums are resampled together with their valid counts that way.
* Generator, counter-based, all arithmetic mod 2^64 (no state, no stored indices)::

      mix(seed, i): z = seed + (i + 1) * 0x9E3779B97F4A7C15
                    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
                    z = (z ^ (z >> 27)) * 0x94D049BB133111EB
                    return z ^ (z >> 31)
      nb = ceil(T / L)                          blocks per replicate, 1 <= L <= T
      start(r, j) = ((mix(seed, r * nb + j) >> 32) * T) >> 32     r = global replicate index
      draws of replicate r: for j = 0 .. nb-1, for i = 0 .. L-1: day (start(r, j) + i) mod T,
                            cut off after T draws

  the circular moving-block bootstrap (``L = 1``: the ordinary one).  The multiply-shift is
  biased: a day's probability differs from ``1/T`` by at most ``2^-32``, a relative ``T / 2^32``.
  All stations of a replicate see the same days, so spatial dependence is kept and the
  per-station sums add up to the overall ones.
* Replicate sums: walking the draws in order, every valid pair does ``A += a``, ``B += b``,
  ``W += w`` (or 1), one fp64 add each from 0; ``diff = (A - B) / W``, ``skill = 1 - A / B``;
  IEEE results stand (``W = 0`` gives NaN).
* Marginal sums: per station over the days ascending, sequentially; per day over its stations
  in a fixed order (64 strided partial sums folded in halves; not part of the contract).  The
  overall sums are those of the day sums, days ascending.
* Diebold-Mariano per column: ``d_t = a - b`` at valid ``t``, ``n`` valid days,
  ``dbar = (sum d_t) / n``, ``g_k = (sum_{t, t+k both valid} (d_t - dbar)(d_{t+k} - dbar)) / n``
  for ``k = 0 .. h``, ``v = g_0 + sum_k 2 (1 - k / (h + 1)) g_k`` (Bartlett), ``var = v / n``,
  ``stat = dbar / sqrt(var)``, ``p = erfc(|stat| / sqrt(2))``; ``n < 2``, ``var <= 0`` or a
  non-finite ``var`` give NaN for ``stat`` and ``p``.

fp64 HIP tensors go to ``gine_compare_reduce`` / ``_bootstrap`` / ``_dm`` (csrc/
gine_compare.hip) on the current stream, without host synchronisation.  CPU tensors, non-fp64
inputs and ``lags > 64`` take the numpy fp64 formulation of the same definitions below: the same
generator and the same sequential sums, so CPU and device agree to the bit wherever the contract
fixes the order (and here also for the day sums, which follow the kernel's order).

Command line::

    python -m raincast_gnn.compare --a RUN_A --b RUN_B --data rf --stations S
        [--replicates 10000 --block-len 7 --lags 3 --fdr 0.05 --seed 0]

reads each run's ``params.json`` and ``results/<data>.csv`` (``tp6``, ``pred_0..``), scores both
with :class:`raincast_gnn.forecast.Forecast`, and writes ``RUN_A/results/compare_<data>.csv``.
"""
from __future__ import annotations

import argparse
import csv
import logging
import math
import os
import sys
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

log = logging.getLogger("raincast_gnn.compare")

MAX_LAGS = _lib.COMPARE_MAX_LAGS
_QUANTILE_ELEMENTS = 1 << 24  # torch.quantile's input limit


@dataclass
class BootstrapResult:
    """What :meth:`PairedScores.bootstrap` returns.  ``diff`` and ``skill`` are the overall
    replicate vectors ``[R]``; ``*_ci`` are ``[2]`` (lower, upper) percentile intervals,
    ``station_*_ci`` ``[2, S]``; ``*_se`` the bootstrap standard error of ``diff``;
    ``significant [S]``: the station's interval of ``diff`` excludes 0.  The station fields are
    None with ``per_station=False``."""
    diff: torch.Tensor
    skill: torch.Tensor
    diff_ci: torch.Tensor
    skill_ci: torch.Tensor
    diff_se: torch.Tensor
    station_diff_ci: torch.Tensor | None
    station_skill_ci: torch.Tensor | None
    station_diff_se: torch.Tensor | None
    significant: torch.Tensor | None
    replicates: int
    block_len: int
    seed: int
    level: float


@dataclass
class DMResult:
    """What :meth:`PairedScores.dm_test` returns: the overall test on the day series (0-dim
    tensors) and, per station ``[S]``, the statistic, its two-sided p-value and ``rejected``,
    Benjamini-Hochberg at ``fdr`` over the stations with a finite p-value."""
    n: torch.Tensor
    mean_d: torch.Tensor
    var: torch.Tensor
    stat: torch.Tensor
    pvalue: torch.Tensor
    station_n: torch.Tensor | None
    station_mean_d: torch.Tensor | None
    station_var: torch.Tensor | None
    station_stat: torch.Tensor | None
    station_pvalue: torch.Tensor | None
    rejected: torch.Tensor | None
    lags: int
    fdr: float


@dataclass
class Comparison:
    """What :func:`compare` returns for one pair of columns."""
    scores: "PairedScores"
    bootstrap: BootstrapResult
    dm: DMResult


# ---------------------------------------------------------------------------------- numpy (fp64)
def _np_mix(seed: int, i: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def block_starts(seed: int, rep_first: int, replicates: int, num_days: int,
                 block_len: int) -> np.ndarray:
    """``start(r, j)`` for ``r = rep_first .. rep_first + replicates - 1``, ``[R, nb]`` int64."""
    nb = -(-num_days // block_len)
    with np.errstate(over="ignore"):
        r = np.uint64(rep_first & 0xFFFFFFFFFFFFFFFF) + np.arange(replicates, dtype=np.uint64)
        i = r[:, None] * np.uint64(nb) + np.arange(nb, dtype=np.uint64)[None, :]
    hi = _np_mix(seed, i) >> np.uint64(32)
    return ((hi * np.uint64(num_days)) >> np.uint64(32)).astype(np.int64)


def _np_reduce(a: np.ndarray, b: np.ndarray):
    """-> (day_a, day_b, day_n, station_a, station_b, station_n) in the kernel's orders."""
    T, S = a.shape
    ok = ~np.isnan(a) & ~np.isnan(b)
    va, vb, vn = np.where(ok, a, 0.0), np.where(ok, b, 0.0), ok.astype(np.float64)
    stations = []
    for v in (va, vb, vn):
        acc = np.zeros(S)
        for t in range(T):
            acc = acc + v[t]
        stations.append(acc)
    days = []
    chunks = -(-S // 64)
    for v in (va, vb, vn):
        pad = np.zeros((T, chunks * 64))
        pad[:, :S] = v
        pad = pad.reshape(T, chunks, 64)
        acc = np.zeros((T, 64))
        for c in range(chunks):  # lane l: stations l, l + 64, ... ascending
            acc = acc + pad[:, c]
        width = 32
        while width >= 1:  # the 64 lane sums fold in halves
            acc = acc[:, :width] + acc[:, width:2 * width]
            width //= 2
        days.append(acc[:, 0])
    return (*days, *stations)


def _np_bootstrap(a, b, w, block_len: int, seed: int, rep_first: int, replicates: int):
    """-> (A, B, W), each ``[R, S]``: the replicate sums, draw by draw."""
    T, S = a.shape
    ok = ~np.isnan(a) & ~np.isnan(b)
    va, vb = np.where(ok, a, 0.0), np.where(ok, b, 0.0)
    vw = ok.astype(np.float64) if w is None else np.where(ok, w, 0.0)
    A = np.zeros((replicates, S))
    B = np.zeros((replicates, S))
    W = np.zeros((replicates, S))
    step = max(1, (1 << 22) // S)
    for r0 in range(0, replicates, step):
        r1 = min(replicates, r0 + step)
        starts = block_starts(seed, rep_first + r0, r1 - r0, T, block_len)
        for d in range(T):
            day = (starts[:, d // block_len] + d % block_len) % T
            A[r0:r1] += va[day]
            B[r0:r1] += vb[day]
            W[r0:r1] += vw[day]
    return A, B, W


def _np_dm(a: np.ndarray, b: np.ndarray, lags: int):
    """-> (n, dbar, var, stat, p), each ``[S]``."""
    T, S = a.shape
    ok = ~np.isnan(a) & ~np.isnan(b)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = a - b
        total, n = np.zeros(S), np.zeros(S)
        for t in range(T):
            total = total + np.where(ok[t], d[t], 0.0)
            n = n + ok[t]
        dbar = total / n
        c = d - dbar
        v = None
        for k in range(lags + 1):
            g = np.zeros(S)
            for t in range(T - k):
                g = g + np.where(ok[t] & ok[t + k], c[t] * c[t + k], 0.0)
            g = g / n
            v = g if k == 0 else v + 2.0 * (1.0 - k / (lags + 1.0)) * g
        var = v / n
        good = (n >= 2.0) & (var > 0.0) & np.isfinite(var)
        stat = np.where(good, dbar / np.sqrt(np.where(good, var, 1.0)), np.nan)
        p = np.array([math.erfc(abs(x) * 0.70710678118654752440) if x == x else math.nan
                      for x in stat])
    return n, dbar, var, stat, p


# ---------------------------------------------------------------------------------- helpers
def _as_grid(x: torch.Tensor, num_stations, what: str) -> torch.Tensor:
    x = x.detach()
    if x.dim() == 2:
        if num_stations is not None and x.size(1) != num_stations:
            raise ValueError(f"{what} has {x.size(1)} stations, num_stations={num_stations}")
        return x
    if x.dim() != 1:
        raise ValueError(f"{what} must be [T, S] or [T * S], got {tuple(x.shape)}")
    if num_stations is None or num_stations < 1:
        raise ValueError(f"{what} is one-dimensional: num_stations is needed")
    if x.numel() % num_stations:
        raise ValueError(f"{what} has {x.numel()} rows, not a multiple of {num_stations} stations")
    step = x.stride(0)
    return x.as_strided((x.numel() // num_stations, num_stations), (num_stations * step, step))


def _grid_args(x: torch.Tensor):
    return _lib.ptr(x), x.stride(0), x.stride(1)


def _column(v: torch.Tensor) -> torch.Tensor:
    return v.reshape(-1, 1)


def percentile_interval(x: torch.Tensor, level: float) -> torch.Tensor:
    """``[2, ...]``: ``torch.nanquantile`` over dim 0 at ``(1 - level) / 2`` and its mirror."""
    lo = (1.0 - level) / 2.0
    q = torch.tensor([lo, 1.0 - lo], dtype=torch.float64, device=x.device)
    return torch.nanquantile(x, q, dim=0)


def nan_std(x: torch.Tensor) -> torch.Tensor:
    """Standard deviation over dim 0 of the non-NaN entries (n - 1 in the denominator)."""
    ok = ~torch.isnan(x)
    n = ok.sum(0).double()
    zero = torch.zeros_like(x)
    mean = torch.where(ok, x, zero).sum(0) / n
    dev = torch.where(ok, x - mean, zero)
    return torch.sqrt((dev * dev).sum(0) / (n - 1.0).clamp_min(0.0))  # 0 / 0 below two values


def benjamini_hochberg(p: torch.Tensor, fdr: float) -> torch.Tensor:
    """Which of ``p [S]`` are rejected at false-discovery rate ``fdr``, over the entries with a
    finite p-value (the others are never rejected).  On the tensor's device, no
    synchronisation."""
    finite = torch.isfinite(p)
    m = finite.sum().double()
    ordered, order = torch.sort(torch.where(finite, p, torch.full_like(p, float("inf"))))
    rank = torch.arange(1, p.numel() + 1, dtype=torch.float64, device=p.device)
    passing = ordered <= rank * fdr / m
    last = torch.where(passing, rank, torch.zeros_like(rank)).max()  # 0: none passes
    out = torch.zeros_like(finite)
    out[order] = rank <= last
    return out & finite


SUM_FIELDS = ("sum_a", "sum_b", "sum_w", "diff", "skill")
DM_FIELDS = ("n", "mean_d", "var", "stat", "pvalue")


def _on_kernel(*grids) -> bool:
    return all(g.is_cuda and g.dtype == torch.float64 for g in grids if g is not None)


def _host(x: torch.Tensor) -> np.ndarray:
    return x.detach().double().cpu().numpy()


def _back(v: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(device)


def marginal_sums(a: torch.Tensor, b: torch.Tensor, days: bool = True,
                  stations: bool = True) -> dict:
    """The marginal sums of the valid pairs of two ``[T, S]`` grids: ``day_a``, ``day_b``,
    ``day_n`` ``[T]`` and ``station_a``, ``station_b``, ``station_n`` ``[S]``, fp64."""
    T, S = a.shape
    names = ("day_a", "day_b", "day_n") * days + ("station_a", "station_b", "station_n") * stations
    if not _on_kernel(a, b):
        full = dict(zip(("day_a", "day_b", "day_n", "station_a", "station_b", "station_n"),
                        _np_reduce(_host(a), _host(b))))
        return {k: _back(full[k], a.device) for k in names}
    d = list(torch.empty(3, T, dtype=torch.float64, device=a.device)) if days else [None] * 3
    s = list(torch.empty(3, S, dtype=torch.float64, device=a.device)) if stations else [None] * 3
    _lib.call("gine_compare_reduce", *_grid_args(a), *_grid_args(b), T, S,
              *[_lib.ptr(o) for o in d + s], _lib.stream_handle(a.device))
    return {k: v for k, v in zip(("day_a", "day_b", "day_n", "station_a", "station_b",
                                  "station_n"), d + s) if v is not None}


def replicate_sums(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor | None = None, *,
                   block_len: int, seed: int = 0, rep_first: int = 0, replicates: int,
                   fields=SUM_FIELDS, out: dict | None = None) -> dict:
    """Replicates ``rep_first .. rep_first + replicates - 1`` of the ``[T, S]`` grids: those of
    ``sum_a``, ``sum_b``, ``sum_w``, ``diff``, ``skill`` named in ``fields``, ``[R, S]`` fp64
    each; ``out``: contiguous tensors to write into, by name, instead."""
    T, S = a.shape
    R = int(replicates)
    if out is None:
        out = {k: torch.empty(R, S, dtype=torch.float64, device=a.device) for k in fields}
    if any(o.shape != (R, S) or not o.is_contiguous() or o.dtype != torch.float64
           for o in out.values()):
        raise ValueError(f"outputs must be contiguous fp64 [{R}, {S}]")
    if not _on_kernel(a, b, w):
        if not 1 <= block_len <= T:
            raise ValueError(f"block_len must be in 1..{T}, got {block_len}")
        A, B, W = _np_bootstrap(_host(a), _host(b), None if w is None else _host(w), block_len,
                                seed, rep_first, R)
        with np.errstate(invalid="ignore", divide="ignore"):
            full = {"sum_a": A, "sum_b": B, "sum_w": W, "diff": (A - B) / W,
                    "skill": 1.0 - A / B}
        for k, o in out.items():
            o.copy_(_back(full[k], a.device))
        return out
    wargs = (None, 0, 0) if w is None else _grid_args(w)
    _lib.call("gine_compare_bootstrap", *_grid_args(a), *_grid_args(b), *wargs, T, S, block_len,
              seed & 0xFFFFFFFFFFFFFFFF, rep_first, R, *[_lib.ptr(out.get(k)) for k in SUM_FIELDS],
              _lib.stream_handle(a.device))
    return out


def dm_columns(a: torch.Tensor, b: torch.Tensor, lags: int) -> dict:
    """Diebold-Mariano per column of the ``[T, S]`` grids: ``n``, ``mean_d``, ``var``, ``stat``,
    ``pvalue``, ``[S]`` fp64 each."""
    T, S = a.shape
    if not 0 <= lags < T:
        raise ValueError(f"lags must be in 0..{T - 1}, got {lags}")
    if not _on_kernel(a, b) or lags > MAX_LAGS:
        return {k: _back(v, a.device) for k, v in zip(DM_FIELDS, _np_dm(_host(a), _host(b), lags))}
    out = list(torch.empty(5, S, dtype=torch.float64, device=a.device))
    _lib.call("gine_compare_dm", *_grid_args(a), *_grid_args(b), T, S, lags,
              *[_lib.ptr(o) for o in out], _lib.stream_handle(a.device))
    return dict(zip(DM_FIELDS, out))


class PairedScores:
    """Two score grids over the same days and stations.

    ``a`` and ``b`` are ``[T, S]``, or ``[T * S]`` with ``num_stations``, on the same device.
    Rows are in collated order -- day-major, the stations of a day in the dataset's order --
    which is what :func:`raincast_gnn.evaluate.predict_model` and
    :func:`raincast_gnn.data.restore_node_order` return, and so the order of the rows of
    ``Forecast.score``, ``RawEnsemble.score`` and the twCRPS entries computed from them.
    Nothing is copied: a column ``rows[:, k]`` of a ``[T * S, K]`` result is read in place.
    NaN = missing; lower scores are better, so ``diff < 0`` and ``skill > 0`` favour ``a``."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor, num_stations: int | None = None):
        self.a = _as_grid(a, num_stations, "a")
        self.b = _as_grid(b, num_stations, "b")
        if self.a.shape != self.b.shape:
            raise ValueError(f"a is {tuple(self.a.shape)}, b is {tuple(self.b.shape)}")
        if self.a.device != self.b.device:
            raise ValueError(f"a is on {self.a.device}, b on {self.b.device}")
        if self.a.size(0) < 1 or self.a.size(1) < 1:
            raise ValueError("at least one day and one station are needed")
        if self.a.size(0) >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 days")
        self._sums = None

    # ------------------------------------------------------------------ layout
    @property
    def device(self):
        return self.a.device

    @property
    def num_days(self) -> int:
        return self.a.size(0)

    @property
    def num_stations(self) -> int:
        return self.a.size(1)

    @property
    def on_kernel(self) -> bool:
        """Whether the HIP kernels take these grids (else the numpy formulation)."""
        return _on_kernel(self.a, self.b)

    def _empty(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    def _reduce(self, a, b, days: bool, stations: bool):
        m = marginal_sums(a, b, days=days, stations=stations)
        return ([m.get(k) for k in ("day_a", "day_b", "day_n")],
                [m.get(k) for k in ("station_a", "station_b", "station_n")])

    def _bootstrap(self, a, b, w, block_len, seed, rep_first, diff, skill):
        replicate_sums(a, b, w, block_len=block_len, seed=seed, rep_first=rep_first,
                       replicates=diff.size(0), out={"diff": diff, "skill": skill})

    def _dm(self, a, b, lags: int):
        r = dm_columns(a, b, lags)
        return [r[k] for k in DM_FIELDS]

    # ------------------------------------------------------------------ point estimates
    def _marginals(self):
        if self._sums is None:
            (da, db, dn), (sa, sb, sn) = self._reduce(self.a, self.b, True, True)
            # the overall sums: the day sums added days ascending (they are never NaN)
            _, (A, B, _) = self._reduce(_column(da), _column(db), False, True)
            _, (N, _, _) = self._reduce(_column(dn), _column(dn), False, True)
            self._sums = SimpleNamespace(day_a=da, day_b=db, day_n=dn, station_a=sa,
                                         station_b=sb, station_n=sn, a=A[0], b=B[0], n=N[0])
        return self._sums

    @property
    def day_sums(self):
        """``(day_a, day_b, day_n)``, each ``[T]``."""
        m = self._marginals()
        return m.day_a, m.day_b, m.day_n

    @property
    def station_sums(self):
        """``(station_a, station_b, station_n)``, each ``[S]``."""
        m = self._marginals()
        return m.station_a, m.station_b, m.station_n

    @property
    def valid(self) -> torch.Tensor:
        return self._marginals().n

    @property
    def mean_a(self) -> torch.Tensor:
        m = self._marginals()
        return m.a / m.n

    @property
    def mean_b(self) -> torch.Tensor:
        m = self._marginals()
        return m.b / m.n

    @property
    def diff(self) -> torch.Tensor:
        m = self._marginals()
        return (m.a - m.b) / m.n

    @property
    def skill(self) -> torch.Tensor:
        m = self._marginals()
        return 1.0 - m.a / m.b

    @property
    def station_valid(self) -> torch.Tensor:
        return self._marginals().station_n

    @property
    def station_mean_a(self) -> torch.Tensor:
        m = self._marginals()
        return m.station_a / m.station_n

    @property
    def station_mean_b(self) -> torch.Tensor:
        m = self._marginals()
        return m.station_b / m.station_n

    @property
    def station_diff(self) -> torch.Tensor:
        m = self._marginals()
        return (m.station_a - m.station_b) / m.station_n

    @property
    def station_skill(self) -> torch.Tensor:
        m = self._marginals()
        return 1.0 - m.station_a / m.station_b

    # ------------------------------------------------------------------ bootstrap
    def bootstrap(self, replicates: int = 1000, block_len: int = 1, seed: int = 0,
                  level: float = 0.95, per_station: bool = True,
                  max_bytes: int = 256 << 20) -> BootstrapResult:
        """Circular moving-block bootstrap of ``diff`` and ``skill``.  Overall: the day sums
        with their valid counts, resampled as one weighted column.  Per station: the grid
        itself, cut into chunks of stations and of replicates so that no ``[R, S]`` buffer a
        kernel writes exceeds ``max_bytes`` (the chunks give the same bits: row ``i`` of a call
        is replicate ``rep_first + i`` and all stations of a replicate see the same days)."""
        T, S, R = self.num_days, self.num_stations, int(replicates)
        if R < 1:
            raise ValueError(f"replicates must be at least 1, got {replicates}")
        if not 1 <= block_len <= T:
            raise ValueError(f"block_len must be in 1..{T}, got {block_len}")
        if not 0.0 < level < 1.0:
            raise ValueError(f"level must be in (0, 1), got {level}")
        m = self._marginals()
        diff, skill = self._empty(R, 1), self._empty(R, 1)
        self._bootstrap(_column(m.day_a), _column(m.day_b), _column(m.day_n), block_len, seed, 0,
                        diff, skill)
        diff, skill = diff[:, 0], skill[:, 0]
        res = BootstrapResult(diff, skill, percentile_interval(diff, level),
                              percentile_interval(skill, level), nan_std(diff), None, None, None,
                              None, R, int(block_len), int(seed), float(level))
        if not per_station:
            return res
        cells = max(1, int(max_bytes) // 8)
        s_chunk = min(S, max(1, min(cells, _QUANTILE_ELEMENTS) // R))
        r_chunk = min(R, max(1, cells // s_chunk))
        d_ci, s_ci, d_se = self._empty(2, S), self._empty(2, S), self._empty(S)
        for s0 in range(0, S, s_chunk):
            s1 = min(S, s0 + s_chunk)
            a, b = self.a[:, s0:s1], self.b[:, s0:s1]
            d_all, k_all = self._empty(R, s1 - s0), self._empty(R, s1 - s0)
            if r_chunk == R:
                self._bootstrap(a, b, None, block_len, seed, 0, d_all, k_all)
            else:
                d_part, k_part = self._empty(r_chunk, s1 - s0), self._empty(r_chunk, s1 - s0)
                for r0 in range(0, R, r_chunk):
                    n = min(r_chunk, R - r0)
                    self._bootstrap(a, b, None, block_len, seed, r0, d_part[:n], k_part[:n])
                    d_all[r0:r0 + n] = d_part[:n]
                    k_all[r0:r0 + n] = k_part[:n]
            d_ci[:, s0:s1] = percentile_interval(d_all, level)
            s_ci[:, s0:s1] = percentile_interval(k_all, level)
            d_se[s0:s1] = nan_std(d_all)
        res.station_diff_ci, res.station_skill_ci, res.station_diff_se = d_ci, s_ci, d_se
        res.significant = (d_ci[0] > 0.0) | (d_ci[1] < 0.0)
        return res

    # ------------------------------------------------------------------ Diebold-Mariano
    def dm_test(self, lags: int = 0, per_station: bool = True, fdr: float = 0.05) -> DMResult:
        """Diebold-Mariano tests of equal mean score with ``lags`` autocovariances under
        Bartlett weights.  Overall: on the day series ``day_a / day_n - day_b / day_n`` (NaN
        for a day without a valid pair).  Per station: statistic, two-sided p-value and
        ``rejected``, Benjamini-Hochberg at ``fdr`` over the stations with a finite p-value."""
        T = self.num_days
        if not 0 <= lags < T:
            raise ValueError(f"lags must be in 0..{T - 1}, got {lags}")
        if not 0.0 < fdr < 1.0:
            raise ValueError(f"fdr must be in (0, 1), got {fdr}")
        m = self._marginals()
        n, mean_d, var, stat, p = (v[0] for v in self._dm(_column(m.day_a / m.day_n),
                                                          _column(m.day_b / m.day_n), lags))
        res = DMResult(n, mean_d, var, stat, p, None, None, None, None, None, None, int(lags),
                       float(fdr))
        if per_station:
            (res.station_n, res.station_mean_d, res.station_var, res.station_stat,
             res.station_pvalue) = self._dm(self.a, self.b, lags)
            res.rejected = benjamini_hochberg(res.station_pvalue, fdr)
        return res


def compare(model_rows: torch.Tensor, other_rows: torch.Tensor, num_stations: int, *,
            replicates: int = 1000, block_len: int = 1, seed: int = 0, level: float = 0.95,
            lags: int = 0, fdr: float = 0.05, per_station: bool = True,
            max_bytes: int = 256 << 20):
    """Per-row scores of a model beside another's over the same rows (``[N]``, ``N = T * S`` in
    collated order) -> a :class:`Comparison`: the :class:`PairedScores`, their bootstrap and
    their Diebold-Mariano tests.  ``[N, K]`` rows (the twCRPS rows of ``K`` thresholds) give a
    list of ``K`` comparisons, each column read in place."""
    if model_rows.shape != other_rows.shape or model_rows.dim() not in (1, 2):
        raise ValueError(f"rows must both be [N] or [N, K], got {tuple(model_rows.shape)} and "
                         f"{tuple(other_rows.shape)}")

    def one(a, b):
        ps = PairedScores(a, b, num_stations)
        return Comparison(ps, ps.bootstrap(replicates, block_len, seed, level, per_station,
                                           max_bytes),
                          ps.dm_test(lags, per_station, fdr))

    other_rows = other_rows.to(model_rows.device)
    if model_rows.dim() == 1:
        return one(model_rows, other_rows)
    return [one(model_rows[:, k], other_rows[:, k]) for k in range(model_rows.size(1))]


# ---------------------------------------------------------------------------------- command line
def _read_run(run: str, data: str, device):
    """-> (targets [N] fp32, CRPS rows [N] fp64) of ``run/results/<data>.csv``."""
    from .forecast import Forecast
    from .params import load_params
    config = load_params(os.path.join(run, "params.json"))
    path = os.path.join(run, "results", f"{data}.csv")
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = next(reader)
        rows = [[float(v) if v != "" else math.nan for v in row] for row in reader if row]
    if not header or header[0] != "tp6" or any(h != f"pred_{i}" for i, h in
                                               enumerate(header[1:])):
        raise ValueError(f"{path}: expected the columns tp6, pred_0, pred_1, ...; got {header}")
    table = torch.tensor(rows, dtype=torch.float64).reshape(len(rows), len(header))
    y = table[:, 0].float().to(device)
    model = SimpleNamespace(loss=config["loss"], grad_u=config.get("grad_u", "False"),
                            u=config.get("u"), xi=config.get("xi"))
    score = Forecast.from_model(model, table[:, 1:].float().to(device)).score(y)
    return y, score.crps_rows.double()


def main(argv=None) -> Comparison:
    ap = argparse.ArgumentParser(description="Compare two runs' CRPS: skill, block-bootstrap "
                                             "intervals and Diebold-Mariano tests per station.")
    ap.add_argument("--a", required=True, help="run directory A (params.json, results/)")
    ap.add_argument("--b", required=True, help="run directory B")
    ap.add_argument("--data", required=True, help="results/<data>.csv of both runs")
    ap.add_argument("--stations", type=int, required=True, help="stations per day")
    ap.add_argument("--replicates", type=int, default=10000)
    ap.add_argument("--block-len", type=int, default=7)
    ap.add_argument("--lags", type=int, default=3)
    ap.add_argument("--fdr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is one")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s",
                        handlers=[logging.StreamHandler(sys.stdout)])
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    ya, rows_a = _read_run(args.a, args.data, device)
    yb, rows_b = _read_run(args.b, args.data, device)
    if ya.shape != yb.shape or not bool(((ya == yb) | (torch.isnan(ya) & torch.isnan(yb))).all()):
        raise SystemExit(f"the targets (tp6) of {args.a} and {args.b} differ: not the same rows")
    res = compare(rows_a, rows_b, args.stations, replicates=args.replicates,
                  block_len=args.block_len, seed=args.seed, level=args.level, lags=args.lags,
                  fdr=args.fdr)
    ps, bs, dm = res.scores, res.bootstrap, res.dm
    log.info("%s vs %s on %s: mean %.6f vs %.6f over %d pairs, diff %.6f [%.6f, %.6f], skill "
             "%.4f [%.4f, %.4f] (%d replicates, blocks of %d, level %.2f); DM stat %.3f p %.3g "
             "(%d lags); %d of %d stations significant, %d rejected at FDR %.2f",
             args.a, args.b, args.data, float(ps.mean_a), float(ps.mean_b), int(ps.valid),
             float(ps.diff), *bs.diff_ci.tolist(), float(ps.skill), *bs.skill_ci.tolist(),
             bs.replicates, bs.block_len, bs.level, float(dm.stat), float(dm.pvalue), dm.lags,
             int(bs.significant.sum()), ps.num_stations, int(dm.rejected.sum()), dm.fdr)
    columns = {
        "valid": ps.station_valid, "mean_a": ps.station_mean_a, "mean_b": ps.station_mean_b,
        "diff": ps.station_diff, "diff_lo": bs.station_diff_ci[0],
        "diff_hi": bs.station_diff_ci[1], "diff_se": bs.station_diff_se,
        "skill": ps.station_skill, "skill_lo": bs.station_skill_ci[0],
        "skill_hi": bs.station_skill_ci[1], "significant": bs.significant.double(),
        "dm_stat": dm.station_stat, "dm_p": dm.station_pvalue, "dm_rejected": dm.rejected.double()}
    host = {k: v.cpu().tolist() for k, v in columns.items()}
    out_dir = os.path.join(args.a, "results")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"compare_{args.data}.csv")
    with open(path, "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(["station", *host])
        for s in range(ps.num_stations):
            writer.writerow([s] + [int(host[k][s]) if k in ("valid", "significant", "dm_rejected")
                                   else repr(host[k][s]) for k in host])
    log.info("wrote %s", path)
    return res


if __name__ == "__main__":
    main()
