"""Reliability diagrams: when the forecast says 30 %, does it happen 30 % of the time?


The probabilities ``p [N, T]`` of the events "``y`` exceeds threshold ``x_t``" are held against
the outcomes by the CORP method (Dimitriadis, Gneiting and Jordan, PNAS 2021): the reliability
curve is the isotonic (pool-adjacent-violators) regression of the event on the forecast
probability, the Brier score splits into ``MCB - DSC + UNC`` with the calibrated probabilities,
and consistency bands and a Monte-Carlo test of "the forecast is reliable" come from
resampling the outcomes under the forecast's own probabilities (Broecker and Smith 2007).

Definitions (the contract; include/gine_hip.h states the same).  Everything runs on a
probability lattice of ``q`` steps, levels ``k = 0 .. q``, ``K = q + 1``, ``1 <= q <= 4096``:

* Cell ``(i, t)`` is **valid** when ``y_i`` and ``x_t`` are not NaN and ``0 <= p <= 1`` (NaN and
  out-of-range ``p`` are invalid, not an error).  Its event is ``(double)y_i > x_t``, its level
  ``k = (int)rint(p * q)`` (one fp64 multiply, round half to even), the level's value
  ``v_k = (double)k / (double)q``.
* Counts per column: ``n_k`` valid cells at level ``k``, ``e_k`` of them with an event (int32);
  ``n = sum n_k``, ``E = sum e_k``.
* Fit per column: PAV over the non-empty levels ascending with a stack of blocks
  ``(E_b, N_b)``: push ``(e_k, n_k)``; while the block below the top has a mean ``>=`` the
  top's -- decided exactly in int64, ``E_prev * N_top >= E_top * N_prev`` -- merge the two.
  ``cal_k = (double)E_b / (double)N_b`` of the level's block, NaN at an empty level.
* Statistics, every fp64 operation rounded once, no fma, sums from ``+0``::

      S     = (sum_k [(double)(n_k - e_k) * (v*v) + (double)e_k * ((1-v)*(1-v))]) / (double)n
      S_cal = (sum_b (double)E_b * ((double)(N_b - E_b) / (double)N_b)) / (double)n
      UNC   = (double)E * ((double)(n - E) / (double)n) / (double)n
      MCB   = S - S_cal          DSC = UNC - S_cal
      AUC   = (double)A2 / ((2.0 * (double)E) * (double)(n - E))
      A2    = sum_k e_k * (2 * C_k + (n_k - e_k))    C_k: the non-events at levels below k

  over the non-empty levels and the blocks ascending.  ``S`` is the Brier score of the lattice
  forecast ``v_k``; it differs from the Brier score of ``p`` itself by at most ``1/q``
  (``|v - p| <= 1/(2q)`` and ``|(v - o)^2 - (p - o)^2| <= 2 |v - p|``).  IEEE results stand:
  ``n = 0`` gives NaN everywhere, ``E = 0`` or ``E = n`` NaN for AUC.
* Resampling, with ``mix`` of :mod:`raincast_gnn.compare`: for global replicate ``r`` and row
  ``i``, ``U = mix(seed, r * N + i) >> 11`` (mod 2^64); the synthetic event of cell ``(i, t)``
  is ``U < (uint64)floor(v_k * 2^53)``.  All columns share ``U``: exceedance probabilities fall
  with the threshold, so the synthetic events are nested as real ones are, and column subsets
  and replicate chunks give the same bits.  Per ``(r, t)``: ``e*_k`` over the valid cells,
  ``n_k`` unchanged, the same fit: ``cal*_k``, ``S*``, ``S*_cal``, ``MCB*``.
* ``p_value = (1 + #{r : MCB*_r >= MCB}) / (R + 1)`` (NaN where ``MCB`` is); the band at level
  ``k`` is the percentile interval of ``cal*_k`` over ``r`` (torch, as
  :func:`raincast_gnn.compare.percentile_interval`).

fp64 HIP tensors go to ``gine_reliability_counts`` / ``_fit`` / ``_resample`` (csrc/
gine_reliability.hip) on the current stream, ``p`` read in place through its strides.  CPU
tensors and non-fp64 ``p`` take the numpy formulation of the same definitions below,
bit-identical in every field.

Command line::

    python -m raincast_gnn.reliability --dir RUN --data rf --thresholds-mm 0.1 1 5 10
        [--levels 1000 --replicates 1000 --seed 0 --band 0.9]

reads ``RUN/params.json`` and ``RUN/results/<data>.csv`` as :mod:`raincast_gnn.compare` does and
writes ``RUN/results/reliability_<data>.csv``.
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
from .compare import _np_mix, percentile_interval

log = logging.getLogger("raincast_gnn.reliability")

MAX_LEVELS = _lib.RELIABILITY_MAX_LEVELS
REPS_PER_BLOCK = _lib.RELIABILITY_REPS_PER_BLOCK
_QUANTILE_ELEMENTS = 1 << 24  # torch.quantile's input limit
STAT_FIELDS = ("n", "E", "S", "S_cal", "UNC", "MCB", "DSC", "AUC")
_TRAVERSALS = {"auto": _lib.RELIABILITY_AUTO, "atomic": _lib.RELIABILITY_ATOMIC,
               "ballot": _lib.RELIABILITY_BALLOT}


@dataclass
class ReliabilityFit:
    """What :meth:`Reliability.fit` returns.  ``v [K]``; ``n_k``, ``e_k`` ``[T, K]`` int32;
    ``cal [T, K]`` (NaN at empty levels); ``block_id [T, K]`` (-1 at empty levels);
    ``block_e``, ``block_n`` ``[T, K]``: entry ``b < num_blocks[t]`` is block ``b``, the rest 0;
    ``a2 [T]`` int64; ``stats [T, 8]`` = ``n, E, S, S_cal, UNC, MCB, DSC, AUC``, also by name."""
    v: torch.Tensor
    n_k: torch.Tensor
    e_k: torch.Tensor
    cal: torch.Tensor
    block_id: torch.Tensor
    block_e: torch.Tensor
    block_n: torch.Tensor
    num_blocks: torch.Tensor
    a2: torch.Tensor
    stats: torch.Tensor
    thresholds: torch.Tensor

    def __getattr__(self, name):
        if name in STAT_FIELDS:
            return self.stats[:, STAT_FIELDS.index(name)]
        raise AttributeError(name)

    @property
    def brier(self) -> torch.Tensor:
        """``S [T]``: the Brier score of the lattice forecast."""
        return self.stats[:, 2]

    def curve(self, t: int):
        """The reliability curve of column ``t``: ``(v, cal, n, e)`` at its non-empty levels."""
        has = self.n_k[t] > 0
        return self.v[has], self.cal[t][has], self.n_k[t][has], self.e_k[t][has]


@dataclass
class ReliabilityBands:
    """What :meth:`Reliability.resample` returns: the consistency band ``lo``, ``hi``
    ``[T, K]`` of the curve under "the forecast is reliable" (NaN at empty levels),
    ``mcb_rep [R, T]`` and the Monte-Carlo ``p_value [T]``."""
    lo: torch.Tensor
    hi: torch.Tensor
    mcb_rep: torch.Tensor
    p_value: torch.Tensor
    replicates: int
    seed: int
    rep_first: int
    level: float


# ---------------------------------------------------------------------------------- numpy (fp64)
def _np_counts(p: np.ndarray, y: np.ndarray, x: np.ndarray, q: int):
    """-> (n_k [T, K] int32, e_k [T, K] int32, level [T, N] int16)."""
    N, T = p.shape
    K = q + 1
    with np.errstate(invalid="ignore"):
        ok = (~np.isnan(y))[:, None] & (~np.isnan(x))[None, :] & (p >= 0.0) & (p <= 1.0)
        k = np.rint(np.where(ok, p, 0.0) * np.float64(q)).astype(np.int64)
        event = ok & (y.astype(np.float64)[:, None] > x[None, :])
    level = np.where(ok, k, -1).astype(np.int16).T.copy()
    n_k = np.zeros((T, K), np.int32)
    e_k = np.zeros((T, K), np.int32)
    for t in range(T):
        n_k[t] = np.bincount(k[ok[:, t], t], minlength=K)
        e_k[t] = np.bincount(k[event[:, t], t], minlength=K)
    return n_k, e_k, level


def _pav(levels, e, n):
    """PAV over the non-empty ``levels`` (ascending) with events ``e`` and cells ``n`` (Python
    ints) -> blocks ``[E_b, N_b, first level]``."""
    blocks = []
    for k, ek, nk in zip(levels, e, n):
        cE, cN, cF = ek, nk, k
        while blocks and blocks[-1][0] * cN >= cE * blocks[-1][1]:
            pE, pN, cF = blocks.pop()
            cE += pE
            cN += pN
        blocks.append((cE, cN, cF))
    return blocks


def _calibrated_sum(blocks) -> np.float64:
    s = np.float64(0.0)
    for E, N, _ in blocks:
        s = s + np.float64(E) * (np.float64(N - E) / np.float64(N))
    return s


def _lattice(q: int):
    """-> (v [K], v*v, (1-v)*(1-v))."""
    v = np.arange(q + 1, dtype=np.float64) / np.float64(q)
    w = 1.0 - v
    return v, v * v, w * w


def _fill_cal(cal_row, id_row, blocks, levels):
    """cal and block id of the non-empty ``levels`` from ``blocks``."""
    firsts = np.array([b[2] for b in blocks], dtype=np.int64)
    which = np.searchsorted(firsts, levels, side="right") - 1
    mean = np.array([np.float64(b[0]) / np.float64(b[1]) for b in blocks], dtype=np.float64)
    cal_row[levels] = mean[which]
    if id_row is not None:
        id_row[levels] = which


def _np_fit(n_k: np.ndarray, e_k: np.ndarray, q: int) -> dict:
    T, K = n_k.shape
    _, vv, ww = _lattice(q)
    out = dict(cal=np.full((T, K), np.nan), block_id=np.full((T, K), -1, np.int32),
               block_e=np.zeros((T, K), np.int32), block_n=np.zeros((T, K), np.int32),
               num_blocks=np.zeros(T, np.int32), a2=np.zeros(T, np.int64),
               stats=np.zeros((T, 8)))
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            levels = np.nonzero(n_k[t])[0]
            n = [int(a) for a in n_k[t][levels]]
            e = [int(a) for a in e_k[t][levels]]
            S = np.float64(0.0)
            A2 = below = 0
            for k, ek, nk in zip(levels, e, n):
                S = S + (np.float64(nk - ek) * vv[k] + np.float64(ek) * ww[k])
                A2 += ek * (2 * below + (nk - ek))
                below += nk - ek
            blocks = _pav([int(k) for k in levels], e, n)
            nn, EE = sum(n), sum(e)
            fn, fE = np.float64(nn), np.float64(EE)
            S = S / fn
            S_cal = _calibrated_sum(blocks) / fn
            UNC = fE * (np.float64(nn - EE) / fn) / fn
            AUC = np.float64(A2) / ((np.float64(2.0) * fE) * np.float64(nn - EE))
            out["stats"][t] = (fn, fE, S, S_cal, UNC, S - S_cal, UNC - S_cal, AUC)
            out["a2"][t] = A2
            out["num_blocks"][t] = len(blocks)
            for b, (E, N, _) in enumerate(blocks):
                out["block_e"][t, b] = E
                out["block_n"][t, b] = N
            if blocks:
                _fill_cal(out["cal"][t], out["block_id"][t], blocks, levels)
    return out


def _np_resample(level: np.ndarray, n_k: np.ndarray, q: int, seed: int, rep_first: int,
                 replicates: int):
    """-> (cal_rep [R, T, K], stats_rep [R, T, 3], e_rep [R, T, K] int32)."""
    T, N = level.shape
    K, R = q + 1, int(replicates)
    v, vv, ww = _lattice(q)
    thr = np.floor(v * 9007199254740992.0).astype(np.uint64)
    cal = np.full((R, T, K), np.nan)
    stats = np.zeros((R, T, 3))
    e_rep = np.zeros((R, T, K), np.int32)
    ok = (level >= 0) & (level < K)
    lv = np.where(ok, level, 0).astype(np.int64)
    step = max(1, (1 << 22) // max(N, 1))
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        with np.errstate(over="ignore"):
            r = np.uint64(rep_first & 0xFFFFFFFFFFFFFFFF) + np.arange(r0, r1, dtype=np.uint64)
            i = r[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
        U = _np_mix(seed, i) >> np.uint64(11)
        rows = np.arange(r1 - r0, dtype=np.int64)[:, None] * K
        for t in range(T):
            fire = ok[t][None, :] & (U < thr[lv[t]][None, :])
            idx = np.broadcast_to(rows + lv[t][None, :], fire.shape)[fire]
            e_rep[r0:r1, t] = np.bincount(idx, minlength=(r1 - r0) * K).reshape(r1 - r0, K)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            levels = np.nonzero(n_k[t])[0]
            n = [int(a) for a in n_k[t][levels]]
            fn = np.float64(sum(n))
            S = np.zeros(R)
            for k, nk in zip(levels, n):  # sequentially over the levels, all replicates at once
                ek = e_rep[:, t, k].astype(np.int64)
                S = S + ((nk - ek).astype(np.float64) * vv[k] + ek.astype(np.float64) * ww[k])
            S = S / fn
            lev = [int(k) for k in levels]
            for r in range(R):
                blocks = _pav(lev, [int(a) for a in e_rep[r, t][levels]], n)
                S_cal = _calibrated_sum(blocks) / fn
                stats[r, t] = (S[r], S_cal, S[r] - S_cal)
                if blocks:
                    _fill_cal(cal[r, t], None, blocks, levels)
    return cal, stats, e_rep


# ---------------------------------------------------------------------------------- the object
class Reliability:
    """The probabilities ``p [N, T]`` of the events "``y`` exceeds ``thresholds[t]``" beside the
    outcomes ``y [N]`` (NaN = missing; thresholds in ``y``'s space), on a lattice of ``levels``
    steps.  ``p`` is read in place (a column view of a wider tensor costs nothing)."""

    def __init__(self, p: torch.Tensor, y: torch.Tensor, thresholds, levels: int = 1000):
        if p.dim() != 2:
            raise ValueError(f"p must be [N, T], got {tuple(p.shape)}")
        q = int(levels)
        if not 1 <= q <= MAX_LEVELS:
            raise ValueError(f"levels must be in 1..{MAX_LEVELS}, got {levels}")
        self.p = p.detach()
        N, T = self.p.shape
        if N >= 2 ** 30:
            raise ValueError("at most 2^30 - 1 rows")
        self.y = y.detach().to(self.p.device).float().reshape(-1).contiguous()
        if self.y.numel() != N:
            raise ValueError(f"y must have {N} entries, got {self.y.numel()}")
        self.x = torch.as_tensor(thresholds, dtype=torch.float64,
                                 device=self.p.device).reshape(-1).contiguous()
        if self.x.numel() != T:
            raise ValueError(f"p has {T} columns, thresholds {self.x.numel()} entries")
        self.q = q
        self._counts = None
        self._fit = None

    # ------------------------------------------------------------------ layout
    @property
    def device(self):
        return self.p.device

    @property
    def num_levels(self) -> int:
        return self.q + 1

    @property
    def on_kernel(self) -> bool:
        """Whether the HIP kernels take these inputs (else the numpy formulation)."""
        return (self.p.is_cuda and self.p.dtype == torch.float64
                and self.p.stride(0) >= 0 and self.p.stride(1) >= 0)

    def _to(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    # ------------------------------------------------------------------ counts
    def counts(self):
        """``(n_k, e_k, level)``: ``[T, K]`` int32 twice and ``[T, N]`` int16 (-1: invalid)."""
        if self._counts is None:
            N, T = self.p.shape
            K = self.q + 1
            if self.on_kernel:
                n_k = torch.empty(T, K, dtype=torch.int32, device=self.device)
                e_k = torch.empty(T, K, dtype=torch.int32, device=self.device)
                level = torch.empty(T, N, dtype=torch.int16, device=self.device)
                _lib.call("gine_reliability_counts", _lib.ptr(self.p), self.p.stride(0),
                          self.p.stride(1), _lib.ptr(self.y), _lib.ptr(self.x), N, T, self.q,
                          _lib.ptr(n_k), _lib.ptr(e_k), _lib.ptr(level),
                          _lib.stream_handle(self.device))
            else:
                n_k, e_k, level = (self._to(a) for a in _np_counts(
                    self.p.double().cpu().numpy(), self.y.cpu().numpy(), self.x.cpu().numpy(),
                    self.q))
            self._counts = (n_k, e_k, level)
        return self._counts

    # ------------------------------------------------------------------ fit
    def fit(self) -> ReliabilityFit:
        """The CORP curve and the statistics of every column."""
        if self._fit is not None:
            return self._fit
        n_k, e_k, _ = self.counts()
        T, K = n_k.shape
        dev = self.device
        v = self._to(_lattice(self.q)[0])  # a device division by a scalar is a multiplication
        if self.on_kernel:
            cal = torch.empty(T, K, dtype=torch.float64, device=dev)
            ids, be, bn = (torch.empty(T, K, dtype=torch.int32, device=dev) for _ in range(3))
            nb = torch.empty(T, dtype=torch.int32, device=dev)
            a2 = torch.empty(T, dtype=torch.int64, device=dev)
            stats = torch.empty(T, 8, dtype=torch.float64, device=dev)
            _lib.call("gine_reliability_fit", _lib.ptr(n_k), _lib.ptr(e_k), T, self.q,
                      _lib.ptr(cal), _lib.ptr(ids), _lib.ptr(be), _lib.ptr(bn), _lib.ptr(nb),
                      _lib.ptr(a2), _lib.ptr(stats), _lib.stream_handle(dev))
        else:
            f = _np_fit(n_k.cpu().numpy(), e_k.cpu().numpy(), self.q)
            cal, ids, be, bn, nb, a2, stats = (self._to(f[k]) for k in (
                "cal", "block_id", "block_e", "block_n", "num_blocks", "a2", "stats"))
        self._fit = ReliabilityFit(v, n_k, e_k, cal, ids, be, bn, nb, a2, stats, self.x)
        return self._fit

    # ------------------------------------------------------------------ resampling
    def replicates(self, replicates: int, seed: int = 0, rep_first: int = 0, *,
                   columns: slice | None = None, events: bool = False,
                   traversal: str = "auto"):
        """Replicates ``rep_first .. rep_first + replicates - 1`` of the columns in ``columns``
        (a slice; all by default): ``(cal_rep [R, T, K], stats_rep [R, T, 3])`` and, with
        ``events``, ``e_rep [R, T, K]`` int32.  ``traversal``: ``"auto"``, ``"atomic"`` or
        ``"ballot"`` (``K <= 64``), how the kernel counts; the bits are the same."""
        n_k, _, level = self.counts()
        if columns is not None:
            n_k, level = n_k[columns], level[columns]
        T, K = n_k.shape
        N, R = level.size(1), int(replicates)
        if R < 0:
            raise ValueError(f"replicates must not be negative, got {replicates}")
        if traversal not in _TRAVERSALS:
            raise ValueError(f"traversal must be one of {sorted(_TRAVERSALS)}, got {traversal!r}")
        if traversal == "ballot" and K > _lib.RELIABILITY_BALLOT_MAX_LEVELS:
            raise ValueError(f"the ballot traversal takes at most "
                             f"{_lib.RELIABILITY_BALLOT_MAX_LEVELS} levels, got {K}")
        dev = self.device
        if self.on_kernel:
            cal = torch.empty(R, T, K, dtype=torch.float64, device=dev)
            stats = torch.empty(R, T, 3, dtype=torch.float64, device=dev)
            e_rep = torch.empty(R, T, K, dtype=torch.int32, device=dev) if events else None
            _lib.call("gine_reliability_resample", _lib.ptr(level), _lib.ptr(n_k), N, T, self.q,
                      seed & 0xFFFFFFFFFFFFFFFF, rep_first & 0xFFFFFFFFFFFFFFFF, R,
                      _TRAVERSALS[traversal], _lib.ptr(cal), _lib.ptr(stats), _lib.ptr(e_rep),
                      _lib.stream_handle(dev))
        else:
            cal, stats, e_rep = (self._to(a) for a in _np_resample(
                level.cpu().numpy(), n_k.cpu().numpy(), self.q, seed, rep_first, R))
        return (cal, stats, e_rep) if events else (cal, stats)

    def resample(self, replicates: int = 1000, seed: int = 0, rep_first: int = 0,
                 level: float = 0.9, max_bytes: int = 256 << 20) -> ReliabilityBands:
        """Consistency resampling: the band of the curve at ``level`` and the Monte-Carlo
        p-value of "the forecast is reliable".  The columns are cut into groups and the
        replicates into chunks so that no buffer a kernel writes in one call exceeds
        ``max_bytes`` (the chunks give the same bits: all columns share the draws and row ``i``
        of a call is replicate ``rep_first + i``)."""
        R = int(replicates)
        if R < 1:
            raise ValueError(f"replicates must be at least 1, got {replicates}")
        if not 0.0 < level < 1.0:
            raise ValueError(f"level must be in (0, 1), got {level}")
        fit = self.fit()
        T, K = fit.n_k.shape
        dev = self.device
        cells = max(1, int(max_bytes) // 8)
        t_chunk = min(max(T, 1), max(1, min(cells, _QUANTILE_ELEMENTS) // (R * K)))
        r_chunk = min(R, max(1, cells // (t_chunk * K)))
        k_chunk = max(1, _QUANTILE_ELEMENTS // (R * t_chunk))
        lo = torch.empty(T, K, dtype=torch.float64, device=dev)
        hi = torch.empty(T, K, dtype=torch.float64, device=dev)
        mcb_rep = torch.empty(R, T, dtype=torch.float64, device=dev)
        for t0 in range(0, T, t_chunk):
            cols = slice(t0, min(T, t0 + t_chunk))
            cal_all = torch.empty(R, cols.stop - t0, K, dtype=torch.float64, device=dev)
            for r0 in range(0, R, r_chunk):
                n = min(r_chunk, R - r0)
                cal, stats = self.replicates(n, seed, rep_first + r0, columns=cols)
                cal_all[r0:r0 + n] = cal
                mcb_rep[r0:r0 + n, cols] = stats[:, :, 2]
            for k0 in range(0, K, k_chunk):
                ci = percentile_interval(cal_all[:, :, k0:k0 + k_chunk], level)
                lo[cols, k0:k0 + k_chunk] = ci[0]
                hi[cols, k0:k0 + k_chunk] = ci[1]
        mcb = fit.stats[:, 5]
        count = (mcb_rep >= mcb.unsqueeze(0)).sum(0).double()
        # tensor by tensor: a true division on the device (by a scalar it is a multiplication)
        p_value = torch.where(torch.isnan(mcb), torch.full_like(mcb, float("nan")),
                              (1.0 + count) / torch.full_like(count, float(R + 1)))
        return ReliabilityBands(lo, hi, mcb_rep, p_value, R, int(seed), int(rep_first),
                                float(level))


# ---------------------------------------------------------------------------------- command line
def _read_run(run: str, data: str, device):
    """-> (Forecast, targets [N] fp32) of ``run/results/<data>.csv``."""
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
    return Forecast.from_model(model, table[:, 1:].float().to(device)), y


def main(argv=None):
    ap = argparse.ArgumentParser(description="Reliability diagram of a run's exceedance "
                                             "probabilities: CORP curve, consistency band, "
                                             "MCB / DSC / UNC per threshold.")
    ap.add_argument("--dir", required=True, help="run directory (params.json, results/)")
    ap.add_argument("--data", required=True, help="results/<data>.csv of the run")
    ap.add_argument("--thresholds-mm", type=float, nargs="+", required=True)
    ap.add_argument("--levels", type=int, default=1000)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--band", type=float, default=0.9)
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is one")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s",
                        handlers=[logging.StreamHandler(sys.stdout)])
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    forecast, y = _read_run(args.dir, args.data, device)
    rel = forecast.reliability(y, args.thresholds_mm, unit="mm", levels=args.levels)
    fit = rel.fit()
    bands = rel.resample(args.replicates, seed=args.seed, level=args.band)
    stats, pv = fit.stats.cpu().tolist(), bands.p_value.cpu().tolist()
    log.info("%s on %s: %d levels, %d replicates, band %.2f", args.dir, args.data, args.levels,
             args.replicates, args.band)
    log.info("%10s %9s %9s %9s %9s %9s %7s %7s", "mm", "n", "Brier", "MCB", "DSC", "UNC", "AUC",
             "p")
    for t, mm in enumerate(args.thresholds_mm):
        n, _, S, _, UNC, MCB, DSC, AUC = stats[t]
        log.info("%10g %9d %9.6f %9.6f %9.6f %9.6f %7.4f %7.4f", mm, int(n) if n == n else 0, S,
                 MCB, DSC, UNC, AUC, pv[t])
    out_dir = os.path.join(args.dir, "results")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"reliability_{args.data}.csv")
    with open(path, "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(["threshold", "v", "n", "e", "cal", "lo", "hi"])
        lo, hi = bands.lo.cpu(), bands.hi.cpu()
        for t, mm in enumerate(args.thresholds_mm):
            has = (fit.n_k[t] > 0).cpu()
            v, cal, n, e = (a.cpu().tolist() for a in fit.curve(t))
            for j, (a, b) in enumerate(zip(lo[t][has].tolist(), hi[t][has].tolist())):
                writer.writerow([repr(mm), repr(v[j]), n[j], e[j], repr(cal[j]), repr(a),
                                 repr(b)])
    log.info("wrote %s", path)
    return rel, fit, bands


if __name__ == "__main__":
    main()
