"""Members scored as fields, per graph: the energy score over a graph's stations, the variogram
score over its station pairs, and the ensemble scores of an area aggregate.

Per-row scores (CRPS, PIT, Brier, twCRPS) look at marginals only: they cannot tell the members
of :meth:`Forecast.ecc <raincast_gnn.forecast.Forecast.ecc>`, which keep the raw ensemble's rank
structure across stations, from independently shuffled quantiles.  These scores can.

A batch is ``members [N, M]``, targets ``y [N]`` (NaN = missing) and ``ptr [G + 1]`` (the rows
of graph ``g`` are ``ptr[g] .. ptr[g+1] - 1``, as ``GraphBatch.ptr``); member values are
``x = shift + scale * members`` in fp64, in model space ``log(mm + 0.01)``.  Per graph:

* ``S`` = the rows with a non-NaN target and at least one non-NaN member, ``rows_valid = |S|``;
* ``V`` = the members non-NaN at every row of ``S`` (a member missing at one station is not a
  field there: it is dropped for that graph only; all ``M`` for an empty ``S``),
  ``members_valid = m = |V|``;
* every score is NaN when ``S`` is empty or ``m = 0``; the two counts never are;
* ``es = (1/m) sum_i |X_i - y| - (1/(2 m^2)) sum_ij |X_i - X_j|`` with the Euclidean norm over
  ``S`` and ``i, j`` in ``V``; ``es_fair`` with ``1/(2 m (m - 1))`` (NaN for ``m < 2``);
* ``vs = sum_{a<b in S} (|y_a - y_b|^p - (1/m) sum_i |X_ai - X_bi|^p)^2`` with unit weights,
  ``pairs = |S| (|S| - 1) / 2``;
* area aggregates in millimetres, ``mm(x) = max(exp(x) - 0.01, 0)``: ``A_i`` = the max or mean
  over ``S`` of ``mm(X_ni)`` for ``i`` in ``V`` (NaN otherwise), ``obs`` the same of ``mm(y)``,
  then ``crps``, ``crps_fair``, ``rank_lo``, ``rank_hi`` of :mod:`raincast_gnn.ensemble` on them.

The scores do not depend on the order of rows within a graph except for rounding.  HIP tensors
with at most 64 members go to ``gine_field_energy`` / ``_variogram`` / ``_area``
(csrc/gine_field.hip), on the current stream and without host synchronisation; CPU tensors and
wider ensembles go to the fp64 torch formulation of the same definitions below, graph by graph.
These are scores, not losses: there are no gradients.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib

STATS = {"max": _lib.FIELD_MAX, "mean": _lib.FIELD_MEAN}
MM_OFFSET = 0.01
_CHUNK_ELEMENTS = 1 << 22  # the torch variogram holds at most this many [chunk, n, m] doubles


@dataclass
class AreaScore:
    """The area aggregate of every member ``members [G, M]`` (mm; NaN outside ``V``) and of the
    targets ``obs [G]``, and the scalar ensemble scores of the first against the second."""
    members: torch.Tensor
    obs: torch.Tensor
    crps: torch.Tensor
    crps_fair: torch.Tensor
    rank_lo: torch.Tensor
    rank_hi: torch.Tensor


@dataclass
class FieldScore:
    """Everything :meth:`MemberFields.score` computes, ``[G]`` fp64 each."""
    es: torch.Tensor
    es_fair: torch.Tensor
    vs: torch.Tensor
    pairs: torch.Tensor
    area: AreaScore
    members_valid: torch.Tensor
    rows_valid: torch.Tensor


def _partials(name: str, *sizes) -> int:
    n = ctypes.c_size_t(0)
    _lib.call(name, *sizes, ctypes.byref(n))
    return n.value


class MemberFields:
    """``members [N, M]`` (fp32 or fp64, any strides: nothing is copied) cut into graphs by
    ``ptr [G + 1]``; ``ptr`` is checked here, once, so the scoring methods never synchronise."""

    def __init__(self, members: torch.Tensor, ptr: torch.Tensor, *, scale: float = 1.0,
                 shift: float = 0.0):
        if members.dim() != 2:
            raise ValueError(f"members must be [N, M], got {tuple(members.shape)}")
        if members.size(1) == 0:
            raise ValueError("a field needs at least one member")
        if members.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"members must be float32 or float64, got {members.dtype}")
        ptr = torch.as_tensor(ptr)
        if ptr.dim() != 1 or ptr.numel() < 1 or ptr.dtype.is_floating_point:
            raise ValueError("ptr must be a one-dimensional integer tensor [G + 1]")
        if ptr.device != members.device:
            raise ValueError(f"ptr is on {ptr.device}, the members on {members.device}")
        host = ptr.detach().cpu().long()
        if int(host[0]) != 0 or int(host[-1]) != members.size(0):
            raise ValueError(f"ptr must run from 0 to N = {members.size(0)}, got "
                             f"{int(host[0])} .. {int(host[-1])}")
        if bool((host[1:] < host[:-1]).any()):
            raise ValueError("ptr must be non-decreasing")
        self.members = members.detach()
        self.ptr = ptr.detach().long().contiguous()
        self._host_ptr = host.tolist()
        self.scale, self.shift = float(scale), float(shift)

    def with_members(self, members: torch.Tensor, *, scale: float = 1.0,
                     shift: float = 0.0) -> "MemberFields":
        """Other members over the same graphs (``Forecast.ecc`` output beside the raw ensemble):
        ``ptr`` was checked already, so this does not synchronise and may be captured."""
        if members.dim() != 2 or members.size(0) != self.members.size(0) or members.size(1) == 0:
            raise ValueError(f"members must be [{self.members.size(0)}, M], got "
                             f"{tuple(members.shape)}")
        if members.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"members must be float32 or float64, got {members.dtype}")
        if members.device != self.device:
            raise ValueError(f"members are on {members.device}, ptr on {self.device}")
        other = object.__new__(MemberFields)
        other.members, other.ptr, other._host_ptr = members.detach(), self.ptr, self._host_ptr
        other.scale, other.shift = float(scale), float(shift)
        return other

    @classmethod
    def from_raw(cls, raw, ptr) -> "MemberFields":
        """The members of a :class:`raincast_gnn.ensemble.RawEnsemble`, with its affine."""
        return cls(raw.members, ptr, scale=raw.scale, shift=raw.shift)

    @classmethod
    def from_batch(cls, batch, column: int, mean: float = 0.0,
                   std: float = 1.0) -> "MemberFields":
        """Column ``column`` of ``batch.ensemble [N, E, F]`` as a view over ``batch.ptr``, the
        dataset's StandardScaler undone (``value = mean + std * stored``)."""
        ens = batch.ensemble
        if ens.dim() != 3:
            raise ValueError(f"ensemble must be [N, E, F], got {tuple(ens.shape)}")
        if not -ens.size(2) <= column < ens.size(2):
            raise ValueError(f"column {column} outside the {ens.size(2)} features")
        return cls(ens[:, :, column], batch.ptr, scale=std, shift=mean)

    # ------------------------------------------------------------------ public
    @property
    def device(self):
        return self.members.device

    @property
    def num_graphs(self) -> int:
        return self.ptr.numel() - 1

    @property
    def on_kernel(self) -> bool:
        """Whether the HIP kernels take these members (else the torch formulation)."""
        return (self.members.is_cuda and self.members.size(1) <= _lib.ENSEMBLE_MAX_MEMBERS
                and self.members.size(0) > 0 and self.num_graphs > 0)

    def values(self) -> torch.Tensor:
        """The members in model space, fp64 ``[N, M]``."""
        return self.shift + self.scale * self.members.double()

    def energy(self, y: torch.Tensor):
        """-> ``(es, es_fair, members_valid, rows_valid)``, each ``[G]`` fp64."""
        y = self._targets(y)
        if not self.on_kernel:
            r = self._torch(y, 0.5, "max", ("energy",))
            return r["es"], r["es_fair"], r["members_valid"], r["rows_valid"]
        N, M = self.members.shape
        out = self._empty(4)
        ws = self._workspace(_partials("gine_field_energy_partials", N, self.num_graphs, M))
        _lib.call("gine_field_energy", *self._member_args(), _lib.ptr(y), N, _lib.ptr(self.ptr),
                  self.num_graphs, *[_lib.ptr(o) for o in out], _lib.ptr(ws),
                  _lib.stream_handle(self.device))
        return out[0], out[1], out[2], out[3]

    def variogram(self, y: torch.Tensor, p: float = 0.5):
        """-> ``(vs, pairs)`` of order ``p > 0``, each ``[G]`` fp64."""
        p = self._order(p)
        y = self._targets(y)
        if not self.on_kernel:
            r = self._torch(y, p, "max", ("variogram",))
            return r["vs"], r["pairs"]
        N = self.members.size(0)
        out = self._empty(2)
        ws = self._workspace(_partials("gine_field_variogram_partials", N, self.num_graphs))
        _lib.call("gine_field_variogram", *self._member_args(), _lib.ptr(y), N,
                  _lib.ptr(self.ptr), self.num_graphs, p, _lib.ptr(out[0]), _lib.ptr(out[1]),
                  None, None, _lib.ptr(ws), _lib.stream_handle(self.device))
        return out[0], out[1]

    def area(self, y: torch.Tensor, stat: str = "max") -> AreaScore:
        """The scores of the area ``stat`` (``"max"`` or ``"mean"``, in mm)."""
        if stat not in STATS:
            raise ValueError(f"stat must be 'max' or 'mean', got {stat!r}")
        y = self._targets(y)
        if not self.on_kernel:
            return self._torch(y, 0.5, stat, ("area",))["area"]
        N, M = self.members.shape
        G = self.num_graphs
        mem = torch.empty(G, M, dtype=torch.float64, device=self.device)
        out = self._empty(5)
        _lib.call("gine_field_area", *self._member_args(), _lib.ptr(y), N, _lib.ptr(self.ptr), G,
                  STATS[stat], _lib.ptr(mem), *[_lib.ptr(o) for o in out], None, None, None,
                  _lib.stream_handle(self.device))
        return AreaScore(mem, out[0], out[1], out[2], out[3], out[4])

    def score(self, y: torch.Tensor, p: float = 0.5, stat: str = "max") -> FieldScore:
        """All three scores of the targets ``y [N]`` (model space, NaN = missing)."""
        p = self._order(p)
        if stat not in STATS:
            raise ValueError(f"stat must be 'max' or 'mean', got {stat!r}")
        if not self.on_kernel:
            r = self._torch(self._targets(y), p, stat, ("energy", "variogram", "area"))
            return FieldScore(r["es"], r["es_fair"], r["vs"], r["pairs"], r["area"],
                              r["members_valid"], r["rows_valid"])
        es, fair, m, rows = self.energy(y)
        vs, pairs = self.variogram(y, p)
        return FieldScore(es, fair, vs, pairs, self.area(y, stat), m, rows)

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _order(p) -> float:
        p = float(p)
        if not 0.0 < p < float("inf"):
            raise ValueError(f"the variogram order must be positive and finite, got {p!r}")
        return p

    def _targets(self, y: torch.Tensor) -> torch.Tensor:
        if y.device != self.device:
            raise ValueError(f"y is on {y.device}, the members on {self.device}")
        y = y.detach().float().reshape(-1).contiguous()
        if y.numel() != self.members.size(0):
            raise ValueError(f"y must have {self.members.size(0)} entries, got {y.numel()}")
        return y

    def _member_args(self):
        mem = self.members
        dtype = _lib.FIELD_F64 if mem.dtype == torch.float64 else _lib.FIELD_F32
        return (_lib.ptr(mem), dtype, mem.stride(0), mem.stride(1), mem.size(1), self.scale,
                self.shift)

    def _empty(self, k: int):
        return torch.empty(k, self.num_graphs, dtype=torch.float64, device=self.device)

    def _workspace(self, count: int) -> torch.Tensor:
        return torch.empty(max(count, 1), dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------ torch (fp64)
    def _torch(self, y: torch.Tensor, p: float, stat: str, what) -> dict:
        G, M, dev = self.num_graphs, self.members.size(1), self.device
        nan = float("nan")
        cols = {k: [nan] * G for k in ("es", "es_fair", "vs", "obs", "crps", "crps_fair",
                                       "rank_lo", "rank_hi")}
        cols.update(pairs=[0.0] * G, members_valid=[0.0] * G, rows_valid=[0.0] * G)
        agg = torch.full((G, M), nan, dtype=torch.float64, device=dev)
        x_all, y_all = self.values(), y.double()
        for g in range(G):
            p0, p1 = self._host_ptr[g], self._host_ptr[g + 1]
            x, yy = x_all[p0:p1], y_all[p0:p1]
            in_s = ~torch.isnan(yy) & (~torch.isnan(x)).any(1)
            x, yy = x[in_s], yy[in_s]
            in_v = ~torch.isnan(x).any(0)
            n, m = x.size(0), int(in_v.sum())
            cols["rows_valid"][g], cols["members_valid"][g] = float(n), float(m)
            cols["pairs"][g] = n * (n - 1) / 2.0
            if n == 0 or m == 0:
                continue
            X = x[:, in_v]
            if "energy" in what:
                cols["es"][g], cols["es_fair"][g] = self._energy_torch(X, yy)
            if "variogram" in what:
                cols["vs"][g] = self._variogram_torch(X, yy, p)
            if "area" in what:
                a, res = self._area_torch(X, yy, stat)
                agg[g, in_v] = a
                for k, v in zip(("obs", "crps", "crps_fair", "rank_lo", "rank_hi"), res):
                    cols[k][g] = v
        t = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in cols.items()}
        t["area"] = AreaScore(agg, t["obs"], t["crps"], t["crps_fair"], t["rank_lo"],
                              t["rank_hi"])
        return t

    @staticmethod
    def _energy_torch(X: torch.Tensor, y: torch.Tensor):
        n, m = X.shape
        to_obs = (X - y.unsqueeze(1)).pow(2).sum(0).sqrt().sum()
        sq = torch.zeros(m, m, dtype=torch.float64, device=X.device)
        step = max(1, _CHUNK_ELEMENTS // (m * m))
        for a in range(0, n, step):
            blk = X[a:a + step]
            sq += (blk.unsqueeze(2) - blk.unsqueeze(1)).pow(2).sum(0)
        between = sq.sqrt().sum()
        es = to_obs / m - between / (2.0 * m * m)
        fair = to_obs / m - between / (2.0 * m * (m - 1)) if m > 1 else float("nan")
        return float(es), float(fair)

    @staticmethod
    def _power(d: torch.Tensor, p: float) -> torch.Tensor:
        if p == 0.5:
            return d.sqrt()
        if p == 1.0:
            return d
        if p == 2.0:
            return d * d
        return d.pow(p)

    @classmethod
    def _variogram_torch(cls, X: torch.Tensor, y: torch.Tensor, p: float) -> float:
        n, m = X.shape
        step = max(1, _CHUNK_ELEMENTS // (n * m))
        index = torch.arange(n, device=X.device)
        total = torch.zeros((), dtype=torch.float64, device=X.device)
        for a in range(0, n, step):
            d = cls._power((X[a:a + step].unsqueeze(1) - X.unsqueeze(0)).abs(), p).sum(2) / m
            w = cls._power((y[a:a + step].unsqueeze(1) - y.unsqueeze(0)).abs(), p)
            upper = index[a:a + step].unsqueeze(1) < index.unsqueeze(0)
            total += torch.where(upper, (w - d).pow(2), torch.zeros_like(d)).sum()
        return float(total)

    @staticmethod
    def _area_torch(X: torch.Tensor, y: torch.Tensor, stat: str):
        m = X.size(1)
        mm = torch.clamp(torch.exp(X) - MM_OFFSET, min=0.0)
        my = torch.clamp(torch.exp(y) - MM_OFFSET, min=0.0)
        a, obs = (mm.max(0).values, my.max()) if stat == "max" else (mm.mean(0), my.mean())
        to_obs = (a - obs).abs().sum()
        between = (a.unsqueeze(0) - a.unsqueeze(1)).abs().sum()
        crps = to_obs / m - between / (2.0 * m * m)
        fair = to_obs / m - between / (2.0 * m * (m - 1)) if m > 1 else float("nan")
        return a, (float(obs), float(crps), float(fair), float((a < obs).sum()),
                   float((a <= obs).sum()))
