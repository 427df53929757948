"""Permutation feature importance on the device.

Which inputs does the model use?  Permute a group of feature columns over samples and stations,
score the model on the permuted data, and compare with the unpermuted score: the importance of
the group is ``permuted_score / base_score - 1`` (the analysis the GNN post-processing paper
reports in CRPS).  The permutation restates the reference's ``utils/data.py: shuffle_features``
-- shuffle the time axis, then the stations differently for each time -- applied to the station
features and to every ensemble member alike.  For a dataset ``x [T, N, F]``, ``ensemble
[T, N, M, F]``, ``y [T, N]``, a plan ``perm_t [T]``, ``perm_n [T, N]`` and columns ``cols``::

    out_x[t, n, f]      = x[perm_t[t], perm_n[t, n], f]             f in cols
    out_ens[t, n, m, f] = ensemble[perm_t[t], perm_n[t, n], m, f]   f in cols, every m
    everything else, and y, unchanged

* :class:`PermutationPlan` -- the two permutations, drawn from a seeded CPU generator (so a run
  is the same whatever the device, as ``batching.DeviceLoader``'s order is), checked once on the
  host, and mapped to the positions a relabelled dataset stores its stations at.
* :func:`fill_batch` -- the collated batch of some samples with the columns permuted:
  ``gine_batch_fill_permuted`` (csrc/gine_batch.hip, one launch, no host synchronisation) for HIP
  tensors with at most 64 features, the torch formulation of the same thing otherwise.  Both
  give the same bits.
* :func:`permutation_importance` -- the whole table.  On a HIP device, per batch: one fill
  launch straight into the inputs of the model's captured forward (``Predictor.bind``), one
  replay, ``Forecast.score`` on the static output, and an fp64 add into device accumulators;
  nothing is read back before the table is complete.

Command line (synthetic station data, as ``raincast_gnn.train``)::

    python -m raincast_gnn.importance --dir RUN --ckpt RUN/models/run_0-best.ckpt \\
        [--repeats 5 --groups tp6 cape,tcw 3 --thresholds-mm 10]
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from dataclasses import dataclass

import torch

from . import _lib
from .batching import DeviceDataset
from .data import inverse_order

log = logging.getLogger("raincast_gnn.importance")

SCHEMES = ("time_station", "station", "time")
# the reference's feature columns in order (utils/data.py: the default feature list without
# station_id / time / number, then the two cyclical day-of-year columns)
FEATURE_NAMES = (
    "cape", "model_orography", "sd", "station_altitude", "station_latitude",
    "station_longitude", "stl1", "swvl1", "t2m", "tcc", "tcw", "tcwv", "u10", "u100", "v10",
    "v100", "vis", "cp6", "mn2t6", "mx2t6", "p10fg6", "slhf6", "sshf6", "ssr6", "ssrd6", "str6",
    "strd6", "tp6", "z", "q", "u", "v", "t", "cos_doy", "sin_doy")


def _is_permutation(p: torch.Tensor, n: int) -> bool:
    """Every row of ``p [..., n]`` holds each of 0..n-1 once."""
    if p.dtype.is_floating_point or p.dtype == torch.bool or p.size(-1) != n:
        return False
    want = torch.arange(n, dtype=torch.long).expand(p.shape)
    return bool(torch.equal(p.long().sort(dim=-1).values, want))


@dataclass
class PermutationPlan:
    """``perm_t [T]``: the sample each sample's permuted columns come from; ``perm_n [T, N]``:
    per sample, the station each station's come from, in the dataset's reference station
    order.  CPU integer tensors; None = the identity."""
    perm_t: torch.Tensor | None
    perm_n: torch.Tensor | None

    @classmethod
    def draw(cls, T: int, N: int, generator: torch.Generator,
             scheme: str = "time_station") -> "PermutationPlan":
        """``"time_station"``: the reference's scheme, ``perm_t = randperm(T)`` and ``perm_n =
        argsort(rand(T, N), dim=1)``; ``"station"``: stations only; ``"time"``: samples only.
        Only what the scheme uses is drawn from ``generator`` (a CPU generator)."""
        if scheme not in SCHEMES:
            raise ValueError(f"scheme must be one of {SCHEMES}, got {scheme!r}")
        perm_t = perm_n = None
        if scheme != "station":
            perm_t = torch.randperm(T, generator=generator)
        if scheme != "time":
            perm_n = torch.argsort(torch.rand(T, N, generator=generator), dim=1)
        return cls(perm_t, perm_n)

    def check(self, T: int, N: int) -> "PermutationPlan":
        """Raises ``ValueError`` unless both parts are permutations of the right size (the
        kernel trusts its indices: this is the one place they are looked at)."""
        if self.perm_t is not None:
            p = torch.as_tensor(self.perm_t).cpu()
            if p.dim() != 1 or not _is_permutation(p, T):
                raise ValueError(f"perm_t must be a permutation of range({T})")
        if self.perm_n is not None:
            p = torch.as_tensor(self.perm_n).cpu()
            if p.dim() != 2 or p.size(0) != T or not _is_permutation(p, N):
                raise ValueError(f"every row of perm_n [{T}, {N}] must be a permutation of "
                                 f"range({N})")
        return self

    def stored(self, order: torch.Tensor | None) -> "PermutationPlan":
        """The plan over stored positions of a dataset whose position ``i`` holds station
        ``order[i]`` (``DeviceDataset.order``): ``stored[t, i] = inv_order[perm_n[t, order[i]]]``,
        so relabelled and unrelabelled datasets permute the same stations."""
        if order is None or self.perm_n is None:
            return self
        order = order.cpu().long()
        return PermutationPlan(self.perm_t, inverse_order(order)[self.perm_n.long()[:, order]])

    def on(self, dataset: DeviceDataset) -> "DevicePlan":
        """Checked, mapped to ``dataset``'s stored positions and uploaded."""
        T, N = dataset.x.size(0), dataset.num_stations
        p = self.check(T, N).stored(dataset.order)
        dev = dataset.device
        return DevicePlan(
            None if p.perm_t is None else p.perm_t.to(dev, torch.int64).contiguous(),
            None if p.perm_n is None else p.perm_n.to(dev, torch.int32).contiguous())


@dataclass
class DevicePlan:
    """A plan as :func:`fill_batch` reads it: ``perm_t [T]`` int64 and ``perm_n [T, N]`` int32
    stored positions on the dataset's device (None = the identity)."""
    perm_t: torch.Tensor | None
    perm_n: torch.Tensor | None


@dataclass
class FilledBatch:
    """``x [B*N, F]``, ``ensemble [B*N, M, F]``, ``y [B*N]`` of a filled batch, in the dataset's
    stored station order; ``on_kernel``: whether the HIP kernel wrote them."""
    x: torch.Tensor
    ensemble: torch.Tensor
    y: torch.Tensor
    on_kernel: bool


def _columns(cols, F: int) -> list[int]:
    out = sorted({int(c) for c in cols})
    if out and not 0 <= out[0] <= out[-1] < F:
        raise ValueError(f"columns {out} outside the {F} features")
    return out


def fill_batch(dataset: DeviceDataset, idx: torch.Tensor, plan, cols, out=None,
               kernel: bool | None = None) -> FilledBatch:
    """The collated batch of the samples ``idx`` with the columns ``cols`` permuted by ``plan``
    (a :class:`PermutationPlan`, checked and uploaded here; a :class:`DevicePlan` from
    ``plan.on(dataset)``, used as it is; or None with no column).  ``out``: ``(x, ensemble, y)``
    tensors to write into (a forward's static inputs).  ``kernel``: None takes the HIP kernel
    where it applies (HIP tensors, at most 64 features), False the torch formulation; the two
    give the same bits."""
    x, ens, y = dataset.x, dataset.ensemble, dataset.y
    T, N, F = x.shape
    M = ens.size(2)
    cols = _columns(cols, F)
    if isinstance(plan, PermutationPlan):
        plan = plan.on(dataset)
    if plan is None or (plan.perm_t is None and plan.perm_n is None):
        if cols and plan is None:
            raise ValueError("fill_batch: columns to permute but no plan")
        cols = []  # both parts the identity: nothing moves
        plan = DevicePlan(None, None)
    idx = torch.as_tensor(idx)
    if not idx.is_cuda and idx.numel() and not 0 <= int(idx.min()) <= int(idx.max()) < T:
        raise ValueError(f"fill_batch: sample indices outside range({T})")  # (device indices
    idx = idx.to(dataset.device, torch.long).reshape(-1).contiguous()       # are the caller's)
    B = idx.numel()
    on_kernel = x.is_cuda and F <= _lib.BATCH_MAX_FEATURES and B > 0
    if kernel is False:
        on_kernel = False
    elif kernel and not on_kernel:
        raise _lib.GineError("fill_batch: the kernel takes HIP tensors with at most "
                             f"{_lib.BATCH_MAX_FEATURES} features")
    if out is None:
        out = (torch.empty(B * N, F, dtype=x.dtype, device=x.device),
               torch.empty(B * N, M, F, dtype=x.dtype, device=x.device),
               torch.empty(B * N, dtype=y.dtype, device=x.device))
    ox, oe, oy = out
    if (tuple(ox.shape) != (B * N, F) or tuple(oe.shape) != (B * N, M, F)
            or tuple(oy.shape) != (B * N,)):
        raise ValueError(f"fill_batch: out must be [{B * N}, {F}], [{B * N}, {M}, {F}] and "
                         f"[{B * N}]")
    if on_kernel:
        if not (x.is_contiguous() and ens.is_contiguous() and y.is_contiguous()
                and ox.is_contiguous() and oe.is_contiguous() and oy.is_contiguous()
                and all(t.dtype == torch.float32 for t in (x, ens, y, ox, oe, oy))):
            raise ValueError("fill_batch: the kernel takes contiguous float32 tensors")
        mask = 0
        for c in cols:
            mask |= 1 << c
        _lib.call("gine_batch_fill_permuted", _lib.ptr(x), _lib.ptr(ens), _lib.ptr(y),
                  _lib.ptr(idx), _lib.ptr(plan.perm_t), _lib.ptr(plan.perm_n), mask, T, N, M, F,
                  B, _lib.ptr(ox), _lib.ptr(oe), _lib.ptr(oy), _lib.stream_handle(x.device))
        return FilledBatch(ox, oe, oy, True)
    # the torch formulation: gather the samples, then overwrite the permuted columns
    gx, ge = x.index_select(0, idx), ens.index_select(0, idx)
    if cols:
        pt = idx if plan.perm_t is None else plan.perm_t[idx]
        pn = (torch.arange(N, device=x.device).expand(B, N) if plan.perm_n is None
              else plan.perm_n[idx].long())
        c = torch.tensor(cols, device=x.device)
        gx[:, :, c] = x[pt.unsqueeze(1), pn][:, :, c]
        ge[:, :, :, c] = ens[pt.unsqueeze(1), pn][:, :, :, c]
    ox.copy_(gx.reshape(B * N, F))
    oe.copy_(ge.reshape(B * N, M, F))
    oy.copy_(y.index_select(0, idx).reshape(B * N))
    return FilledBatch(ox, oe, oy, False)


# ------------------------------------------------------------------------------------------
# the importance table
# ------------------------------------------------------------------------------------------
def _feature_names(F: int) -> list[str]:
    return list(FEATURE_NAMES) if F == len(FEATURE_NAMES) else [f"f{j}" for j in range(F)]


def resolve_groups(groups, F: int) -> tuple[list[str], list[list[int]]]:
    """``groups`` -- a list whose entries are a column index, a column name (``FEATURE_NAMES``,
    for the reference's 35 columns) or a list of those -- as (labels, column lists).  None: one
    group per column."""
    names = _feature_names(F)

    def column(c) -> int:
        if isinstance(c, str):
            if c not in names:
                raise ValueError(f"unknown feature {c!r}")
            return names.index(c)
        c = int(c)
        if not 0 <= c < F:
            raise ValueError(f"column {c} outside the {F} features")
        return c

    if groups is None:
        groups = list(range(F))
    labels, cols = [], []
    for g in groups:
        members = [g] if isinstance(g, (int, str)) else list(g)
        if not members:
            raise ValueError("an empty feature group")
        cs = [column(c) for c in members]
        cols.append(cs)
        labels.append("+".join(names[c] for c in cs))
    return labels, cols


@dataclass
class FeatureImportance:
    """The table of :func:`permutation_importance` (CPU fp64 tensors).  ``base_crps``: the mean
    CRPS over the ``valid`` rows of the dataset; ``permuted_crps [G, R]``: the same with group
    ``g`` permuted, repeat ``r``; ``importance = permuted_crps / base_crps - 1``, ``mean [G]`` and
    ``std [G]`` over the repeats (the sample standard deviation; 0 for one repeat).  With
    thresholds, the same of the mean twCRPS per threshold: ``base_twcrps [K]``,
    ``permuted_twcrps`` / ``tw_importance [G, R, K]``, ``tw_mean`` / ``tw_std [G, K]``, and the
    ``thresholds [K]`` in model space."""
    groups: list
    labels: list
    base_crps: torch.Tensor
    permuted_crps: torch.Tensor
    importance: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    valid: torch.Tensor
    thresholds: torch.Tensor | None = None
    base_twcrps: torch.Tensor | None = None
    permuted_twcrps: torch.Tensor | None = None
    tw_importance: torch.Tensor | None = None
    tw_mean: torch.Tensor | None = None
    tw_std: torch.Tensor | None = None

    def rows(self) -> list[tuple]:
        """(label, mean, std[, twCRPS means...]) sorted by mean importance, largest first."""
        order = torch.argsort(self.mean, descending=True).tolist()
        out = []
        for g in order:
            row = [self.labels[g], float(self.mean[g]), float(self.std[g])]
            if self.tw_mean is not None:
                row += [float(v) for v in self.tw_mean[g]]
            out.append(tuple(row))
        return out

    def table(self) -> str:
        width = max([len(s) for s in self.labels] + [7])
        head = f"{'feature':<{width}}  {'importance':>11}  {'std':>9}"
        if self.thresholds is not None:
            for k in range(self.thresholds.numel()):
                head += f"  {'tw[' + str(k) + ']':>11}"
        lines = [f"base CRPS {float(self.base_crps):.6f} over {int(self.valid)} rows", head]
        for row in self.rows():
            line = f"{row[0]:<{width}}  {row[1]:>+11.5f}  {row[2]:>9.5f}"
            for v in row[3:]:
                line += f"  {v:>+11.5f}"
            lines.append(line)
        return "\n".join(lines)

    def csv(self) -> str:
        head = ["feature", "columns", "importance_mean", "importance_std"]
        head += [f"permuted_crps_{r}" for r in range(self.permuted_crps.size(1))]
        if self.tw_mean is not None:
            head += [f"tw_importance_mean_{k}" for k in range(self.tw_mean.size(1))]
        lines = [",".join(head)]
        for g, label in enumerate(self.labels):
            row = [label, " ".join(str(c) for c in self.groups[g]), repr(float(self.mean[g])),
                   repr(float(self.std[g]))]
            row += [repr(float(v)) for v in self.permuted_crps[g]]
            if self.tw_mean is not None:
                row += [repr(float(v)) for v in self.tw_mean[g]]
            lines.append(",".join(row))
        return "\n".join(lines) + "\n"


def _spread(v: torch.Tensor) -> torch.Tensor:
    """Sample standard deviation over dim 1 (0 for a single repeat)."""
    return v.std(dim=1) if v.size(1) > 1 else torch.zeros_like(v.select(1, 0))


@torch.no_grad()
def permutation_importance(model: torch.nn.Module, dataset: DeviceDataset, groups=None,
                           repeats: int = 5, batch_size: int = 32, seed: int = 0,
                           scheme: str = "time_station", thresholds=None, unit: str = "mm",
                           fused: bool = True, plans=None) -> FeatureImportance:
    """Permutation importance of each feature group of ``dataset`` under ``model``'s own CRPS
    (and, with ``thresholds`` in ``unit``, its twCRPS per threshold).

    The score of a variant is the sum of the per-row scores over all valid rows of the dataset
    divided by their number.  Variants are walked base first, then (group, repeat) in order, the
    batches of each in dataset order (a short last batch included), so every sum has a fixed
    order.  The plan of each (group, repeat) is drawn in that order from one CPU generator seeded
    with ``seed`` (``plans``: a ``[G][R]`` nest of user :class:`PermutationPlan` instead, each
    checked on the host).

    ``fused=True`` on a HIP device: per batch one ``gine_batch_fill_permuted`` launch into the
    inputs of the model's captured forward, one replay, the score kernels on the static output,
    fp64 adds into device accumulators; one readback at the end.  ``fused=False``, and any other
    device: the torch fill and ``model.eval()(batch)``."""
    from .forecast import Forecast
    from .inference import predictor_for
    if repeats < 1:
        raise ValueError("repeats must be at least 1")
    if scheme not in SCHEMES:
        raise ValueError(f"scheme must be one of {SCHEMES}, got {scheme!r}")
    dev = dataset.device
    T, N, F = dataset.x.shape
    labels, cols = resolve_groups(groups, F)
    G, R = len(cols), int(repeats)
    if plans is None:
        gen = torch.Generator()
        gen.manual_seed(seed)
        plans = [[PermutationPlan.draw(T, N, gen, scheme) for _ in range(R)] for _ in range(G)]
    elif len(plans) != G or any(len(p) != R for p in plans):
        raise ValueError(f"plans must be a [{G}][{R}] nest of PermutationPlan")
    for row in plans:
        for p in row:
            p.check(T, N)
    model.eval()
    fused = bool(fused) and dev.type == "cuda"
    K = 0
    tw_points = None
    if thresholds is not None:
        # model-space thresholds on the device, once: the score calls then copy nothing
        tw_points = Forecast.from_model(model, torch.zeros(0, _pred_width(model), device=dev)
                                        )._thresholds(thresholds, unit)
        K = tw_points.numel()
    V = 1 + G * R
    acc = torch.zeros(V, 2 + K, dtype=torch.float64, device=dev)  # crps sum | valid | tw sums
    starts = list(range(0, T, batch_size))
    all_idx = torch.arange(T, device=dev)
    bound = {}  # batch length -> (handle or static GraphBatch, y buffer)

    def binding(B: int):
        hit = bound.get(B)
        if hit is None:
            tmpl = dataset.batch(all_idx[:B])
            fwd = predictor_for(model).bind(tmpl) if fused else tmpl
            hit = bound[B] = (fwd, torch.empty_like(tmpl.y))
        return hit

    for v in range(V):
        g, r = divmod(v - 1, R) if v else (None, None)
        plan = plans[g][r].on(dataset) if v else None
        vcols = cols[g] if v else []
        for s in starts:
            idx = all_idx[s:s + batch_size]
            fwd, ybuf = binding(idx.numel())
            if fused:
                fill_batch(dataset, idx, plan, vcols, out=(fwd.x, fwd.ensemble, ybuf))
                pred = fwd.run()
            else:
                fill_batch(dataset, idx, plan, vcols, out=(fwd.x, fwd.ensemble, ybuf),
                           kernel=False)
                pred = model(fwd)
            fc = Forecast.from_model(model, pred)
            sc = fc.score(ybuf)
            acc[v, 0:1] += torch.nansum(sc.crps_rows).reshape(1)
            acc[v, 1:2] += sc.valid
            if K:
                tw = fc.twcrps(ybuf, tw_points, rows=True)
                acc[v, 2:] += torch.nansum(tw.rows, dim=0)
    host = acc.cpu()  # the one readback
    count = host[:, 1]
    crps = host[:, 0] / count
    perm = crps[1:].reshape(G, R)
    imp = perm / crps[0] - 1.0
    res = FeatureImportance(cols, labels, crps[0], perm, imp, imp.mean(1), _spread(imp), count[0])
    if K:
        tw = host[:, 2:] / count.unsqueeze(1)
        res.thresholds = tw_points.cpu()
        res.base_twcrps = tw[0]
        res.permuted_twcrps = tw[1:].reshape(G, R, K)
        res.tw_importance = res.permuted_twcrps / tw[0] - 1.0
        res.tw_mean = res.tw_importance.mean(1)
        res.tw_std = _spread(res.tw_importance)
    return res


def _pred_width(model) -> int:
    if model.loss == "NormalCRPS":
        return 2
    if model.loss == "MixedNormalCRPS":
        return 3
    return 5 if getattr(model, "grad_u", "False") == "True" else 4


# ------------------------------------------------------------------------------------------
# command line (synthetic station data: the EUPPBench ETL is out of scope)
# ------------------------------------------------------------------------------------------
def _parse_groups(tokens):
    if not tokens:
        return None
    out = []
    for tok in tokens:
        members = [int(c) if c.lstrip("-").isdigit() else c for c in tok.split(",") if c]
        out.append(members[0] if len(members) == 1 else members)
    return out


def main(argv=None) -> FeatureImportance:
    from .data import synthetic_samples
    from .models import gnn_from_params
    from .params import load_params

    ap = argparse.ArgumentParser(description="Permutation feature importance of a trained GNN.")
    ap.add_argument("--dir", required=True, help="run directory with params.json")
    ap.add_argument("--ckpt", required=True, help="state_dict checkpoint to score")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--groups", nargs="*", default=None,
                    help="feature groups: a column index or name each, commas join the columns "
                         "of one group (default: one group per column)")
    ap.add_argument("--thresholds-mm", type=float, nargs="*", default=None,
                    help="also the twCRPS importance above these thresholds")
    ap.add_argument("--scheme", choices=SCHEMES, default="time_station")
    ap.add_argument("--batch-size", type=int, default=None, help="default: params.json's")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--stations", type=int, default=122, help="synthetic station count")
    ap.add_argument("--samples", type=int, default=64, help="synthetic samples (times)")
    ap.add_argument("--k", type=int, default=10, help="k-NN graph")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--torch-loop", action="store_true",
                    help="the torch fill and model.eval() instead of the fused loop")
    args = ap.parse_args(argv)

    config = load_params(os.path.join(args.dir, "params.json"))
    os.makedirs(os.path.join(args.dir, "results"), exist_ok=True)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s",
                        handlers=[logging.StreamHandler(sys.stdout)])
    device = torch.device(args.device)
    samples = synthetic_samples(args.stations, args.samples, k=args.k, seed=args.seed)
    dataset = DeviceDataset(samples, device)
    model = gnn_from_params(config, in_channels=samples[0].x.size(1)).to(device)
    model.load_state_dict(torch.load(args.ckpt, map_location=device, weights_only=True))
    res = permutation_importance(
        model, dataset, groups=_parse_groups(args.groups), repeats=args.repeats,
        batch_size=args.batch_size or config["batch_size"], seed=args.seed, scheme=args.scheme,
        thresholds=args.thresholds_mm or None, fused=not args.torch_loop)
    path = os.path.join(args.dir, "results", "importance.csv")
    with open(path, "w") as f:
        f.write(res.csv())
    log.info("permutation importance (%s, %d repeats)\n%s", args.scheme, args.repeats,
             res.table())
    log.info("wrote %s", path)
    return res


if __name__ == "__main__":
    main()
