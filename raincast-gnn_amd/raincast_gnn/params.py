"""Experiment configurations.

``load_params`` reads a reference ``params.json`` as-is (train.py:127-134); the twelve
shipped configurations (trained_models/{24,72,120}h_{normal,normal_mixed,mixed,mixed_u}/
params.json) share every key except ``loss``, ``grad_u`` and ``max_dist``, which
:data:`EXPERIMENTS` records.  :data:`BENCH_CONFIGS` are the benchmark shapes of
BASELINE.json / SURVEY.md section 8.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, replace

_COMMON = {"batch_size": 8, "gnn_hidden": 128, "gnn_layers": 4, "heads": 8, "lr": 0.0001,
           "max_dist": 100, "max_epochs": 20, "u": 1.71, "xi": 0.5}

_VARIANTS = {
    "normal": {"loss": "NormalCRPS", "grad_u": "False"},
    "normal_mixed": {"loss": "MixedNormalCRPS", "grad_u": "False"},
    "mixed": {"loss": "MixedLoss", "grad_u": "False"},
    "mixed_u": {"loss": "MixedLoss", "grad_u": "True"},
}

EXPERIMENTS: dict[str, dict] = {}
for _lt in ("24h", "72h", "120h"):
    for _name, _v in _VARIANTS.items():
        cfg = dict(_COMMON, **_v)
        if _lt == "24h" and _name == "normal_mixed":
            cfg["max_dist"] = 1  # trained_models/24h_normal_mixed/params.json:6
        EXPERIMENTS[f"{_lt}_{_name}"] = cfg


_SCHEDULE_KEYS = {"kind", "warmup_steps", "total_steps", "min_lr_ratio"}
_SCHEDULE_KINDS = ("constant", "cosine", "linear")


def check_optimizer_keys(params: dict) -> None:
    """The two optional keys this package adds to a ``params.json`` (none of the reference's
    files has them): ``max_grad_norm`` (a positive number) and ``lr_schedule`` (``{"kind",
    "warmup_steps", "total_steps", "min_lr_ratio"}``, only ``kind`` required;
    ``total_steps`` defaults to ``max_epochs`` x the number of training batches)."""
    if "max_grad_norm" in params:
        v = params["max_grad_norm"]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
            raise ValueError(f"params.json max_grad_norm={v!r}: expected a positive number")
    if "lr_schedule" in params:
        s = params["lr_schedule"]
        if not isinstance(s, dict) or not set(s) <= _SCHEDULE_KEYS or "kind" not in s:
            raise ValueError(f"params.json lr_schedule={s!r}: expected an object with 'kind' "
                             f"and any of {sorted(_SCHEDULE_KEYS - {'kind'})}")
        if s["kind"] not in _SCHEDULE_KINDS:
            raise ValueError(f"params.json lr_schedule kind {s['kind']!r}: expected one of "
                             f"{_SCHEDULE_KINDS}")
        for k in ("warmup_steps", "total_steps", "min_lr_ratio"):
            if k in s and (isinstance(s[k], bool) or not isinstance(s[k], (int, float))
                           or s[k] < 0):
                raise ValueError(f"params.json lr_schedule {k}={s[k]!r}: expected a number >= 0")


def tw_from_params(params: dict):
    """The optional threshold-weighted loss term of a ``params.json``: ``tw_threshold_mm`` (a
    threshold in millimetres, > -0.01) and ``tw_weight`` (in [0, 1]) -> ``(tw_threshold,
    tw_weight)`` with the threshold in model space ``log(mm + 0.01)``; ``(None, 0.0)`` when the
    keys are absent (none of the reference's files has them)."""
    mm, w = params.get("tw_threshold_mm"), params.get("tw_weight", 0.0)
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w <= 1.0:
        raise ValueError(f"params.json tw_weight={w!r}: expected a number in [0, 1]")
    if mm is None:
        if w != 0.0:
            raise ValueError("params.json has tw_weight but no tw_threshold_mm")
        return None, 0.0
    if isinstance(mm, bool) or not isinstance(mm, (int, float)) or not mm > -0.01 \
            or mm == float("inf"):
        raise ValueError(f"params.json tw_threshold_mm={mm!r}: expected a finite number > -0.01")
    return math.log(mm + 0.01), float(w)


def load_params(path: str) -> dict:
    with open(path) as f:
        params = json.load(f)
    check_optimizer_keys(params)
    tw_from_params(params)
    return params


@dataclass(frozen=True)
class BenchConfig:
    name: str
    experiment: str
    num_stations: int
    k: int
    graphs_per_gpu: int
    gnn_layers: int | None = None   # override of params.json
    note: str = ""
    gnn_hidden: int | None = None   # override of params.json (the D=64 sweep, BASELINE.md:47)

    def params(self) -> dict:
        p = dict(EXPERIMENTS[self.experiment])
        if self.gnn_layers is not None:
            p["gnn_layers"] = self.gnn_layers
        if self.gnn_hidden is not None:
            p["gnn_hidden"] = self.gnn_hidden
        return p

    def with_hidden(self, hidden: int | None) -> "BenchConfig":
        """This configuration at hidden size ``hidden`` (None or params.json's own value:
        unchanged); the name records the sweep point, e.g. ``cfg2-D64``."""
        if hidden is None or hidden == EXPERIMENTS[self.experiment]["gnn_hidden"]:
            return self
        return replace(self, gnn_hidden=int(hidden), name=f"{self.name}-D{int(hidden)}")


BENCH_CONFIGS = {
    1: BenchConfig("cfg1", "24h_mixed", 500, 10, 1, note="CPU-runnable reference case"),
    2: BenchConfig("cfg2", "24h_mixed", 500, 10, 32, note="headline single-GPU workload"),
    3: BenchConfig("cfg3", "72h_mixed_u", 2000, 16, 64, note="HBM-bound roofline run"),
    4: BenchConfig("cfg4", "24h_mixed", 500, 10, 256, note="global batch 256, strong scaling"),
    5: BenchConfig("cfg5", "120h_normal_mixed", 10000, 32, 8, gnn_layers=3,
                   note="10k-station dense graph, 3 GINE layers"),
}
