"""Microbenchmark of the pool kernels (csrc/gine_pool.hip) at a season of station days:
N = 89,060 rows (122 stations x 730 days), M in {5, 10} checkpoints, T = 4 thresholds / levels,
MIXED kind (u = 1.71, xi = 0.5).

Per M: gine_pool_prob (exceedance), gine_pool_quantile (T levels in the body), gine_pool_score,
each --reps calls captured into one HIP graph and replayed, timed with device events around
the replay (median and range over --rounds, the variants alternating inside one run); beside
them the package's fp64 torch formulation of the same three on the same device (eager, event
timed, --torch-runs calls) and M calls of Forecast.score (gine_forecast_score), the closed-form
part of the pool's CRPS alone.  The rule's cost is reported as member-distribution evaluations
(one erfc or one pow each) per row: 2 M per node of a non-empty panel, counted on the host from
the rows' breakpoints.
    python tools/pool_micro.py [--reps 3 --rounds 5 --out profiles/pool_micro.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ensemble_micro import capture, timed_us  # noqa: E402
from raincast_gnn.forecast import C_DEFAULT  # noqa: E402
from raincast_gnn.pool import BREAK_K, GJ_NODES, GL_NODES, ForecastPool  # noqa: E402

U, XI = 1.71, 0.5


def make_members(N, M, seed=0):
    """[M, N, 4] float32: one base forecast per row and M checkpoints scattered around it (the
    spread of a deep ensemble: a few tenths of sigma)."""
    r = np.random.default_rng(seed)
    sp = lambda v: np.log1p(np.exp(v)) + 1e-6  # noqa: E731
    base = [r.normal(-1.0, 2.0, N), r.normal(0, 1, N), r.normal(0, 1, N), r.normal(0, 1, N)]
    out = np.empty((M, N, 4), dtype=np.float32)
    for m in range(M):
        d = [b + 0.3 * r.normal(0, 1, N) for b in base]
        out[m] = np.stack([d[0], sp(d[1]), 1 / (1 + np.exp(-d[2])), sp(d[3])], 1)
    return out


def evaluations_per_row(params):
    """Mean member-distribution evaluations per row of the diversity rule."""
    M, N, _ = params.shape
    P = params.astype(np.float64)
    bp = (P[:, :, 0:1] + np.array(BREAK_K) * P[:, :, 1:2]).transpose(1, 0, 2).reshape(N, -1)
    bp = np.concatenate([bp, np.full((N, 1), U), np.full((N, 1), C_DEFAULT)], 1)
    bp = np.sort(np.clip(bp, C_DEFAULT, U), 1)
    panels = (np.diff(bp, axis=1) > 0).sum(1)
    return float((2 * M * (GL_NODES * panels + GJ_NODES)).mean()), float(panels.mean())


def eager_us(fn, runs):
    fn()
    torch.cuda.synchronize()
    return statistics.median(timed_us(fn, 1) for _ in range(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--rows", type=int, default=122 * 730)
    ap.add_argument("--members", type=int, nargs="*", default=[5, 10])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be N={args.rows}, M={args.members})")
    dev = torch.device("cuda:0")
    N, T = args.rows, 4
    lines = [f"# N={N} kind=mixed u={U} xi={XI} T={T} reps={args.reps} rounds={args.rounds} "
             f"device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    r = np.random.default_rng(1)
    y = np.where(r.random(N) < 0.5, np.float32(C_DEFAULT), r.normal(0.5, 1.5, N)).astype(np.float32)
    y[r.random(N) < 0.05] = np.nan
    y = torch.from_numpy(y).to(dev)
    x = torch.tensor([C_DEFAULT, 0.0, 1.0, 2.5], dtype=torch.float64, device=dev)
    q = torch.tensor([0.5, 0.9, 0.99, 0.999], dtype=torch.float64, device=dev)
    for M in args.members:
        params = make_members(N, M)
        evals, panels = evaluations_per_row(params)
        pool = ForecastPool(torch.from_numpy(params).to(dev), "mixed", u=U, xi=XI)
        table = {"pool_prob": lambda: pool.exceedance(x),
                 "pool_quantile": lambda: pool.quantile(q),
                 "pool_score": lambda: pool.score(y, x),
                 "M x forecast_score": lambda: [f.score(y, x) for f in pool.members()]}
        graphs = {k: capture(fn, args.reps) for k, fn in table.items()}
        times = {k: [] for k in table}
        for _ in range(args.rounds):
            for k in table:
                times[k].append(timed_us(graphs[k].replay, args.reps))
        for k, ts in times.items():
            lines.append(json.dumps({"M": M, "variant": k,
                                     "us_median": round(statistics.median(ts), 1),
                                     "us_min": round(min(ts), 1), "us_max": round(max(ts), 1)}))
            print(lines[-1], flush=True)
        torch_table = {"torch prob": lambda: pool._prob_torch(x.reshape(1, -1), True),
                       "torch quantile": lambda: pool._quantile_torch(q, False),
                       "torch score": lambda: pool._score_torch(y, x)}
        for k, fn in torch_table.items():
            lines.append(json.dumps({"M": M, "variant": k,
                                     "us_median": round(eager_us(fn, args.torch_runs), 1)}))
            print(lines[-1], flush=True)
        a, b = pool.score(y, x), pool._score_torch(y, x)
        ok = ~torch.isnan(y)
        scale = b.crps_rows[ok].abs().max()
        lines.append(json.dumps({
            "M": M, "evaluations_per_row": round(evals, 1), "nonempty_panels_per_row":
            round(panels, 1), "kernel_vs_torch_crps_of_scale":
            float(((a.crps_rows - b.crps_rows)[ok].abs().max() / scale).item()),
            "mean_crps": float(a.crps.item()),
            "mean_member_crps": float((torch.nansum(a.member_crps_rows) / a.valid[0]).item()),
            "mean_diversity": float((a.diversity_rows[ok].sum() / a.valid[0]).item())}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
