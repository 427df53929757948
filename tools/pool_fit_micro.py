"""Microbenchmark of gine_pool_pairs (csrc/gine_pool.hip) at a season of station
days: N = 89,060 rows (122 stations x 730 days), M in {5, 10} checkpoints, MIXED kind (u = 1.71,
xi = 0.5), 5 folds; members and targets as tools/pool_micro.py.

Per M, each --reps calls captured into one HIP graph and replayed, timed with device events
around the replay (median and range over --rounds, the variants alternating inside one run):
  pool_pairs            one gine_pool_pairs launch (5 segments)
  pairwise pool_score   (a) M (M - 1) / 2 two-member gine_pool_score calls: the only route to D
                        without the kernel
  pool_score            (b) one gine_pool_score call at the same M: the floor in member
                        evaluations
beside them (c) the torch formulation of pair_sums on the same device (eager, event timed,
--torch-runs calls) and the host time of solve_pool_weights on the kernel's sums (median of 20
calls, time.perf_counter).
    python tools/pool_fit_micro.py [--reps 3 --rounds 5 --out profiles/pool_fit_micro.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ensemble_micro import capture, timed_us  # noqa: E402
from pool_micro import U, XI, eager_us, make_members  # noqa: E402
from raincast_gnn.forecast import C_DEFAULT  # noqa: E402
from raincast_gnn.pool import ForecastPool, solve_pool_weights  # noqa: E402

FOLDS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--rows", type=int, default=122 * 730)
    ap.add_argument("--members", type=int, nargs="*", default=[5, 10])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_fit_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_fit_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be N={args.rows}, M={args.members})")
    dev = torch.device("cuda:0")
    N = args.rows
    lines = [f"# N={N} kind=mixed u={U} xi={XI} folds={FOLDS} reps={args.reps} "
             f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    r = np.random.default_rng(1)
    y = np.where(r.random(N) < 0.5, np.float32(C_DEFAULT), r.normal(0.5, 1.5, N)).astype(np.float32)
    y[r.random(N) < 0.05] = np.nan
    y = torch.from_numpy(y).to(dev)
    none = torch.zeros(0, dtype=torch.float64, device=dev)
    for M in args.members:
        params = torch.from_numpy(make_members(N, M)).to(dev)
        pool = ForecastPool(params, "mixed", u=U, xi=XI)
        ptr = pool._segments(FOLDS)
        ptr_dev = torch.from_numpy(ptr).to(dev)
        two = [ForecastPool(params[[m, l]], "mixed", u=U, xi=XI)
               for m in range(M) for l in range(m + 1, M)]
        table = {"pool_pairs": lambda: pool._pairs_hip(y, ptr_dev),
                 "pairwise pool_score": lambda: [p.score(y, none) for p in two],
                 "pool_score": lambda: pool.score(y, none)}
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
        lines.append(json.dumps({"M": M, "variant": "torch pair_sums", "us_median": round(
            eager_us(lambda: pool._pairs_torch(y, ptr), args.torch_runs), 1)}))
        print(lines[-1], flush=True)
        count, cbar, dist = pool._pairs_hip(y, ptr_dev)
        tc, tb, td = pool._pairs_torch(y, ptr)
        ps = pool.pair_sums(y, FOLDS)
        c, D = ps.member_crps.sum(0).cpu().numpy(), ps.distance.sum(0).cpu().numpy()
        host = []
        for _ in range(20):
            t0 = time.perf_counter()
            w, info = solve_pool_weights(c, D)
            host.append((time.perf_counter() - t0) * 1e6)
        fit = pool.fit_weights(y, FOLDS)
        lines.append(json.dumps({
            "M": M, "host_solve_us_median": round(statistics.median(host), 1),
            "solver_steps": info["iterations"], "solver_gap_of_max_c":
            float(info["gap"] / np.abs(c).max()), "support": info["support"],
            "kernel_vs_torch_distance_of_largest": float(((dist - td).abs().max()
                                                          / td.abs().max()).item()),
            "kernel_vs_torch_member_crps_of_largest": float(((cbar - tb).abs().max()
                                                             / tb.abs().max()).item()),
            "count_equal": bool(torch.equal(count, tc)), "crps": fit.crps,
            "crps_equal": fit.crps_equal, "cv_crps": fit.cv_crps,
            "cv_crps_equal": fit.cv_crps_equal,
            "weights": [round(float(v), 6) for v in fit.weights]}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
