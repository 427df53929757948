"""Microbenchmark of the threshold-weighted CRPS kernels at cfg2's row count: the two score
kernels (csrc/gine_forecast.hip: gine_forecast_twcrps, gine_ensemble_twcrps) at T = 1 and 8
thresholds, and the loss pass (csrc/gine_loss.hip: gine_crps_tw_fwd_grad) beside the plain
gine_crps_fwd_grad on the same inputs.

Shapes: N = 16,000 rows, MIXED kind (u = 1.71, xi = 0.5), M = 11 members, about half the targets
and members at c and 5 % NaN.  Each variant is --reps calls captured into one HIP graph and
replayed, timed with device events around the replay (device time alone; the variants alternate
inside one run, --rounds times each; median and range over the rounds).  The ensemble rows time
the kernel's launch alone (the means of RawEnsemble.twcrps are torch reductions of its rows, as
those of RawEnsemble.score are); the forecast rows time Forecast.twcrps, which is one launch and a
memset.  Bytes are what the
shapes say a call has to move at least (inputs read once, outputs written once).
    python tools/twcrps_micro.py [--reps 20 --rounds 9 --out profiles/twcrps_micro_cfg2.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from ensemble_micro import capture, make_case, timed_us  # noqa: E402
from raincast_gnn import _lib  # noqa: E402
from raincast_gnn import loss as L  # noqa: E402

TW_T, TW_W = 1.0, 0.5


def loss_pass(pred, y, tw):
    """One forward-with-gradient pass of the fused loss on pred [N, 4] (needs a gradient)."""
    p = pred.detach().requires_grad_(True)
    if tw:
        return lambda: L._fused_tw(p, y, _lib.LOSS_MIXED, TW_T, TW_W, u=1.71, xi=0.5)
    return lambda: L._fused(p, y, _lib.LOSS_MIXED, u=1.71, xi=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rows", type=int, default=16000)
    ap.add_argument("--members", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twcrps_micro_cfg2.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("twcrps_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be N={args.rows}, M={args.members})")
    dev = torch.device("cuda:0")
    N, M = args.rows, args.members
    raw, fc, y, _ = make_case(N, M, dev)
    K = fc.pred.size(1)
    lines = [f"# N={N} kind=mixed M={M} tw_threshold={TW_T} tw_weight={TW_W} reps={args.reps} "
             f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    table, nbytes = {}, {}
    for T in (1, 8):
        x = torch.linspace(-1.0, 4.0, T, dtype=torch.float64, device=dev) if T > 1 else \
            torch.tensor([TW_T], dtype=torch.float64, device=dev)
        table[f"forecast_twcrps T={T}"] = lambda x=x: fc.twcrps(y, x, rows=True)
        nbytes[f"forecast_twcrps T={T}"] = N * (4 * K + 4) + 8 * T + 8 * N * T + 8 * (T + 1)
        table[f"ensemble_twcrps T={T}"] = lambda x=x: raw._twcrps_hip(y, x)  # the launch alone
        nbytes[f"ensemble_twcrps T={T}"] = N * (4 * M + 4) + 8 * T + 2 * 8 * N * T
    table["loss plain (gine_crps_fwd_grad)"] = loss_pass(fc.pred, y, False)
    table["loss tw (gine_crps_tw_fwd_grad)"] = loss_pass(fc.pred, y, True)
    for k in ("loss plain (gine_crps_fwd_grad)", "loss tw (gine_crps_tw_fwd_grad)"):
        # pred, y, count parts in; dpred fp64, grad_unit fp32, partials out
        nbytes[k] = N * (4 * K + 4) + 4 * 64 + N * K * (8 + 4) + 16 * ((N + 63) // 64)
    graphs = {k: capture(fn, args.reps) for k, fn in table.items()}
    times = {k: [] for k in table}
    for _ in range(args.rounds):  # alternate the variants inside one run
        for k in table:
            times[k].append(timed_us(graphs[k].replay, args.reps))
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        lines.append(json.dumps({"variant": k, "us_median": round(med[k], 2),
                                 "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                                 "bytes": nbytes[k],
                                 "GB_per_s": round(nbytes[k] / med[k] / 1e3, 1)}))
        print(lines[-1], flush=True)
    ratio = med["loss tw (gine_crps_tw_fwd_grad)"] / med["loss plain (gine_crps_fwd_grad)"]
    lines.append(json.dumps({"tw_loss_pass_over_plain": round(ratio, 2)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
