"""Microbenchmark of the raw-ensemble kernels (csrc/gine_forecast.hip: gine_ensemble_score,
gine_ensemble_ecc) against the fp64 torch formulation of the same definitions
(raincast_gnn/ensemble.py: torch.sort, scatter, elementwise passes) on the same device.

Shapes: N = 16,000 rows (cfg2) with M = 51 (forecasts) and M = 11 (reforecasts) members, about
half of them tied at c and 5 % NaN; MIXED kind (u = 1.71, xi = 0.5); 3 thresholds.  Each
variant produces the same outputs: score = the five row outputs and prob [N, 3]; ecc = the
[N, M] members at the uniform levels.

Two timings per variant, both with device events around work that ends in a synchronise:
  graph  --reps calls captured into one HIP graph and replayed: device time alone, no host
  eager  --reps calls issued from Python: what a caller pays, launch overhead included
The variants alternate inside one run, --rounds times each; rows show the median and the range
over the rounds, and the ratio torch / kernel of the medians.
    python tools/ensemble_micro.py [--reps 20 --rounds 9 --out profiles/ensemble_micro.txt]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd")]

import torch  # noqa: E402

from raincast_gnn.ensemble import RawEnsemble, ecc  # noqa: E402
from raincast_gnn.forecast import Forecast  # noqa: E402

C = math.log(0.01)
THRESHOLDS = [C, math.log(1.01), math.log(10.01)]


def make_case(n, M, dev):
    torch.manual_seed(1000 + M)  # the Gamma draw reads the global generator
    gen = torch.Generator().manual_seed(1000 + M)
    rain = torch.where(torch.rand(n, M, generator=gen) < 0.5, torch.zeros(n, M),
                       torch.distributions.Gamma(0.7, 1 / 6.0).sample((n, M)))
    mem = torch.log(rain + 0.01).float()
    mem[torch.rand(n, M, generator=gen) < 0.05] = float("nan")
    y = torch.where(torch.rand(n, generator=gen) < 0.5, torch.full((n,), C),
                    torch.randn(n, generator=gen) * 1.5 + 0.5).float()
    pred = torch.stack([torch.randn(n, generator=gen) * 2 - 1,
                        torch.nn.functional.softplus(torch.randn(n, generator=gen)) + 1e-6,
                        torch.sigmoid(torch.randn(n, generator=gen)),
                        torch.nn.functional.softplus(torch.randn(n, generator=gen)) + 1e-6], 1)
    raw = RawEnsemble(mem.to(dev))
    fc = Forecast(pred.float().to(dev), "mixed", u=1.71, xi=0.5)
    x = torch.tensor(THRESHOLDS, dtype=torch.float64, device=dev)
    return raw, fc, y.to(dev), x


def variants(raw, fc, y, x):
    return {
        "score kernel": lambda: raw._score_hip(y, x),
        "score torch": lambda: raw._score_torch(y, x),
        "ecc kernel": lambda: ecc(fc, raw),
        "ecc torch": lambda: fc._quantile_cpu(raw._levels_torch("uniform"), False),
    }


def capture(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def timed_us(run, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rows", type=int, default=16000)
    ap.add_argument("--members", type=int, nargs="*", default=[51, 11])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be N={args.rows}, M={args.members})")
    dev = torch.device("cuda:0")
    lines = [f"# N={args.rows} kind=mixed thresholds={len(THRESHOLDS)} reps={args.reps} "
             f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    for M in args.members:
        raw, fc, y, x = make_case(args.rows, M, dev)
        table = variants(raw, fc, y, x)
        # the two sides of each pair agree before anything is timed
        rk, pk = table["score kernel"]()
        rt, pt = table["score torch"]()
        assert torch.equal(torch.nan_to_num(pk, nan=-1.0), torch.nan_to_num(pt, nan=-1.0))
        assert (torch.nan_to_num(rk - rt).abs().max() <= 1e-12)
        graphs = {}
        for k, fn in table.items():
            try:
                graphs[k] = capture(fn, args.reps)
            except RuntimeError as err:  # an op that a capture cannot record
                graphs[k] = None
                lines.append(f"# M={M} {k}: not captured ({str(err).splitlines()[0][:80]})")
                torch.cuda.synchronize()
        times = {(k, mode): [] for k in table for mode in ("graph", "eager")}
        for _ in range(args.rounds):  # alternate the variants inside one run
            for k, fn in table.items():
                if graphs[k] is not None:
                    times[k, "graph"].append(timed_us(graphs[k].replay, args.reps))
                times[k, "eager"].append(
                    timed_us(lambda: [fn() for _ in range(args.reps)], args.reps))
        med = {}
        for (k, mode), ts in times.items():
            if not ts:
                continue
            med[k, mode] = statistics.median(ts)
            lines.append(json.dumps({"M": M, "variant": k, "mode": mode,
                                     "us_median": round(med[k, mode], 2),
                                     "us_min": round(min(ts), 2), "us_max": round(max(ts), 2)}))
            print(lines[-1], flush=True)
        for what in ("score", "ecc"):
            for mode in ("graph", "eager"):
                a, b = med.get((f"{what} kernel", mode)), med.get((f"{what} torch", mode))
                if a and b:
                    lines.append(json.dumps({"M": M, "what": what, "mode": mode,
                                             "torch_over_kernel": round(b / a, 2)}))
                    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
