"""Microbenchmark of the field-score kernels (csrc/gine_field.hip: gine_field_energy,
gine_field_variogram, gine_field_area) against the fp64 torch formulation of the same
definitions (raincast_gnn/fields.py: per graph, the variogram in row chunks) on the same device.

Shapes: 32 graphs x 500 stations and 16 graphs x 2,000 stations, M = 51 and M = 11 fp32 members,
about half of the values tied at c; per graph each member is patchy w.p. 0.1 (NaN at 40 % of
the rows, so it leaves that graph's member set) and 5 % of the targets are NaN; p = 0.5, area
maximum.  Each variant produces the same [G] outputs.

Two timings per kernel variant, both with device events around work that ends in a synchronise:
  graph  --reps calls captured into one HIP graph and replayed: device time alone, no host
  eager  --reps calls issued from Python: what a caller pays, launch overhead included
The torch formulation loops over the graphs on the host and reads sizes back, so it cannot be
captured: eager only, --torch-reps calls per sample.  The variants alternate inside one run,
--rounds times each; rows show the median and the range over the rounds, and the ratio
torch / kernel of the eager medians.
    python tools/field_micro.py [--reps 5 --rounds 5 --out profiles/field_micro.txt]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from raincast_gnn.fields import MemberFields  # noqa: E402

C = math.log(0.01)
SHAPES = [(32, 500), (16, 2000)]
P, STAT = 0.5, "max"


def make_case(G, n, M, dev):
    r = np.random.default_rng(1000 * G + M)
    N = G * n
    rain = np.where(r.random((N, M)) < 0.5, 0.0, r.gamma(0.7, 6.0, (N, M)))
    x = np.log(rain + 0.01).astype(np.float32)
    for g in range(G):
        patchy = r.random(M) < 0.1
        x[g * n:(g + 1) * n][(r.random((n, M)) < 0.4) & patchy] = np.nan
    y = np.where(r.random(N) < 0.5, np.float32(C), r.normal(0.5, 1.5, N)).astype(np.float32)
    y[r.random(N) < 0.05] = np.nan
    ptr = torch.arange(0, N + 1, n, dtype=torch.int64, device=dev)
    return MemberFields(torch.from_numpy(x).to(dev), ptr), torch.from_numpy(y).to(dev)


def variants(mf, y):
    yt = mf._targets(y)
    return {
        "energy kernel": lambda: mf.energy(y),
        "energy torch": lambda: mf._torch(yt, P, STAT, ("energy",)),
        "variogram kernel": lambda: mf.variogram(y, P),
        "variogram torch": lambda: mf._torch(yt, P, STAT, ("variogram",)),
        "area kernel": lambda: mf.area(y, STAT),
        "area torch": lambda: mf._torch(yt, P, STAT, ("area",)),
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


def agree(table):
    """The two sides of each pair agree before anything is timed."""
    es_k, vs_k, ar_k = (table[f"{w} kernel"]() for w in ("energy", "variogram", "area"))
    es_t, vs_t, ar_t = (table[f"{w} torch"]() for w in ("energy", "variogram", "area"))
    for a, b in ((es_k[0], es_t["es"]), (vs_k[0], vs_t["vs"]), (ar_k.crps, ar_t["crps"])):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and not torch.isnan(a).all()
        assert (torch.nan_to_num(a - b).abs() <= 1e-10 * torch.nan_to_num(a).abs()).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--members", type=int, nargs="*", default=[51, 11])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be {SHAPES}, M={args.members})")
    dev = torch.device("cuda:0")
    lines = [f"# p={P} stat={STAT} reps={args.reps} torch_reps={args.torch_reps} "
             f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    for G, n in SHAPES:
        for M in args.members:
            mf, y = make_case(G, n, M, dev)
            table = variants(mf, y)
            agree(table)
            tag = {"G": G, "n": n, "M": M}
            graphs = {k: capture(fn, args.reps) for k, fn in table.items() if "kernel" in k}
            times = {}
            for _ in range(args.rounds):  # alternate the variants inside one run
                for k, fn in table.items():
                    reps = args.reps if "kernel" in k else args.torch_reps
                    if k in graphs:
                        times.setdefault((k, "graph"), []).append(
                            timed_us(graphs[k].replay, args.reps))
                    times.setdefault((k, "eager"), []).append(
                        timed_us(lambda: [fn() for _ in range(reps)], reps))
            med = {}
            for (k, mode), ts in times.items():
                med[k, mode] = statistics.median(ts)
                lines.append(json.dumps({**tag, "variant": k, "mode": mode,
                                         "us_median": round(med[k, mode], 1),
                                         "us_min": round(min(ts), 1),
                                         "us_max": round(max(ts), 1)}))
                print(lines[-1], flush=True)
            for what in ("energy", "variogram", "area"):
                a, b = med[f"{what} kernel", "eager"], med[f"{what} torch", "eager"]
                lines.append(json.dumps({**tag, "what": what, "mode": "eager",
                                         "torch_over_kernel": round(b / a, 1)}))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
