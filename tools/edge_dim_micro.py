"""Microbenchmark of the K-wide message passing (csrc/gine_mpek.hip) against the K = 1
gather kernels, at one layer shape (default cfg2: 32 graphs x 500 stations, k = 10 plus self
loops, D = 128).

Variants, forward and backward (backward = the kernel plus its fixed-order finish launch):
  a        gine_mp_fwd / gine_mp_bwd, K = 1, fma mode (the shipped K = 1 gather kernels)
  b        gine_mp_fwd_ek / gine_mp_bwd_ek at K = 1 (what generality costs)
  c2 c4 c8 the same at K = 2, 4, 8
  d1 d4    the backward with the edge_attr gradient at K = 1 and K = 4
Every variant is captured into a HIP graph of --reps calls (no host time in the window); the
graphs are replayed in alternation, --rounds times each, timed with device events; the row
shows the median and the range over the rounds.  Bytes: what each variant must move, from
the shapes (node rows once per direction, CSR, attributes 4*K*E, 4*K*E more for d edge_attr).
    python tools/edge_dim_micro.py [--stations 500 --k 10 --graphs 32 --D 128]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from raincast_gnn import functional as Fn  # noqa: E402
from raincast_gnn import options  # noqa: E402
from raincast_gnn.graph import GineGraph  # noqa: E402
from helpers import knn_batch_graph  # noqa: E402


def capture(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def replay_us(graph, reps, inner=5):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / (inner * reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stations", type=int, default=500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_dim_micro needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    D = args.D
    options.MP_WINDOW = "0"  # the gather kernels on both sides of the comparison
    ei, ea, N = knn_batch_graph(args.stations, args.k, args.graphs, seed=0)
    E = ei.size(1)
    ei = ei.to(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, D, generator=g).to(dev)
    dz = torch.randn(N, D, generator=g).to(dev)
    eps = torch.tensor([0.1], device=dev)
    lb = torch.randn(D, generator=g).to(dev)
    cols = torch.cat([ea.reshape(-1, 1), torch.randn(E, 7, generator=g)], dim=1)

    fwd, bwd = {}, {}
    keep = []
    for name, K, eid, old in (("a", 1, False, True), ("b", 1, False, False),
                              ("c2", 2, False, False), ("c4", 4, False, False),
                              ("c8", 8, False, False), ("d1", 1, True, False),
                              ("d4", 4, True, False)):
        attr = cols[:, :K].contiguous().to(dev)
        graph = GineGraph(ei, attr, N, with_eid=eid)
        W = (torch.randn(D, K, generator=g) * 0.5).to(dev)
        keep.append((graph, W, attr))
        nb = 4 * (N * D + N + 1 + E * (1 + K) + D * (K + 1))  # one row table, CSR, attrs, lin
        if old:
            fwd[name] = (lambda gr=graph, w=W.reshape(-1): Fn.mp_forward(x, gr, w, lb, eps,
                                                                          lin_flag=0),
                         nb + 4 * N * D)
            bwd[name] = (lambda gr=graph, w=W.reshape(-1): Fn.mp_backward(dz, x, gr, w, lb, eps,
                                                                           lin_flag=0),
                         nb + 8 * N * D)
        elif not eid:
            fwd[name] = (lambda gr=graph, w=W: Fn.mp_forward(x, gr, w, lb, eps, wide=True),
                         nb + 4 * N * D)
            bwd[name] = (lambda gr=graph, w=W: Fn.mp_backward(dz, x, gr, w, lb, eps, wide=True),
                         nb + 8 * N * D)
        else:
            bwd[name] = (lambda gr=graph, w=W: Fn.mp_backward(dz, x, gr, w, lb, eps,
                                                               edge_grad=True),
                         nb + 8 * N * D + 4 * E + 4 * K * E)
    print(f"# N={N} E={E} D={D} reps={args.reps} rounds={args.rounds} "
          f"device={torch.cuda.get_device_name(0)}")
    for side, table in (("fwd", fwd), ("bwd", bwd)):
        graphs = {k: capture(fn, args.reps) for k, (fn, _) in table.items()}
        times = {k: [] for k in table}
        for _ in range(args.rounds):  # alternate the variants inside one run
            for k, gr in graphs.items():
                times[k].append(replay_us(gr, args.reps))
        for k, ts in times.items():
            med = statistics.median(ts)
            print(json.dumps({"side": side, "variant": k, "us_median": round(med, 2),
                              "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                              "bytes": table[k][1],
                              "GBps": round(table[k][1] / med / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
