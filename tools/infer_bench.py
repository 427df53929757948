"""Eval-mode forward of the station-graph GNN, timed three ways on one device in one session.

    python tools/infer_bench.py [--config 2] [--rounds 12] [--chunk 25] [--settle 100]
                                [--stations S --max-dist KM] [--force-deep] [--separate]

  (a) model    ``model.eval()(batch)`` under ``no_grad``: the path evaluate.predict_model takes
               by default (three launches per GINE layer, a head launch);
  (b) eager    ``Predictor(model, capture=False)``: one gine_mp_fwd_layer_eval launch per layer
               (gine_mp_fwd_layer_eval_deep on a graph past the degree limit), the last one
               carrying the head;
  (c) graph    ``Predictor(model, capture=True)``: (b) captured in one HIP graph and replayed
               (the copies of x and ensemble into the static inputs are inside the timing).

``--stations S --max-dist KM`` times the reference's radius graph (utils/data.py:261-284) on S
stations instead of the configuration's k-NN graph; ``--force-deep`` lifts
``inference.DEEP_MAX_NODES`` for the run, so the deep launch is timed at any N;
``--separate`` adds (d) eager_sep and (e) graph_sep, (b) and (c) with the deep launch off (the
layers on GINEConv's separate eval launches, inside the Predictor and its HIP graph).  The record
holds the graph's largest in-degree and the entry the Predictor's layers ran.

The three are checked to give the same bits first.  After ``--settle`` replays of (c) (the
clock ramp) the variants alternate: every round times one chunk of ``--chunk``
back-to-back forwards of each (host clock around a device synchronise), so drift of the box
hits all three alike.  Reported: kernel launches per forward (torch.profiler, one forward, in
a pass of its own before the timing) and p10 / p50 / p90 of the per-forward milliseconds over
the rounds; the last line is one JSON record.  Needs a HIP device: there is no CPU mode.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "raincast-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from raincast_gnn.data import relabel_stations, station_order, synthetic_batch  # noqa: E402
from raincast_gnn import _lib, inference  # noqa: E402
from raincast_gnn.graph import get_graph  # noqa: E402
from raincast_gnn.inference import Predictor  # noqa: E402
from raincast_gnn.models import gnn_from_params  # noqa: E402
from raincast_gnn.params import BENCH_CONFIGS  # noqa: E402


def count_launches(fn) -> int | None:
    """Device kernels of one call of ``fn`` (graph replays report their kernels too)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events()
                   if str(getattr(e, "device_type", "")).endswith("CUDA")
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as exc:  # the profiler is optional here; the timing is not
        print(f"launch count unavailable: {exc!r}")
        return None


def layer_entries(fn) -> dict:
    """{entry point: calls} of the GINE layers in one call of ``fn``: the one-launch entries,
    or the separate launches' message-passing entries where neither applies."""
    names, real = [], _lib.call

    def counting(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = counting
    try:
        fn()
    finally:
        _lib.call = real
    return {n: names.count(n) for n in sorted(set(names)) if n.startswith("gine_mp_fwd")}


def pct(v: list[float], q: float) -> float:
    s = sorted(v)
    return s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", type=int, default=2, choices=sorted(BENCH_CONFIGS))
    ap.add_argument("--graphs", type=int, default=None, help="graphs per batch (default: the "
                    "configuration's per-GPU count)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--chunk", type=int, default=25, help="forwards per timed chunk")
    ap.add_argument("--settle", type=int, default=100)
    ap.add_argument("--stations", type=int, default=None, help="stations per graph (default: "
                    "the configuration's)")
    ap.add_argument("--max-dist", type=float, default=None, metavar="KM", help="radius graph "
                    "with this cut-off instead of the configuration's k-NN graph")
    ap.add_argument("--force-deep", action="store_true", help="no DEEP_MAX_NODES limit")
    ap.add_argument("--separate", action="store_true", help="also time the Predictor with the "
                    "deep launch off")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/infer_bench.py needs a HIP device")
    dev = torch.device("cuda", 0)
    cfg = BENCH_CONFIGS[args.config]
    graphs = args.graphs or cfg.graphs_per_gpu
    torch.manual_seed(42)
    model = gnn_from_params(cfg.params()).to(dev)
    stations = args.stations or cfg.num_stations
    if args.force_deep:
        inference.DEEP_MAX_NODES = None
    batch = synthetic_batch(stations, graphs, k=cfg.k, seed=1000, max_dist=args.max_dist)
    graph0 = batch.edge_index[:, :batch.edge_index.size(1) // graphs]
    batch = relabel_stations(batch, station_order(graph0, stations)).to(dev)
    max_deg = get_graph(batch.edge_index, batch.edge_attr.float(), batch.x.size(0)).max_in_degree
    with torch.no_grad():  # train mode twice: running statistics off their initial values
        model.train()
        model(batch)
        model(batch)
    model.eval()
    eager = Predictor(model, capture=False)
    graph = Predictor(model, capture=True, warmup=0)

    @torch.no_grad()
    def run_model():
        return model(batch)

    variants = {"model": run_model, "eager": lambda: eager(batch), "graph": lambda: graph(batch)}
    if args.separate:
        def deep_off(pred):  # (a capture keeps the choice made while it was taken)
            def run():
                keep, inference.DEEP_MAX_NODES = inference.DEEP_MAX_NODES, 0
                try:
                    return pred(batch)
                finally:
                    inference.DEEP_MAX_NODES = keep
            return run
        variants["eager_sep"] = deep_off(Predictor(model, capture=False))
        variants["graph_sep"] = deep_off(Predictor(model, capture=True, warmup=0))
    want = run_model()
    for name, fn in variants.items():
        for _ in range(3):
            got = fn()
        assert torch.equal(got, want), f"{name}: predictions differ from model.eval()(batch)"
    torch.cuda.synchronize()
    launches = {name: count_launches(fn) for name, fn in variants.items()}
    entries = layer_entries(variants["eager"])
    for _ in range(args.settle):
        variants["graph"]()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.chunk):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.chunk)
    rec = {"tool": "infer_bench", "config": cfg.name, "graphs": graphs,
           "nodes": int(batch.x.size(0)), "device": torch.cuda.get_device_name(0),
           "stations": stations, "max_dist_km": args.max_dist,
           "max_in_degree": int(max_deg), "predictor_layer_entries": entries,
           "deep_max_nodes": inference.DEEP_MAX_NODES,
           "rounds": args.rounds, "chunk": args.chunk, "settle": args.settle, "variants": {}}
    edges = f"radius {args.max_dist:g} km" if args.max_dist is not None else f"k = {cfg.k}"
    print(f"{cfg.name}: {graphs} x {stations} stations, {edges}, max in-degree {max_deg}, "
          f"N = {batch.x.size(0)}; {args.rounds} rounds x {args.chunk} forwards, alternating")
    print(f"Predictor layers ran: {entries}")
    print(f"{'variant':<9} {'launches':>8} {'p10 ms':>9} {'p50 ms':>9} {'p90 ms':>9}")
    for name in variants:
        p10, p50, p90 = (pct(ms[name], q) for q in (0.1, 0.5, 0.9))
        rec["variants"][name] = {"launches": launches[name], "p10_ms": p10, "p50_ms": p50,
                                 "p90_ms": p90, "chunks_ms": ms[name]}
        print(f"{name:<9} {str(launches[name]):>8} {p10:>9.4f} {p50:>9.4f} {p90:>9.4f}")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
