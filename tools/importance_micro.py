"""Microbenchmark of the permutation-importance loop (raincast_gnn/importance.py)
at the cfg2 shape: batches of 32 samples x 500 stations, 11 members, 35 features, k = 10, out of
a device-resident dataset of --samples samples (larger than the Infinity Cache by default).

1. The fill kernel alone (gine_batch_fill_permuted): --reps launches over consecutive batches
   captured into one HIP graph and replayed, so the time is device time without the host; with
   no column, one column and all columns permuted.  Its byte floor is 2 * B*N*(M+1)*F * 4 bytes
   (every element read once and written once) over 6.3 TB/s.
2. The per-batch loop, --batches batches per sample, three forms alternating inside one run:
     fused           fill kernel into Predictor.bind's inputs, replay, score, fp64 accumulate
     torch+predictor torch fill, Predictor.__call__ (two copies, replay, clone), score, accumulate
     torch+eval      torch fill, model.eval()(batch), score, accumulate   (fused=False)
   Each sample is timed with device events around work that ends in a synchronise; rows give
   the median and the range over --rounds rounds, per batch.
    python tools/importance_micro.py [--out profiles/importance_micro.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd")]

import torch  # noqa: E402

from raincast_gnn.batching import DeviceDataset  # noqa: E402
from raincast_gnn.data import GraphBatch, synthetic_samples  # noqa: E402
from raincast_gnn.forecast import Forecast  # noqa: E402
from raincast_gnn.importance import PermutationPlan, fill_batch  # noqa: E402
from raincast_gnn.inference import Predictor  # noqa: E402
from raincast_gnn.models import gnn_from_params  # noqa: E402
from raincast_gnn.params import BENCH_CONFIGS  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # achievable, MI355X


def make_dataset(cfg, T, dev):
    """The cfg's station graph with T samples generated on the device."""
    seed_samples = synthetic_samples(cfg.num_stations, 2, k=cfg.k, seed=1)
    ds = DeviceDataset(seed_samples, dev)
    N, F = seed_samples[0].x.shape
    M = seed_samples[0].ensemble.size(1)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    ds.x = torch.randn(T, N, F, device=dev, generator=g)
    ds.ensemble = torch.randn(T, N, M, F, device=dev, generator=g)
    ds.y = torch.randn(T, N, device=dev, generator=g)
    ds.y[torch.rand(T, N, device=dev, generator=g) < 0.01] = float("nan")
    return ds


def timed_us(run, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / calls


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--reps", type=int, default=16, help="fill launches per captured graph")
    ap.add_argument("--batches", type=int, default=16, help="batches per loop sample")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "importance_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("importance_micro needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    cfg = BENCH_CONFIGS[2]
    B = cfg.graphs_per_gpu
    T = args.samples
    ds = make_dataset(cfg, T, dev)
    _, N, F = ds.x.shape
    M = ds.ensemble.size(2)
    torch.manual_seed(0)
    model = gnn_from_params(cfg.params(), in_channels=F).to(dev).eval()
    gen = torch.Generator()
    gen.manual_seed(0)
    plan = PermutationPlan.draw(T, N, gen).on(ds)
    all_idx = torch.arange(T, device=dev)
    windows = [all_idx[s:s + B] for s in range(0, T - B + 1, B)]
    lines = [f"# cfg2: B={B} N={N} M={M} F={F} T={T} reps={args.reps} batches={args.batches} "
             f"rounds={args.rounds} device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    # -- 1. the fill kernel alone ------------------------------------------------------------
    moved = 2 * B * N * (M + 1) * F * 4
    floor_us = moved / HBM_BYTES_PER_S * 1e6
    out = (torch.empty(B * N, F, device=dev), torch.empty(B * N, M, F, device=dev),
           torch.empty(B * N, device=dev))
    masks = {"no column": [], "one column": [27], "all columns": list(range(F))}
    graphs = {}
    for name, cols in masks.items():
        def fills(cols=cols):
            for r in range(args.reps):
                fill_batch(ds, windows[r % len(windows)], plan, cols, out=out, kernel=True)
        graphs[name] = capture(fills)
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            times[k].append(timed_us(g.replay, args.reps))
    for k, ts in times.items():
        med = statistics.median(ts)
        emit({"what": "fill kernel", "columns": k, "us_median": round(med, 2),
              "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
              "bytes": moved, "floor_us": round(floor_us, 2),
              "time_over_floor": round(med / floor_us, 2),
              "TB_per_s": round(moved / med / 1e6, 2)})

    # -- 2. the per-batch loop ---------------------------------------------------------------
    pred = Predictor(model)
    tmpl = ds.batch(windows[0])
    handle = pred.bind(tmpl)
    ybuf = torch.empty_like(tmpl.y)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    cols = [27]

    def account(out_pred, y):
        sc = Forecast.from_model(model, out_pred).score(y)
        acc[0:1] += torch.nansum(sc.crps_rows).reshape(1)
        acc[1:2] += sc.valid

    def torch_batch(idx):
        got = fill_batch(ds, idx, plan, cols, kernel=False)
        return GraphBatch(got.x, got.ensemble, tmpl.edge_index, tmpl.edge_attr, got.y,
                          tmpl.batch, tmpl.ptr, tmpl.num_graphs, dict(tmpl.extra))

    def loop_fused():
        for i in range(args.batches):
            fill_batch(ds, windows[i % len(windows)], plan, cols,
                       out=(handle.x, handle.ensemble, ybuf))
            account(handle.run(), ybuf)

    def loop_torch_predictor():
        for i in range(args.batches):
            b = torch_batch(windows[i % len(windows)])
            account(pred(b), b.y)

    def loop_torch_eval():
        for i in range(args.batches):
            b = torch_batch(windows[i % len(windows)])
            account(model(b), b.y)

    def loop_forward_only():
        for _ in range(args.batches):
            handle.run()

    loops = {"fused": loop_fused, "torch+predictor": loop_torch_predictor,
             "torch+eval": loop_torch_eval, "replay only": loop_forward_only}
    with torch.no_grad():
        sums = {}
        for k, fn in loops.items():  # warm up, and the three forms agree
            acc.zero_()
            fn()
            torch.cuda.synchronize()
            sums[k] = acc.cpu().clone()
        ref = sums["fused"]
        emit({"what": "loop sums agree within 1e-12", **{
            k: bool(sums[k][1] == ref[1] > 0
                    and abs(sums[k][0] - ref[0]) <= 1e-12 * abs(ref[0]))
            for k in ("torch+predictor", "torch+eval")}})
        times = {k: [] for k in loops}
        for _ in range(args.rounds):
            for k, fn in loops.items():
                times[k].append(timed_us(fn, args.batches))
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        emit({"what": "loop, per batch", "form": k, "us_median": round(med[k], 1),
              "us_min": round(min(ts), 1), "us_max": round(max(ts), 1)})
    emit({"what": "loop ratio", "torch+predictor_over_fused":
          round(med["torch+predictor"] / med["fused"], 2),
          "torch+eval_over_fused": round(med["torch+eval"] / med["fused"], 2)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
