"""Microbenchmark of the optimizer end of the training step (csrc/gine_optim.hip), at cfg2's
flat buffer (209,800 parameters plus the 64-float alignment gaps) and at 1,000,000 elements.

Variants, one optimizer step each:
  a  gine_adamw_step                        host scalars (the default FlatAdamW)
  b  gine_adamw_step_ctl without partials   device control block, no norm
  c  gine_grad_sumsq + gine_adamw_step_ctl  clipping and the non-finite test: one launch and
                                            one read of the gradient more than (a)
Every variant is captured into a HIP graph of --reps calls (no host time in the window); the
graphs are replayed in alternation, --rounds times each, timed with device events; the row
shows the median and the range over the rounds.  (c) - (a) is the price of clipping.  Bytes:
what each variant must move (param, exp_avg, exp_avg_sq read and written, grad read: 28 n;
(c) reads grad once more: 32 n).
    python tools/adamw_micro.py [--reps 50 --rounds 9]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd")]

import torch  # noqa: E402

from raincast_gnn import _lib  # noqa: E402
from raincast_gnn.models import gnn_from_params  # noqa: E402
from raincast_gnn.optim import FlatAdamW  # noqa: E402
from raincast_gnn.params import BENCH_CONFIGS  # noqa: E402

B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.01


def cfg2_flat_numel() -> int:
    """FlatAdamW's layout of the cfg2 model, from the shapes (no device needed)."""
    off = 0
    for p in gnn_from_params(BENCH_CONFIGS[2].params()).parameters():
        off = -(-(off + p.numel()) // FlatAdamW.ALIGN) * FlatAdamW.ALIGN
    return off


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


def variants(n, dev):
    """{name: (callable, bytes)} on buffers of their own (so the variants do not share
    cache lines)."""
    out = {}
    floats = ctypes.c_int64(0)
    _lib.call("gine_adamw_state_floats", ctypes.byref(floats))
    num = ctypes.c_int32(0)
    _lib.call("gine_grad_sumsq_num_partials", n, ctypes.byref(num))
    gen = torch.Generator().manual_seed(0)
    for name in ("a", "b", "c"):
        p = torch.randn(n, generator=gen).to(dev)
        g = (torch.randn(n, generator=gen) * 1e-2).to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        state = torch.zeros(floats.value, device=dev)
        ctl = torch.frombuffer(bytearray(bytes(_lib.AdamWCtl(1e-4, 1.0, _lib.LR_COSINE, 100.0,
                                                             1e6, 0.1, 1))),
                               dtype=torch.float32).to(dev)
        report = torch.zeros(4, device=dev)
        partials = torch.zeros(num.value, 2, dtype=torch.float64, device=dev)
        keep = (p, g, m, v, state, ctl, report, partials)
        bufs = (_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(state), n)

        def step_a(bufs=bufs, keep=keep):
            _lib.call("gine_adamw_step", *bufs, 1e-4, B1, B2, EPS, WD, _lib.stream_handle(dev))

        def step_b(bufs=bufs, keep=keep):
            _lib.call("gine_adamw_step_ctl", *bufs, _lib.ptr(keep[5]), None, 0,
                      _lib.ptr(keep[6]), B1, B2, EPS, WD, _lib.stream_handle(dev))

        def step_c(bufs=bufs, keep=keep):
            _lib.call("gine_grad_sumsq", bufs[1], n, _lib.ptr(keep[7]), keep[7].size(0),
                      _lib.stream_handle(dev))
            _lib.call("gine_adamw_step_ctl", *bufs, _lib.ptr(keep[5]), _lib.ptr(keep[7]),
                      keep[7].size(0), _lib.ptr(keep[6]), B1, B2, EPS, WD,
                      _lib.stream_handle(dev))

        out[name] = ({"a": step_a, "b": step_b, "c": step_c}[name],
                     (32 if name == "c" else 28) * n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=None,
                    help="flat-buffer lengths (default: cfg2's and 1,000,000)")
    args = ap.parse_args()
    sizes = args.sizes or [cfg2_flat_numel(), 1_000_000]
    if not torch.cuda.is_available():
        raise SystemExit(f"adamw_micro needs a HIP device: nothing is measured without one "
                         f"(sizes would be {sizes})")
    dev = torch.device("cuda:0")
    print(f"# reps={args.reps} rounds={args.rounds} device={torch.cuda.get_device_name(0)}")
    for n in sizes:
        table = variants(n, dev)
        graphs = {k: capture(fn, args.reps) for k, (fn, _) in table.items()}
        times = {k: [] for k in table}
        for _ in range(args.rounds):  # alternate the variants inside one run
            for k, gr in graphs.items():
                times[k].append(replay_us(gr, args.reps))
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            print(json.dumps({"n": n, "variant": k, "us_median": round(med[k], 2),
                              "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                              "bytes": table[k][1],
                              "GBps": round(table[k][1] / med[k] / 1e3, 1)}), flush=True)
        print(json.dumps({"n": n, "clipping_us": round(med["c"] - med["a"], 2),
                          "control_block_us": round(med["b"] - med["a"], 2)}), flush=True)


if __name__ == "__main__":
    main()
