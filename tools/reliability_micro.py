"""Microbenchmark of the reliability kernels (csrc/gine_reliability.hip: gine_reliability_counts,
gine_reliability_fit, gine_reliability_resample) against a torch formulation on the same device.

Shapes (N, T, q, R): the workload's own (730 * 122, 5, 1000, 1000), the same rows with
ensemble-like probabilities on q = 11, and one tenfold N.  The probabilities fall with the
threshold and the outcomes are drawn from them, so the events are nested as real ones are.

The resampling kernel is timed in each traversal it has at the shape: atomic (one LDS add per
synthetic event) everywhere, ballot (a ballot and popcount per level) at K <= 64.

The comparator is torch on the same device: the same generator in int64 arithmetic (it wraps
like the kernel's uint64; logical shifts are masked arithmetic ones), the compare against
thr[level], and scatter_add_ into [R_chunk, K] counts per column.  torch has no isotonic fit:
the comparator covers the DRAW-AND-COUNT HALF ONLY, while the kernel's time includes the fit of
every (replicate, column) and the store of cal_rep.  Its counts are checked against the
kernel's e* before anything is timed.

Kernel times are replays of a captured graph of --reps calls (device time alone); the torch
side is timed eager.  The variants alternate inside one run, --rounds times each; rows show the
median and the range.  Per shape the tool prints draws (R * N hashes) and cells (R * N * T
compares) per second, and the cycles a SIMD spends per wavefront-draw (64 draws with their T
cells each, 1,024 SIMDs at 2.4 GHz) next to the 79 cycles per wavefront-draw measured for the
bootstrap of DESIGN.md 6j, with the instruction count of the resampling kernels from the
library's disassembly.
    python tools/reliability_micro.py [--reps 3 --rounds 5 --out profiles/reliability_micro.txt]
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

from raincast_gnn import _lib  # noqa: E402
from raincast_gnn.reliability import Reliability  # noqa: E402

BASE_N = 730 * 122
SHAPES = [(BASE_N, 5, 1000, 1000), (BASE_N, 5, 11, 1000), (10 * BASE_N, 5, 1000, 1000)]
SEED = 0
SIMDS, CLOCK_HZ = 1024, 2.4e9
CHUNK_CELLS = 1 << 26  # [R_chunk, N] int64 elements of the torch side


def signed(c: int) -> int:
    return c - (1 << 64) if c >= 1 << 63 else c


def lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    return (z >> k) & ((1 << (64 - k)) - 1)


def torch_counts(level, q, R, dev):
    """-> e* [R, T, K] int64: the draw-and-count half in torch."""
    T, N = level.shape
    K = q + 1
    v = torch.from_numpy(np.arange(K, dtype=np.float64) / np.float64(q))
    thr = torch.floor(v * 9007199254740992.0).to(torch.int64).to(dev)
    ok = level >= 0
    lv = torch.where(ok, level, torch.zeros_like(level)).long()
    limit = thr[lv]  # [T, N]
    out = torch.empty(R, T, K, dtype=torch.int64, device=dev)
    step = max(1, CHUNK_CELLS // N)
    i = torch.arange(N, dtype=torch.int64, device=dev)
    for r0 in range(0, R, step):
        n = min(step, R - r0)
        r = torch.arange(r0, r0 + n, dtype=torch.int64, device=dev)
        z = SEED + (r[:, None] * N + i[None, :] + 1) * signed(0x9E3779B97F4A7C15)
        z = (z ^ lsr(z, 30)) * signed(0xBF58476D1CE4E5B9)
        z = (z ^ lsr(z, 27)) * signed(0x94D049BB133111EB)
        U = lsr(z ^ lsr(z, 31), 11)  # below 2^53: the signed compare is the unsigned one
        for t in range(T):
            fire = (ok[t][None, :] & (U < limit[t][None, :])).long()
            counts = torch.zeros(n, K, dtype=torch.int64, device=dev)
            counts.scatter_add_(1, lv[t][None, :].expand(n, N), fire)
            out[r0:r0 + n, t] = counts
    return out


def make_inputs(N, T, q, dev, ensemble_like):
    r = np.random.default_rng(N + q)
    base = r.beta(0.6, 2.0, N)
    p = np.stack([base ** (1.0 + 0.7 * t) for t in range(T)], 1)
    if ensemble_like:
        p = np.rint(p * q) / q
    u = r.random(N)
    y = ((u[:, None] < p).sum(1) - 0.5).astype(np.float32)  # y > t  iff  u < p_t (p falls with t)
    y[r.random(N) < 0.03] = np.nan
    x = np.arange(T, dtype=np.float64)
    return torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(x).to(dev)


def capture(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
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


def measure(table, reps, rounds, tag, lines):
    """table: name -> (fn, capturable).  Appends one row per variant; -> medians."""
    graphs = {k: capture(fn, reps) for k, (fn, cap) in table.items() if cap}
    times = {}
    for _ in range(rounds):  # alternate the variants inside one run
        for k, (fn, cap) in table.items():
            if cap:
                times.setdefault((k, "graph"), []).append(timed_us(graphs[k].replay, reps))
            else:
                times.setdefault((k, "eager"), []).append(timed_us(fn, 1))
    med = {}
    for (k, mode), ts in times.items():
        med[k] = statistics.median(ts)
        lines.append(json.dumps({**tag, "variant": k, "mode": mode, "us_median": round(med[k], 1),
                                 "us_min": round(min(ts), 1), "us_max": round(max(ts), 1)}))
        print(lines[-1], flush=True)
    return med


def instruction_counts():
    """Static instruction counts of the resampling kernels, from the library's disassembly."""
    try:
        import isa_audit
        table = {}
        for obj in isa_audit.code_objects(_lib.LIB_PATH):
            if b"k_reliability_resample" in obj:  # this source's code object alone
                table.update(isa_audit.count_ops(isa_audit.disassemble(obj)))
    except Exception as e:  # the disassembler is not everywhere
        return {"error": repr(e)}
    return {("ballot" if "Lb1" in k else "atomic"): v.get("insts")
            for k, v in table.items() if "k_reliability_resample" in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reliability_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reliability_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be {SHAPES})")
    dev = torch.device("cuda:0")
    lines = [f"# seed={SEED} reps={args.reps} rounds={args.rounds} "
             f"device={torch.cuda.get_device_name(0)}",
             "# the torch rows cover the draw-and-count half only (torch has no isotonic fit); "
             "the resample rows include the fit of every (replicate, column) and the cal_rep store",
             json.dumps({"resample_kernel_static_instructions": instruction_counts()})]
    print("\n".join(lines), flush=True)
    for N, T, q, R in SHAPES:
        K = q + 1
        p, y, x = make_inputs(N, T, q, dev, ensemble_like=q <= 64)
        rel = Reliability(p, y, x, levels=q)
        n_k, e_k, level = rel.counts()
        fit = rel.fit()
        # the torch counts are the kernel's, in every traversal
        check = 4
        want = torch_counts(level, q, check, dev)
        hows = ("atomic",) + (("ballot",) if K <= 64 else ())
        for how in hows:
            got = rel.replicates(check, SEED, 0, events=True, traversal=how)[2]
            assert torch.equal(got.long(), want), how
        cal = torch.empty(R, T, K, dtype=torch.float64, device=dev)
        stats = torch.empty(R, T, 3, dtype=torch.float64, device=dev)
        fit_stats = torch.empty(T, 8, dtype=torch.float64, device=dev)
        fit_cal = torch.empty(T, K, dtype=torch.float64, device=dev)
        s_n, s_e, s_level = torch.empty_like(n_k), torch.empty_like(e_k), torch.empty_like(level)

        def counts():
            _lib.call("gine_reliability_counts", p.data_ptr(), p.stride(0), p.stride(1),
                      y.data_ptr(), x.data_ptr(), N, T, q, s_n.data_ptr(), s_e.data_ptr(),
                      s_level.data_ptr(), _lib.stream_handle(dev))

        def fit_call():
            _lib.call("gine_reliability_fit", n_k.data_ptr(), e_k.data_ptr(), T, q,
                      fit_cal.data_ptr(), None, None, None, None, None, fit_stats.data_ptr(),
                      _lib.stream_handle(dev))

        def resample(how):
            def run():
                _lib.call("gine_reliability_resample", level.data_ptr(), n_k.data_ptr(), N, T, q,
                          SEED, 0, R, how, cal.data_ptr(), stats.data_ptr(), None,
                          _lib.stream_handle(dev))
            return run

        table = {"counts": (counts, True), "fit": (fit_call, True),
                 "resample atomic": (resample(_lib.RELIABILITY_ATOMIC), True)}
        if K <= 64:
            table["resample ballot"] = (resample(_lib.RELIABILITY_BALLOT), True)
        table["torch draw+count"] = (lambda: torch_counts(level, q, R, dev), False)
        tag = {"N": N, "T": T, "q": q, "R": R}
        med = measure(table, args.reps, args.rounds, tag, lines)
        for k in [k for k in med if k.startswith("resample")]:
            us = med[k]
            lines.append(json.dumps({
                **tag, "variant": k, "draws": R * N, "cells": R * N * T,
                "gdraws_per_s": round(R * N / us / 1e3, 2),
                "gcells_per_s": round(R * N * T / us / 1e3, 2),
                "simd_cycles_per_wavefront_draw": round(
                    us * 1e-6 * CLOCK_HZ * SIMDS / (R * N / 64.0), 1),
                "bootstrap_6j_cycles_per_wavefront_draw": 79,
                "torch_draw_count_over_kernel": round(med["torch draw+count"] / us, 2)}))
            print(lines[-1], flush=True)
        del cal, stats, want, fit, rel
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
