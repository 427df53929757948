"""Microbenchmark of the paired-comparison kernels (csrc/gine_compare.hip: gine_compare_bootstrap
and gine_compare_dm) against a torch formulation on the same device.

The torch bootstrap draws the block starts with the same generator (int64 arithmetic wraps like
the kernel's uint64; logical shifts are masked arithmetic ones), builds the [R, T] matrix of how
often each day is drawn and multiplies it, in fp64, with the masked [T, 3 S] grid (a, b and the
valid flags, zeros at invalid pairs): the same sums in another order, checked to 1e-10 before
anything is timed.  The torch Diebold-Mariano pass is the vectorised form of the definitions.

Shapes (T, S, R, L): (730, 122, 10000, 1), (730, 122, 10000, 7), (730, 10000, 1000, 1) and the
overall column (730, 1, 100000, 1) with its weight; the DM pass at h = 7 on the first and third
grid.  Per shape the tool prints what the kernel has to do whatever its speed: 3 R T S fp64 adds
and 16 R T S bytes of on-chip reads (24 with a weight), and the rates they come to.

Two timings per kernel, both with device events around work that ends in a synchronise:
  graph  --reps calls captured into one HIP graph and replayed: device time alone
  eager  --reps calls issued from Python: what a caller pays, launch overhead included
The torch side is timed eager.  The variants alternate inside one run, --rounds times each;
rows show the median and the range over the rounds.
    python tools/compare_micro.py [--reps 3 --rounds 5 --out profiles/compare_micro.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raincast-gnn_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from raincast_gnn import compare as C  # noqa: E402

SHAPES = [(730, 122, 10000, 1), (730, 122, 10000, 7), (730, 10000, 1000, 1),
          (730, 1, 100000, 1)]
DM_SHAPES = [(730, 122), (730, 10000)]
LAGS = 7
SEED = 0
REP_CHUNK = 20000  # replicates per [R, T] count matrix of the torch side


def signed(c: int) -> int:
    return c - (1 << 64) if c >= 1 << 63 else c


def lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    return (z >> k) & ((1 << (64 - k)) - 1)


def torch_starts(seed, rep_first, R, T, L, dev):
    nb = -(-T // L)
    r = torch.arange(rep_first, rep_first + R, dtype=torch.int64, device=dev)
    i = r[:, None] * nb + torch.arange(nb, dtype=torch.int64, device=dev)[None, :]
    z = seed + (i + 1) * signed(0x9E3779B97F4A7C15)
    z = (z ^ lsr(z, 30)) * signed(0xBF58476D1CE4E5B9)
    z = (z ^ lsr(z, 27)) * signed(0x94D049BB133111EB)
    z = z ^ lsr(z, 31)
    return (lsr(z, 32) * T) >> 32


def torch_bootstrap(a, b, w, L, R):
    """-> (A, B, W), [R, S] each, by count matrix and matmul."""
    T, S = a.shape
    ok = ~torch.isnan(a) & ~torch.isnan(b)
    zero = torch.zeros_like(a)
    flags = ok.double() if w is None else torch.where(ok, w, zero)
    grid = torch.cat([torch.where(ok, a, zero), torch.where(ok, b, zero), flags], 1)
    step = torch.arange(L, dtype=torch.int64, device=a.device)
    out = []
    for r0 in range(0, R, REP_CHUNK):
        n = min(REP_CHUNK, R - r0)
        starts = torch_starts(SEED, r0, n, T, L, a.device)
        days = ((starts[:, :, None] + step) % T).reshape(n, -1)[:, :T]
        counts = torch.zeros(n, T, dtype=torch.float64, device=a.device)
        counts.scatter_add_(1, days, torch.ones_like(days, dtype=torch.float64))
        out.append(counts @ grid)
    res = torch.cat(out, 0)
    return res[:, :S], res[:, S:2 * S], res[:, 2 * S:]


def torch_dm(a, b, h):
    T = a.size(0)
    ok = ~torch.isnan(a) & ~torch.isnan(b)
    zero = torch.zeros_like(a)
    d = torch.where(ok, a - b, zero)
    n = ok.sum(0).double()
    dbar = d.sum(0) / n
    c = torch.where(ok, d - dbar, zero)
    v = (c * c).sum(0) / n
    for k in range(1, h + 1):
        v = v + 2.0 * (1.0 - k / (h + 1.0)) * ((c[:T - k] * c[k:]).sum(0) / n)
    var = v / n
    stat = dbar / torch.sqrt(var)
    return stat, torch.erfc(stat.abs() * 0.70710678118654752440)


def make_grid(T, S, dev):
    r = np.random.default_rng(T + S)
    a = r.gamma(2.0, 0.4, (T, S)) + 0.05
    b = a * np.exp(r.normal(0.05, 0.3, (T, S)))
    a[r.random((T, S)) < 0.07] = np.nan
    b[r.random((T, S)) < 0.05] = np.nan
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)


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


def close(x, y, what):
    assert torch.equal(torch.isnan(x), torch.isnan(y)), what
    assert (torch.nan_to_num(x - y).abs() <= 1e-10 * torch.nan_to_num(y).abs()).all(), what


def measure(table, reps, rounds, tag, lines):
    """table: name -> (fn, capturable).  Appends one row per variant and mode; -> medians."""
    for fn, _ in table.values():  # warm every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    graphs = {k: capture(fn, reps) for k, (fn, cap) in table.items() if cap}
    times = {}
    for _ in range(rounds):  # alternate the variants inside one run
        for k, (fn, _) in table.items():
            if k in graphs:
                times.setdefault((k, "graph"), []).append(timed_us(graphs[k].replay, reps))
            times.setdefault((k, "eager"), []).append(
                timed_us(lambda: [fn() for _ in range(reps)], reps))
    med = {}
    for (k, mode), ts in times.items():
        med[k, mode] = statistics.median(ts)
        lines.append(json.dumps({**tag, "variant": k, "mode": mode,
                                 "us_median": round(med[k, mode], 1),
                                 "us_min": round(min(ts), 1), "us_max": round(max(ts), 1)}))
        print(lines[-1], flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compare_micro needs a HIP device: nothing is measured without one "
                         f"(shapes would be {SHAPES}, DM at h={LAGS} on {DM_SHAPES})")
    dev = torch.device("cuda:0")
    lines = [f"# seed={SEED} reps={args.reps} rounds={args.rounds} "
             f"device={torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    for T, S, R, L in SHAPES:
        if S == 1:  # the overall column: day sums with their counts as the weight
            m = C.marginal_sums(*make_grid(T, 122, dev))
            a, b, w = (m[k].reshape(-1, 1) for k in ("day_a", "day_b", "day_n"))
        else:
            (a, b), w = make_grid(T, S, dev), None
        out = {k: torch.empty(R, S, dtype=torch.float64, device=dev) for k in C.SUM_FIELDS}

        def kernel():
            return C.replicate_sums(a, b, w, block_len=L, seed=SEED, replicates=R, out=out)

        def by_matmul():
            return torch_bootstrap(a, b, w, L, R)

        got, want = kernel(), by_matmul()
        for k, v in zip(("sum_a", "sum_b", "sum_w"), want):
            close(got[k], v, k)
        tag = {"T": T, "S": S, "R": R, "L": L}
        med = measure({"bootstrap kernel": (kernel, True), "bootstrap torch": (by_matmul, False)},
                      args.reps, args.rounds, tag, lines)
        adds, read = 3 * R * T * S, (16 if w is None else 24) * R * T * S
        us = med["bootstrap kernel", "graph"]
        lines.append(json.dumps({
            **tag, "fp64_adds": adds, "on_chip_read_bytes": read,
            "output_bytes": 5 * 8 * R * S, "kernel_gadds_per_s": round(adds / us / 1e3, 1),
            "kernel_read_tb_per_s": round(read / us / 1e6, 2),
            "torch_over_kernel_eager": round(med["bootstrap torch", "eager"]
                                             / med["bootstrap kernel", "eager"], 2)}))
        print(lines[-1], flush=True)
        del out, got, want
    for T, S in DM_SHAPES:
        a, b = make_grid(T, S, dev)
        r = C.dm_columns(a, b, LAGS)
        stat, p = torch_dm(a, b, LAGS)
        close(r["stat"], stat, "stat")
        close(r["pvalue"], p, "pvalue")
        tag = {"T": T, "S": S, "lags": LAGS}
        med = measure({"dm kernel": (lambda: C.dm_columns(a, b, LAGS), True),
                       "dm torch": (lambda: torch_dm(a, b, LAGS), False)},
                      args.reps, args.rounds, tag, lines)
        lines.append(json.dumps({**tag, "torch_over_kernel_eager":
                                 round(med["dm torch", "eager"] / med["dm kernel", "eager"], 2)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
