"""Microbenchmark of the encoder's backward: the fused launch (gine_deepset_bwd_chain) against
the pair it replaces (gine_chain_bwd_folded2 then gine_deepset_bwd), HIP events, standalone
(back-to-back launches on one stream) and captured (replays of a HIP graph holding one).
    python tools/enc_bwd_micro.py [--reps 200] [--shapes 16000x128,8224x128,8200x128,16416x64]
Both leave the DeepSet slab unreduced (dw1 = NULL), as the training step does."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "raincast-gnn_amd"))
import torch  # noqa: E402

from raincast_gnn import _lib  # noqa: E402

P = _lib.ptr


def timed(fn, reps):
    for _ in range(10):
        fn()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(reps):
        fn()
    en.record()
    torch.cuda.synchronize()
    return round(st.elapsed_time(en) * 1e3 / reps, 2)


def captured(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return timed(g.replay, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--shapes", default="16000x128,8224x128,8200x128,16416x64")
    ap.add_argument("--M", type=int, default=11)
    ap.add_argument("--F", type=int, default=35)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    M, F = a.M, a.F
    for shape in a.shapes.split(","):
        N, H = map(int, shape.split("x"))
        ok = ctypes.c_int32(0)
        _lib.call("gine_deepset_bwd_chain_ok", N, H, F, F, ctypes.byref(ok))
        if not ok.value:
            print(shape, "not eligible for the fused launch", flush=True)
            continue
        ens, x = torch.randn(N, M, F, device=dev), torch.randn(N, F, device=dev)
        w1, b1 = torch.randn(H, F, device=dev) / F ** 0.5, torch.randn(H, device=dev) * 0.1
        sq = [torch.randn(H, H, device=dev) / H ** 0.5 for _ in range(3)]   # wp2, wr0, wr1
        bs = [torch.randn(H, device=dev) * 0.1 for _ in range(4)]           # bp2, br0, br1, bdr
        wdr = torch.randn(H, F + H, device=dev) / (F + H) ** 0.5
        dh0 = torch.randn(N, H, device=dev)
        nbytes = ctypes.c_size_t(0)
        _lib.call("gine_deepset_mask_bytes", N, M, H, ctypes.byref(nbytes))
        mask = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        n1 = 2 * H * (F + H) + H
        wfold = torch.empty(n1 + H * H + H, device=dev)
        r, u, h0, dt, dr = (torch.empty(N, H, device=dev) for _ in range(5))
        parts = ctypes.c_int32(0)
        _lib.call("gine_deepset_bwd_num_partials", N, H, ctypes.byref(parts))
        slab = torch.empty(parts.value * (H * F + H), device=dev)

        def s():
            return _lib.stream_handle(dev)
        _lib.call("gine_deepset_fwd_fold2", P(ens), P(w1), P(b1), P(r), P(mask), N, M, F, H,
                  P(sq[2]), P(bs[2]), P(wdr), P(bs[3]), P(wfold), F, P(sq[1]), P(bs[1]),
                  P(sq[0]), P(bs[0]), P(wfold[n1:]), s())
        _lib.call("gine_chain_fwd_folded2", P(r), P(x), P(wfold[:n1]), P(wfold[n1:]), P(u),
                  P(h0), N, H, F, s())

        def chain():
            _lib.call("gine_chain_bwd_folded2", P(dh0), P(u), P(wfold[:n1]), P(wfold[n1:]),
                      P(dt), P(dr), N, H, F, s())

        def ds():
            _lib.call("gine_deepset_bwd", P(ens), P(mask), P(dr), P(slab), None, None, N, M, F,
                      H, s())

        def pair():
            chain()
            ds()

        def fused():
            _lib.call("gine_deepset_bwd_chain", P(ens), P(mask), P(dh0), P(u), P(wfold[:n1]),
                      P(wfold[n1:]), P(dt), P(slab), None, None, N, M, F, H, F, s())
        res = {"chain_us": timed(chain, a.reps), "deepset_us": timed(ds, a.reps),
               "pair_us": timed(pair, a.reps), "fused_us": timed(fused, a.reps),
               "pair_captured_us": captured(pair, a.reps),
               "fused_captured_us": captured(fused, a.reps)}
        print(shape, json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
