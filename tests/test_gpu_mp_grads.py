"""GPU: every output of the message-passing backward against the exact oracle
(tests/mp_grad_oracle.py), in every launch form, at the cases of tests/mp_grad_cases.py.

* ``dx`` has the oracle's bits (acc [+ fl((1 + eps) dz)] [+ dres]);
* ``dlin_w``, ``dlin_b`` and ``deps`` lie within ``bound(S, A, n) = 2^-24 |S| +
  gamma_n(2^-53) A + 2^-149`` of the exact sum S of the per-node fp32 values, per channel;
  where a term is not finite, the output is the oracle's NaN or infinity;
* ``d edge_attr`` has the bits of ``edge_grad``'s fp32 restatement and lies within
  ``(log2 L + 3) 2^-24 sum_c |dm_c W_ck|`` of the exact value;
* the window form's per-tile partial rows are held to the oracle restricted to the tile's
  nodes, so a wrong tile is named;
* two launches give the same bits.

Forms: gine_mp_bwd (+ gine_mp_bwd_finalize), gine_mp_bwd_ek (+ _ek_finalize), gine_mp_bwd_win
and gine_mp_bwd_win_side (+ _win_finalize), and gine_mp_bwd_win_mlp_wgrad as the layer's
backward launches it (its finish is then the batched one).  The capped cases (8,205 nodes at
D = 256: 2,052 tiles on 1,024 workgroups, the last tile partial) run the persistent tile loop
of k_mp_bwd and k_mp_bwd_ek, the uneven XCD spans and the carry of the fp64 partials across
tiles.

Printed by each test, not asserted: the worst error / bound and how many outputs are not the
correctly rounded S.  Measured on an MI355X (gfx950), worst over all cases of a form:

    form                        outputs   worst error/bound   not correctly rounded
    gine_mp_bwd                   8,280        0.995                  0
    gine_mp_bwd_ek                7,262        0.999                  0
    gine_mp_bwd_win               1,770        0.970                  0
    gine_mp_bwd_win_side          1,770        0.970                  0
    gine_mp_bwd_win_mlp_wgrad       257        0.934                  0
    d edge_attr (175,108 values)               0.441   (every value has the restatement's bits)
    window partial rows (fp64)                 0.000   (no row differs from its exact sum)

Every output is the correctly rounded exact sum, so the error is the one final rounding and
error / bound comes within a rounding of 1 wherever |S| sits at the bottom of its binade.
Three mutant libraries, each run once against this file (71 tests): multiply-then-add in place
of the fma of bwd_edge / bwd_edge_ek fails 59, ``pw`` / ``pb`` kept in fp32 fails 52,
``-ffp-contract=fast`` fails 63; the max-norm tests of the same outputs
(test_gpu_parity.py::test_mp_backward, ::test_mp_window_path_matches_gather_and_oracle and
test_gpu_edge_dim.py::test_mp_backward, 112 cases) pass on the first two.
"""
import ctypes

import numpy as np
import pytest
import torch

import mp_grad_cases as MC
import mp_grad_oracle as MO
from helpers import knn_batch_graph
from raincast_gnn import GINEConv, _lib, functional as Fn, options
from raincast_gnn import graph as G
from raincast_gnn import nn as rnn
from raincast_gnn._lib import call, ptr
from raincast_gnn.graph import GineGraph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(c):
    d = {k: _t(c[k]) for k in ("x", "dz", "dres", "W", "b")}
    d["eps"] = torch.tensor([c["eps"]], dtype=torch.float32, device=DEV)
    return d


def _flag(c):
    return 0 if c["mode"] == "fma" else _lib.GINE_MP_LIN_MULADD


def _report(tag, name, stats):
    worst = max(s[1] for s in stats.values())
    print(f"[{tag}] {name}: worst error/bound {worst:.3f}; not correctly rounded: "
          + ", ".join(f"{k} {s[2]}/{s[3]}" for k, s in stats.items()))


def _hold_params(name, got, ex):
    """dlin_w / dlin_b / deps of one launch against exact(): {output: (ok, worst, misrounded,
    outputs)}, asserted per channel."""
    dlw, dlb, deps = (_np(t) for t in got)
    stats = {}
    for key, val in (("dW", dlw), ("db", dlb), ("deps", deps)):
        ok, worst, mis = MO.held(val, ex[key])
        stats[key] = (ok, worst, mis, ex[key]["S"].size)
        assert ok, f"{name}: {key} leaves the oracle's bound (worst error/bound {worst:.3f})"
    return stats


def _same(a, b):
    return all(MO.same_bits(_np(u), _np(v)) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------
# gather form: gine_mp_bwd + gine_mp_bwd_finalize
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.GATHER)
def test_gather_form(name, monkeypatch):
    c, o = MC.case("gather", name), MC.oracle("gather", name)
    monkeypatch.setattr(options, "MP_WINDOW", "0")
    g = GineGraph(_t(c["ei"]), _t(c["ea"]), c["n"])
    N, D = c["x"].shape
    assert g.window_plan("out", D) is None
    if name.startswith("capped"):
        assert Fn._count("gine_mp_bwd_num_partials", N, D) == MC.CAP_PARTIALS
    d = _dev(c)
    args = (d["dz"], d["x"], g, d["W"].reshape(-1), d["b"], d["eps"])
    first = None
    for self_term in (True, False):
        for dres in (None, "dres"):
            kw = dict(dres=None if dres is None else d[dres], self_term=self_term,
                      lin_flag=_flag(c))
            r1, r2 = Fn.mp_backward(*args, **kw), Fn.mp_backward(*args, **kw)
            assert _same(r1, r2), f"{name}: two launches differ"
            want = MO.dx32(o["ns"]["acc"], c["dz"], c["eps"], self_term,
                           None if dres is None else c["dres"])
            assert MO.same_bits(_np(r1[0]), want), f"{name}: dx (self {self_term}, {dres})"
            if first is None:
                first = r1
            assert _same(first[1:], r1[1:])  # the parameter sums do not depend on the epilogue
    _report("gine_mp_bwd", name, _hold_params(name, first[1:], o["ex"]))


# ---------------------------------------------------------------------------------------
# K-wide form: gine_mp_bwd_ek + gine_mp_bwd_ek_finalize
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.EK)
def test_k_wide_form(name):
    c, o = MC.case("ek", name), MC.oracle("ek", name)
    N, D = c["x"].shape
    K = c["W"].shape[1]
    g = GineGraph(_t(c["ei"]), _t(c["ea"]), c["n"], with_eid=K == 1)
    if name.startswith("capped"):
        assert Fn._count3("gine_mp_bwd_ek_num_partials", N, D, K) == MC.CAP_PARTIALS
    d = _dev(c)
    args = (d["dz"], d["x"], g, d["W"], d["b"], d["eps"])
    on1, on2 = (Fn.mp_backward(*args, edge_grad=True) for _ in range(2))
    off = Fn.mp_backward(*args)
    assert len(on1) == 5 and len(off) == 4
    assert _same(on1, on2), f"{name}: two launches differ"
    assert _same(on1[:4], off), f"{name}: edge_grad on and off differ"
    assert MO.same_bits(_np(on1[0]), MO.dx32(o["ns"]["acc"], c["dz"], c["eps"]))
    alt = Fn.mp_backward(*args, dres=d["dres"], self_term=False, edge_grad=True)
    assert MO.same_bits(_np(alt[0]), MO.dx32(o["ns"]["acc"], c["dz"], c["eps"], False, c["dres"]))
    assert _same(alt[1:], on1[1:])
    stats = _hold_params(name, on1[1:4], o["ex"])
    # the edge_attr gradient: the restatement's bits, and the analytic bound less the fp64
    # reference's own error
    want, ref, mag, ref_err = o["dea"]
    dea = _np(on1[4])
    assert dea.shape == want.shape
    assert MO.same_bits(dea, want), f"{name}: d edge_attr is not edge_grad's restatement"
    L = MO.pow2ceil(D // 4)
    fin = np.isfinite(mag)
    with np.errstate(all="ignore"):
        lim = MO.edge_grad_bound(mag, L) - ref_err
        err = np.abs(dea.astype(np.float64) - ref)
    assert np.isfinite(dea[fin]).all() and (err[fin] <= lim[fin]).all(), name
    ratio = float((err[fin] / np.maximum(lim[fin], 2.0 ** -1000)).max()) if fin.any() else 0.0
    _report("gine_mp_bwd_ek", name, stats)
    print(f"[gine_mp_bwd_ek] {name}: d edge_attr worst error/bound {ratio:.3f} over {fin.sum()} "
          f"finite entries of {fin.size}")


# ---------------------------------------------------------------------------------------
# window form: gine_mp_bwd_win, gine_mp_bwd_win_side + gine_mp_bwd_win_finalize
# ---------------------------------------------------------------------------------------
def _tile_nodes(name):
    return 4 if name.startswith("planted") else 32 if name.startswith("hubs") else 128


def _win_launch(form, d, g, plan, flags, dres, N, D):
    """One window launch and its finish, as functional.mp_backward issues them, keeping the
    partial rows [tile, 3, D]."""
    P = plan.num_tiles
    partials = torch.zeros(P, 3, D, dtype=torch.float64, device=DEV)
    dx = torch.empty_like(d["x"])
    out = [torch.empty(D, device=DEV), torch.empty(D, device=DEV), torch.empty(1, device=DEV)]
    stream = _lib.stream_handle(DEV)
    args = (ptr(d["dz"]), ptr(d["x"]), ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_attr),
            ptr(d["W"].reshape(-1)), ptr(d["b"]), ptr(d["eps"]), ptr(dres), ptr(dx))
    if form == "win":
        call("gine_mp_bwd_win", *args, ptr(partials), N, D, flags, ctypes.byref(plan), stream)
    else:
        Dm = 64  # a node-MLP weight-gradient slab for the launch's extra workgroups to reduce
        C = Fn._count("gine_mlp_wgrad_num_chunks", N, Dm)
        slab = torch.randn(2 * C * (Dm * Dm + Dm), device=DEV)
        w = [torch.empty(Dm, Dm, device=DEV), torch.empty(Dm, device=DEV),
             torch.empty(Dm, Dm, device=DEV), torch.empty(Dm, device=DEV)]
        call("gine_mp_bwd_win_side", *args, ptr(partials), N, D, flags, ctypes.byref(plan),
             ptr(slab), C, Dm, *(ptr(t) for t in w), stream)
        # the side job did its own work too: z = 0 -> dW2 | db2, z = 1 -> dW1 | db1
        tot = slab.view(2, C, Dm * Dm + Dm).double().sum(1).float()
        for z, (wg, bg) in enumerate(((w[2], w[3]), (w[0], w[1]))):
            assert torch.allclose(wg.reshape(-1), tot[z, :Dm * Dm], rtol=1e-6, atol=1e-6)
            assert torch.allclose(bg, tot[z, Dm * Dm:], rtol=1e-6, atol=1e-6)
    call("gine_mp_bwd_win_finalize", ptr(partials), P, D, plan.slice_channels, *(ptr(t) for t in out),
         stream)
    torch.cuda.synchronize()
    return [dx] + out, partials


@pytest.mark.parametrize("form", ["win", "side"])
@pytest.mark.parametrize("name", MC.WIN)
def test_window_form(name, form, monkeypatch):
    c, o = MC.case("win", name), MC.oracle("win", name)
    N, D = c["x"].shape
    cs = dict(MC.WIN_SHAPES)[D]
    monkeypatch.setattr(options, "WINDOW_NODES", str(_tile_nodes(name)))
    monkeypatch.setattr(options, "MP_WINDOW", "all")
    g = GineGraph(_t(c["ei"]), _t(c["ea"]), c["n"])
    entry = g.window_plan_entry("out", D)
    assert entry is not None, f"{name}: no window plan at D = {D}"
    plan = entry[0]
    assert plan.slice_channels == cs, (plan.slice_channels, cs)
    tb = _np(entry[1][0])
    assert len(tb) == plan.num_tiles + 1 and tb[0] == 0 and tb[-1] == N
    d = _dev(c)
    flags = _lib.GINE_MP_BWD_SELF | _flag(c)
    (r1, p1), (r2, p2) = (_win_launch(form, d, g, plan, flags, d["dres"], N, D) for _ in range(2))
    assert _same(r1, r2) and torch.equal(p1, p2), f"{name}: two launches differ"
    want = MO.dx32(o["ns"]["acc"], c["dz"], c["eps"], True, c["dres"])
    assert MO.same_bits(_np(r1[0]), want), f"{name}: dx"
    r3, _ = _win_launch(form, d, g, plan, _flag(c), None, N, D)
    assert MO.same_bits(_np(r3[0]), MO.dx32(o["ns"]["acc"], c["dz"], c["eps"], False, None))
    assert _same(r3[1:], r1[1:])
    stats = _hold_params(name, r1[1:], o["ex"])
    # the partial rows, tile by tile (fp64: no final rounding), eps slice by slice
    part = _np(p1)
    worst = 0.0
    for t in range(plan.num_tiles):
        rows = (int(tb[t]), int(tb[t + 1]))
        ex = MO.exact(o["ns"], c["x"], c["dz"], rows=rows)
        for key, row in (("dW", part[t, 0]), ("db", part[t, 1])):
            S, A = ex[key]["S"].reshape(-1), ex[key]["A"].reshape(-1)
            lim = MO.bound64(S, A, max(ex[key]["n"], 1))
            err = np.abs(row - S)
            assert (err <= lim).all(), f"{name}: {key} partial row of tile {t} (nodes {rows})"
            worst = max(worst, float((err / np.maximum(lim, 2.0 ** -1000)).max()))
        for s in range(D // cs):
            e = MO.exact(o["ns"], c["x"], c["dz"], rows=rows, cols=(s * cs, (s + 1) * cs))["deps"]
            lim = MO.bound64(e["S"], e["A"], max(e["n"], 1))[0]
            assert abs(part[t, 2, s] - e["S"][0]) <= lim, (
                f"{name}: eps partial of tile {t} (nodes {rows}), slice {s}")
    _report(f"gine_mp_bwd_win{'_side' if form == 'side' else ''}", name, stats)
    print(f"[window partial rows] {name}: {plan.num_tiles} tiles, worst error/bound {worst:.3f}")


# ---------------------------------------------------------------------------------------
# window form with the node-MLP weight-gradient engine: as the layer's backward launches it
# ---------------------------------------------------------------------------------------
def test_window_form_with_engine_through_the_layer(monkeypatch):
    """gine_mp_bwd_win_mlp_wgrad needs the node MLP's saved tensors, so the layer launches it:
    the message passing's inputs and outputs are taken from that call and held to the oracle
    of those inputs.  Its finish is the batched one (gine_grad_finalize_batch)."""
    D = 128
    ei, ea, n = knn_batch_graph(300, 8, 2, seed=91)
    monkeypatch.setattr(options, "MP_WINDOW", "all")
    monkeypatch.setattr(rnn, "USE_TORCH_EXT", False)  # the Python Function calls mp_backward
    G.graph_cache.clear()
    calls = []
    inner = Fn.mp_backward

    def recording(dz, x, graph, lw, lb, ep, **kw):
        out = inner(dz, x, graph, lw, lb, ep, **kw)
        calls.append((dz, x, graph, lw, lb, ep, kw, out))
        return out
    monkeypatch.setattr(Fn, "mp_backward", recording)
    torch.manual_seed(12)
    mlp = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.BatchNorm1d(D), torch.nn.ReLU(),
                              torch.nn.Linear(D, D))
    conv = GINEConv(nn=mlp, train_eps=True, edge_dim=1).to(DEV).train()
    x = torch.randn(n, D, device=DEV, requires_grad=True)
    try:
        y = conv.forward_residual_relu(x, ei.to(DEV), ea.to(DEV))
        y.backward(torch.randn(n, D, device=DEV))
        torch.cuda.synchronize()
    finally:
        G.graph_cache.clear()
    assert len(calls) == 1
    dz, xs, graph, lw, lb, ep, kw, out = calls[0]
    plan = graph.window_plan("out", D)
    assert plan is not None and plan.slice_channels == 32
    assert kw.get("engine") is not None, "the layer did not launch gine_mp_bwd_win_mlp_wgrad"
    assert kw.get("lin_flag") is None and kw.get("self_term", True)
    mode = "fma" if Fn.edge_linear_flag() == 0 else "muladd"
    E = graph.num_edges
    xn, dzn = _np(xs), _np(dz)
    ns = MO.node_sums(xn, dzn, _np(graph.out_rowptr), _np(graph.out_dst)[:E],
                      _np(graph.out_attr).reshape(-1)[:E], _np(lw), _np(lb), mode)
    ex = MO.exact(ns, xn, dzn)
    MO.check_ranges(ex)
    dres = kw.get("dres")
    assert dres is not None
    want = MO.dx32(ns["acc"], dzn, float(_np(ep).reshape(-1)[0]), True, _np(dres))
    assert MO.same_bits(_np(out[0]), want)
    assert MO.same_bits(_np(x.grad), want)
    _report("gine_mp_bwd_win_mlp_wgrad", "knn300_k8_b2_D128",
            _hold_params("engine", out[1:4], ex))
    assert MO.same_bits(_np(conv.lin.bias.grad), _np(out[2]))
