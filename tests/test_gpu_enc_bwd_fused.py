"""GPU: the encoder's backward as one launch (gine_deepset_bwd_chain, csrc/gine_deepset.hip
k_deepset_bwd_chain) against the pair it replaces, gine_chain_bwd_folded2 then
gine_deepset_bwd, on the same inputs.

The fused launch runs the chain kernel's arithmetic (same fragments, k order and lane-half
split) and hands dr to the DeepSet walk through LDS, so dt, the DeepSet slab, dW1 and db1 must
be the pair's bits -- also with non-finite operands, where the NaN pattern and every finite
value must agree.  Shapes: the smallest with 16-node halves (N > 8,192 at H = 128, N > 16,384
at H = 64) that have whole groups, short last groups (rows past N in the chain tile and in
s_dr), and members per node below, at and across the 16-row half-tile.
"""
import copy
import ctypes

import pytest
import torch

from raincast_gnn import _lib, options

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = _lib.ptr
_REAL_CALL = _lib.call


def _ok(N, H, F, FX):
    ok = ctypes.c_int32(0)
    _lib.call("gine_deepset_bwd_chain_ok", N, H, F, FX, ctypes.byref(ok))
    return bool(ok.value)


class _Case:
    """Random ens, x, weights and dh0; wfold, the mask, r and u from the forward launches."""

    def __init__(self, N, M, H, F=35, FX=35, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed)

        def rnd(*shape, scale=1.0):
            return (torch.randn(*shape, generator=g) * scale).to(DEV)
        self.N, self.M, self.H, self.F, self.FX = N, M, H, F, FX
        self.ens, self.x = rnd(N, M, F), rnd(N, FX)
        w1, b1 = rnd(H, F, scale=F ** -0.5), rnd(H, scale=0.1)
        wp2, wr0, wr1 = (rnd(H, H, scale=H ** -0.5) for _ in range(3))
        bp2, br0, br1, bdr = (rnd(H, scale=0.1) for _ in range(4))
        wdr = rnd(H, FX + H, scale=(FX + H) ** -0.5)
        self.dh0 = rnd(N, H)
        st = _lib.stream_handle(DEV)
        nbytes = ctypes.c_size_t(0)
        _lib.call("gine_deepset_mask_bytes", N, M, H, ctypes.byref(nbytes))
        self.mask = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
        self.n1 = 2 * H * (FX + H) + H
        self.wfold = torch.empty(self.n1 + H * H + H, device=DEV)
        self.r, self.u, h0 = (torch.empty(N, H, device=DEV) for _ in range(3))
        _lib.call("gine_deepset_fwd_fold2", P(self.ens), P(w1), P(b1), P(self.r), P(self.mask),
                  N, M, F, H, P(wr1), P(br1), P(wdr), P(bdr), P(self.wfold), FX, P(wr0), P(br0),
                  P(wp2), P(bp2), P(self.wfold[self.n1:]), st)
        _lib.call("gine_chain_fwd_folded2", P(self.r), P(self.x), P(self.wfold[:self.n1]),
                  P(self.wfold[self.n1:]), P(self.u), P(h0), N, H, FX, st)
        parts = ctypes.c_int32(0)
        _lib.call("gine_deepset_bwd_num_partials", N, H, ctypes.byref(parts))
        self.parts = parts.value

    def _outs(self):
        H, F = self.H, self.F
        return (torch.empty(self.N, H, device=DEV), torch.empty(self.parts * (H * F + H), device=DEV),
                torch.empty(H, F, device=DEV), torch.empty(H, device=DEV))

    def pair(self):
        dt, slab, dw, db = self._outs()
        dr = torch.empty(self.N, self.H, device=DEV)
        st = _lib.stream_handle(DEV)
        _lib.call("gine_chain_bwd_folded2", P(self.dh0), P(self.u), P(self.wfold[:self.n1]),
                  P(self.wfold[self.n1:]), P(dt), P(dr), self.N, self.H, self.FX, st)
        _lib.call("gine_deepset_bwd", P(self.ens), P(self.mask), P(dr), P(slab), P(dw), P(db),
                  self.N, self.M, self.F, self.H, st)
        return dt, slab, dw, db

    def fused(self):
        assert _ok(self.N, self.H, self.F, self.FX)
        dt, slab, dw, db = self._outs()
        _lib.call("gine_deepset_bwd_chain", P(self.ens), P(self.mask), P(self.dh0), P(self.u),
                  P(self.wfold[:self.n1]), P(self.wfold[self.n1:]), P(dt), P(slab), P(dw), P(db),
                  self.N, self.M, self.F, self.H, self.FX, _lib.stream_handle(DEV))
        return dt, slab, dw, db


def _same(a, b):
    """Equal values with equal NaN patterns (inf compares equal to itself)."""
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0.), b.masked_fill(nb, 0.))


@pytest.mark.parametrize("N,M,H,F,FX", [
    (8224, 11, 128, 35, 35),    # 257 whole groups
    (8200, 11, 128, 35, 35),    # last group has 8 nodes
    (8193, 11, 128, 35, 35),    # last group has one node
    (8224, 1, 128, 35, 35),     # every row is a node of its own
    (8224, 16, 128, 35, 35),    # a node is exactly one half-tile
    (8224, 3, 128, 35, 35),     # nodes straddle tiles
    (8224, 11, 128, 35, 64),    # ldw = F + D with the other x width
    (16416, 11, 64, 35, 35),    # the H = 64 form
], ids=["whole", "short8", "short1", "M1", "M16", "M3", "x64", "H64"])
def test_fused_launch_same_bits_as_pair(N, M, H, F, FX):
    c = _Case(N, M, H, F, FX, seed=N + M + H + FX)
    ref, got = c.pair(), c.fused()
    for name, a, b in zip(("dt", "slab", "dW1", "db1"), got, ref):
        assert torch.equal(a, b), name
    assert torch.isfinite(got[2]).all() and got[2].abs().max() > 0


def test_not_eligible_shapes():
    assert _ok(16000, 128, 35, 35) and _ok(16384, 128, 35, 35) and _ok(8193, 128, 35, 35)
    assert not _ok(8192, 128, 35, 35)      # 8-node halves
    assert not _ok(16385, 128, 35, 35)     # more groups than workgroups
    assert not _ok(16000, 64, 35, 35) and _ok(16416, 64, 35, 35)
    assert not _ok(16416, 64, 48, 35)      # the H = 64, 48-feature kernel spills
    assert not _ok(16000, 256, 35, 35) and not _ok(16000, 128, 35, 65)
    buf = torch.empty(64, device=DEV)
    rc = _lib.load().gine_deepset_bwd_chain(*([P(buf)] * 10), 500, 11, 35, 128, 35, None)
    assert rc == _lib.GINE_ERR_INVALID


def test_non_finite_operands_same_pattern_as_pair():
    """A NaN row of dh0, +inf in Wf and a NaN ens value."""
    c = _Case(8224, 11, 128, seed=5)
    c.dh0[777] = float("nan")
    c.wfold[c.n1 + 5 * 128 + 9] = float("inf")
    c.ens[4321, 3, 7] = float("nan")
    ref, got = c.pair(), c.fused()
    for name, a, b in zip(("dt", "slab", "dW1", "db1"), got, ref):
        assert _same(a, b), name
    # the operands did reach the results: dt's row 777 and, through dr's row 777 (NaN in every
    # column, so in every hidden unit with a live member), dW1
    dt = got[0]
    assert dt[777].isnan().any() and torch.isfinite(dt[:777]).all() and got[2].isnan().any()


def test_rows_past_n_contribute_zero_with_nan_weight():
    """N = 8,200: the last group's chain tile has 24 rows past N, whose zero rows times a NaN
    weight are NaN in the tile; they must reach neither dt nor dW1 / db1."""
    c = _Case(8200, 11, 128, seed=6)
    c.wfold[c.n1 + 3 * 128 + 17] = float("nan")          # Wf[3][17]: column 17 of dr
    ref, got = c.pair(), c.fused()
    for name, a, b in zip(("dt", "slab", "dW1", "db1"), got, ref):
        assert _same(a, b), name
    dt, slab, dw, db = got
    assert torch.isfinite(dt).all()
    rows = torch.ones(128, dtype=torch.bool, device=DEV)
    rows[17] = False
    assert torch.isfinite(dw[rows]).all() and torch.isfinite(db[rows]).all()
    # the same with the NaN in W' (stage 1): rows past N stay out of the last slab row's bias
    c2 = _Case(8200, 11, 128, seed=7)
    c2.wfold[40 * (35 + 128) + 35 + 5] = float("nan")    # W'[40][F + 5]: column 5 of dt
    ref2, got2 = c2.pair(), c2.fused()
    for name, a, b in zip(("dt", "slab", "dW1", "db1"), got2, ref2):
        assert _same(a, b), name


def test_fused_launch_deterministic():
    c = _Case(8200, 11, 128, seed=8)
    a, b = c.fused(), c.fused()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


_ENC_LAUNCHES = ("gine_chain_bwd_folded2", "gine_deepset_bwd", "gine_deepset_bwd_chain",
                 "gine_chain_wgrad_folded2")


def _model_step(stations, graphs, fused, monkeypatch, base, batch):
    monkeypatch.setattr(options, "ENC_BWD_FUSED", fused)
    names = []

    def call(name, *args):
        names.append(name)
        return _REAL_CALL(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    m = copy.deepcopy(base)
    pred = m(batch)
    loss = m.loss_fn.crps(pred, batch.y)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    return pred.detach().clone(), loss.detach().clone(), grads, [n for n in names
                                                                  if n in _ENC_LAUNCHES]


@pytest.mark.parametrize("stations,graphs,eligible", [(257, 32, True), (500, 1, False)],
                         ids=["N8224", "N500"])
def test_model_same_bits_with_switch_on_and_off(stations, graphs, eligible, monkeypatch):
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.models import GNN
    torch.manual_seed(11)
    base = GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5).to(DEV).train()
    batch = synthetic_batch(stations, graphs, k=6, seed=4).to(DEV)
    assert _ok(stations * graphs, 128, 35, 35) == eligible
    p_off, l_off, g_off, n_off = _model_step(stations, graphs, False, monkeypatch, base, batch)
    p_on, l_on, g_on, n_on = _model_step(stations, graphs, True, monkeypatch, base, batch)
    assert torch.equal(p_on, p_off) and torch.equal(l_on, l_off)
    assert g_on.keys() == g_off.keys() and len(g_on) > 10
    for k in g_on:
        assert torch.equal(g_on[k], g_off[k]), k
    assert n_off == ["gine_chain_bwd_folded2", "gine_chain_wgrad_folded2", "gine_deepset_bwd"]
    if eligible:  # one launch fewer
        assert n_on == ["gine_deepset_bwd_chain", "gine_chain_wgrad_folded2"]
    else:
        assert n_on == n_off
