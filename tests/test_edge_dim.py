"""CPU: GINEConv edge_dim up to 8 -- the new C-ABI entries' host validation, the torch
restatement of the K-term fma chain (tests/edge_dim_cases.py), the K-column station graph
and the models' ``edge_dim`` argument.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from edge_dim_cases import aggregate_chain, chain_lin, mp_params, widen
from helpers import special_graphs
from oracle import gine_cpu as O
from raincast_gnn import _lib
from raincast_gnn import data as rdata
from raincast_gnn.models import GNN, ResGnn, gnn_from_params

TOL = 1e-5
NEW = ("gine_mp_fwd_ek", "gine_mp_bwd_ek_num_partials", "gine_mp_bwd_ek",
       "gine_mp_bwd_ek_finalize", "gine_graph_build_ek", "gine_graph_same_edges_ek")
INVALID, DIM = _lib.GINE_ERR_INVALID, _lib.GINE_ERR_DIM


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.MP_MAX_EDGE_DIM == 8


def test_host_validation_without_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def fwd(N, E, D, K, ops=(p,) * 8):
        return lib.gine_mp_fwd_ek(*ops, N, E, D, K, None)

    def bwd(N, E, D, K, ops=(p,) * 13, flags=1):
        return lib.gine_mp_bwd_ek(*ops, N, E, D, K, flags, None)
    for K in (0, 9, -1):
        assert fwd(10, 20, 128, K) == INVALID
        assert bwd(10, 20, 128, K) == INVALID
        assert lib.gine_mp_bwd_ek_finalize(p, 4, 128, K, p, p, p, None) == INVALID
    for D in (6, 260, 0, 1024):
        assert fwd(10, 20, D, 2) == DIM
        assert bwd(10, 20, D, 2) == DIM
        assert lib.gine_mp_bwd_ek_finalize(p, 4, D, 2, p, p, p, None) == DIM
    assert fwd(0, 0, 128, 3) == 0 and bwd(0, 0, 128, 3) == 0           # nothing launched
    assert fwd(-1, 0, 128, 3) == INVALID and fwd(5, -1, 128, 3) == INVALID
    assert bwd(5, 5, 128, 3, flags=2) == INVALID                       # no rounding flag here
    assert fwd(1 << 23, 8, 256, 2) == _lib.GINE_ERR_TOO_LARGE          # N * D * 4 = 2^33
    assert fwd(8, 1 << 28, 128, 8) == _lib.GINE_ERR_TOO_LARGE          # E * K * 4 = 2^33
    for i in (0, 1, 4, 5, 6, 7):                                       # NULL operands
        assert fwd(10, 20, 128, 2, (p,) * i + (None,) + (p,) * (7 - i)) == INVALID
    assert fwd(10, 20, 128, 2, (p, p, None, p, p, p, p, p)) == INVALID  # edges, no in_src
    for i in (0, 1, 2, 6, 7, 8, 10, 12):
        assert bwd(10, 20, 128, 2, (p,) * i + (None,) + (p,) * (12 - i)) == INVALID
    assert bwd(10, 20, 128, 2, (p,) * 5 + (None,) + (p,) * 7) == INVALID  # dea without out_eid
    n = ctypes.c_int32(0)
    assert lib.gine_mp_bwd_ek_num_partials(16000, 128, 4, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.gine_mp_bwd_ek_num_partials(16000, 128, 9, ctypes.byref(n)) == INVALID
    assert lib.gine_mp_bwd_ek_num_partials(16000, 260, 4, ctypes.byref(n)) == DIM
    assert lib.gine_mp_bwd_ek_num_partials(16000, 128, 4, None) == INVALID
    g = lib.gine_graph_build_ek
    assert g(p, p, 10, 20, 9, p, p, p, p, p, p, p, p, p, 1 << 20, None) == INVALID
    assert g(p, p, 10, 20, 0, p, p, p, p, p, p, p, p, p, 1 << 20, None) == INVALID
    assert g(p, p, 10, 20, 2, p, p, p, p, p, p, None, p, p, 1 << 20, None) == INVALID  # out_eid
    assert g(p, None, 10, 20, 2, p, p, p, p, p, p, p, p, p, 1 << 20, None) == INVALID
    s = lib.gine_graph_same_edges_ek
    assert s(p, p, p, p, 8, 9, p, None) == INVALID and s(p, p, p, p, 8, 2, None, None) == INVALID
    assert s(p, p, p, None, 8, 2, p, None) == INVALID


def test_chain_lin_at_k1_is_one_fma():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(500, 1, generator=g) * 3
    w = torch.randn(32, 1, generator=g)
    b = torch.randn(32, generator=g)
    ref = (a.double() * w.double().T + b.double()).float()
    assert torch.equal(chain_lin(a, w, b), ref)
    # ... and at K = 3 it is the chain, term by term, not one rounding of the exact sum
    a3, w3 = torch.randn(500, 3, generator=g), torch.randn(32, 3, generator=g)
    e = b.expand(500, -1)
    for k in range(3):
        e = torch.from_numpy(np.float32(a3[:, k:k + 1].numpy().astype(np.float64)
                                        * w3[:, k].numpy().astype(np.float64)
                                        + e.numpy().astype(np.float64)))
    assert torch.equal(chain_lin(a3, w3, b), e)


@pytest.mark.parametrize("case", special_graphs(), ids=lambda c: c[0])
def test_aggregate_chain_agrees_with_the_oracle(case):
    """Against torch's own Linear(3, D) (oracle.gine_cpu.gine_aggregate): within TOL, forward
    and every gradient."""
    name, ei, ea, n = case
    D, K = 64, 3
    ea = widen(ea, K, seed=5)
    torch.manual_seed(11)
    x = torch.randn(n, D)
    dz = torch.randn(n, D)
    W, b, eps = mp_params(D, K, seed=2)
    got, ref = [], []
    for fn, out in ((aggregate_chain, got), (O.gine_aggregate, ref)):
        leaves = [t.clone().requires_grad_(True) for t in (x, ea, W, b, eps)]
        z = fn(leaves[0], ei, leaves[1], leaves[2], leaves[3], leaves[4])
        z.backward(dz)
        out.append(z.detach())
        out.extend(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves)
    for a, r in zip(got, ref):
        assert a.shape == r.shape
        if not r.numel():  # E = 0: the edge_attr gradient is [0, K]
            continue
        den = r.abs().max().item()
        assert (a - r).abs().max().item() <= TOL * den if den else not a.abs().max().item()


def test_build_edge_index_and_attr_extra_columns():
    lat, lon = rdata.synthetic_stations(40, seed=3)
    dist = rdata.haversine_matrix(lat, lon)
    ei0, ea0 = rdata.build_edge_index_and_attr(dist, 200.0)
    alt = np.random.default_rng(0).standard_normal((40, 40)).astype(np.float32)
    flag = (np.arange(40)[:, None] % 3 == np.arange(40)[None, :] % 3).astype(np.float32)
    ei, ea = rdata.build_edge_index_and_attr(dist, 200.0, extra=[alt, flag])
    E = ei0.size(1)
    assert E > 40 and torch.equal(ei, ei0)
    assert ea.shape == (E, 3) and ea.dtype == torch.float32
    assert torch.equal(ea[:, :1], ea0)                                  # column 0: today's
    row, col = ei[0, :E - 40].numpy(), ei[1, :E - 40].numpy()
    assert np.array_equal(ea[:E - 40, 1].numpy(), alt[row, col])        # column order
    assert np.array_equal(ea[:E - 40, 2].numpy(), flag[row, col])
    assert torch.equal(ea[E - 40:], torch.tensor([[1.0, 0.0, 0.0]]).expand(40, 3))  # loops
    for none in (None, [], ()):
        ei1, ea1 = rdata.build_edge_index_and_attr(dist, 200.0, extra=none)
        assert torch.equal(ei1, ei0) and torch.equal(ea1, ea0) and ea1.shape == (E, 1)
    with pytest.raises(ValueError):
        rdata.build_edge_index_and_attr(dist, 200.0, extra=[alt[:5]])


def test_models_take_edge_dim():
    D = 32
    m3 = GNN(35, D, D, 2, loss="NormalCRPS", edge_dim=3)
    m1 = GNN(35, D, D, 2, loss="NormalCRPS", edge_dim=1)
    m0 = GNN(35, D, D, 2, loss="NormalCRPS")
    for conv in m3.conv.convolutions:
        assert conv.lin.weight.shape == (D, 3) and conv.lin.bias.shape == (D,)
    s0, s1, s3 = m0.state_dict(), m1.state_dict(), m3.state_dict()
    assert list(s0) == list(s1) == list(s3)                             # same keys
    assert {k: v.shape for k, v in s0.items()} == {k: v.shape for k, v in s1.items()}
    assert [k for k in s0 if s0[k].shape != s3[k].shape] == [
        f"conv.convolutions.{i}.lin.weight" for i in range(2)]
    assert ResGnn(D, D, 1, D, edge_dim=5).convolutions[0].lin.in_features == 5
    cfg = {"gnn_hidden": D, "gnn_layers": 1, "lr": 1e-3, "loss": "NormalCRPS", "grad_u": "False",
           "u": 1.0, "xi": 0.5}
    assert gnn_from_params(cfg).conv.convolutions[0].lin.in_features == 1
    assert gnn_from_params(dict(cfg, edge_dim=4)).conv.convolutions[0].lin.in_features == 4
    assert gnn_from_params(cfg, edge_dim=2).conv.convolutions[0].lin.in_features == 2


def test_batching_carries_wide_attributes():
    """collate and DeviceDataset concatenate / repeat edge_attr along dim 0: [E, K] stays
    [B * E, K], block after block."""
    from raincast_gnn.batching import DeviceDataset
    samples = rdata.synthetic_samples(30, 3, k=4, seed=2)
    wide = widen(samples[0].edge_attr, 3, seed=4)
    for s in samples:
        s.edge_attr = wide
    E = wide.size(0)
    b = rdata.collate(samples[:2])
    assert b.edge_attr.shape == (2 * E, 3) and torch.equal(b.edge_attr, torch.cat([wide, wide]))
    for relabel in (False, True):
        ds = DeviceDataset(samples, "cpu", relabel=relabel)
        gb = ds.batch(torch.tensor([2, 0]))
        assert gb.edge_attr.shape == (2 * E, 3) and gb.edge_index.shape == (2, 2 * E)
        assert torch.equal(gb.edge_attr, torch.cat([wide, wide]))   # edge order is kept
