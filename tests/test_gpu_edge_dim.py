"""GPU: GINEConv with edge_dim up to 8 and the edge_attr gradient (csrc/gine_mpek.hip).

Bit-exact against the torch restatement of the K-term fma chain (tests/edge_dim_cases.py):
the graph build, the forward z and the backward dx.  Everything with a reduction over edges
or nodes (dW, db, deps, d edge_attr) and everything behind the node MLP: max-norm relative
1e-5 against the fp32 CPU reference with the fp64 tie-break (helpers.assert_close_tiebreak).
"""
import copy

import numpy as np
import pytest
import torch

from edge_dim_cases import GRAPHS, GRAPH_NAMES, SHAPES, mp_case, widen
from helpers import assert_close_tiebreak
from oracle import gine_cpu as O
from raincast_gnn import GINEConv, functional as Fn, options
from raincast_gnn.graph import GineGraph, _GraphCache, get_graph
from raincast_gnn.models import GNN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5


def _graph(c, K):
    """The K-wide graph of a case (at K = 1: the wide builder's, with out_eid)."""
    return GineGraph(c["ei"].to(DEV), c["ea"].to(DEV), c["n"], with_eid=K == 1)


def _dev(c, *names):
    return [c[k].to(DEV) for k in names]


# ---------------------------------------------------------------------------------------
# 1. graph build
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_graph_build_wide(name):
    ei, ea, n = GRAPHS[name]
    ea = widen(ea, 3, seed=1)
    g = GineGraph(ei.to(DEV), ea.to(DEV), n)
    E = ei.size(1)
    assert g.edge_dim == 3 and g.num_edges == E
    assert g.window_plan("in", 128) is None and g.window_plan("out", 128) is None
    assert g.layer_windows is None and not Fn.fused_forward_ok(g, n, 128)
    for key, other, rowptr, nbr, attr in ((1, 0, g.in_rowptr, g.in_src, g.in_attr),
                                          (0, 1, g.out_rowptr, g.out_dst, g.out_attr)):
        perm = np.argsort(ei[key].numpy(), kind="stable")
        counts = np.bincount(ei[key].numpy(), minlength=n)
        assert np.array_equal(rowptr.cpu().numpy(),
                              np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
        if E:
            assert np.array_equal(nbr.cpu().numpy()[:E], ei[other].numpy()[perm])
            assert attr.shape == (E, 3)
            assert np.array_equal(attr.cpu().numpy(), ea.numpy()[perm])
            if key == 0:
                assert np.array_equal(g.out_eid.cpu().numpy()[:E], perm)


def test_graph_build_wide_target_to_source():
    ei, ea, n = GRAPHS["hubs_unsorted"]
    ea = widen(ea, 3, seed=2)
    g = GineGraph(ei.to(DEV), ea.to(DEV), n, flow="target_to_source")
    # i = edge_index[0], j = edge_index[1]; edge ids stay those of the caller's tensor
    perm_in = np.argsort(ei[0].numpy(), kind="stable")
    perm_out = np.argsort(ei[1].numpy(), kind="stable")
    assert np.array_equal(g.in_src.cpu().numpy(), ei[1].numpy()[perm_in])
    assert np.array_equal(g.in_attr.cpu().numpy(), ea.numpy()[perm_in])
    assert np.array_equal(g.out_dst.cpu().numpy(), ei[0].numpy()[perm_out])
    assert np.array_equal(g.out_attr.cpu().numpy(), ea.numpy()[perm_out])
    assert np.array_equal(g.out_eid.cpu().numpy(), perm_out)


def test_content_cache_compares_every_attribute_column():
    ei, ea, n = GRAPHS["knn64_k4"]
    ea = widen(ea, 3, seed=3)
    other = ea.clone()
    other[-1, 2] += 1.0  # the last of the 4 * K * E attribute bytes
    cache = _GraphCache()
    eid = ei.to(DEV)
    g1 = cache.get(eid, ea.to(DEV), n)
    g2 = cache.get(eid.clone(), other.to(DEV), n)
    assert g2 is not g1 and cache.stats["builds"] == 2
    assert torch.equal(g2.in_attr.cpu(), other[torch.argsort(ei[1], stable=True)])
    g3 = cache.get(eid.clone(), ea.to(DEV), n)
    assert g3 is g1 and cache.stats["content_hits"] == 1
    g4 = cache.get(eid.clone(), other.to(DEV), n)
    assert g4 is g2 and cache.stats["content_hits"] == 2
    # the one-column graph of the same edge list is another graph again
    g5 = cache.get(eid.clone(), ea[:, :1].contiguous().to(DEV), n)
    assert g5.edge_dim == 1 and g5.out_eid is None and g5 is not g1


# ---------------------------------------------------------------------------------------
# 2. forward: the bits of the chain
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("D,K", SHAPES)
def test_mp_forward_bits(name, D, K):
    c = mp_case(name, D, K)
    x, W, b, eps = _dev(c, "x", "W", "b", "eps")
    z = Fn.mp_forward(x, _graph(c, K), W, b, eps)
    assert torch.equal(z.cpu(), c["z32"]), f"max diff {(z.cpu() - c['z32']).abs().max().item()}"
    if K == 1:
        # the new kernel on a plain K = 1 graph against the existing kernel's fma mode
        plain = GineGraph(c["ei"].to(DEV), c["ea"].to(DEV), c["n"])
        assert plain.out_eid is None
        z_new = Fn.mp_forward(x, plain, W.reshape(-1), b, eps, wide=True)
        z_old = Fn.mp_forward(x, plain, W.reshape(-1), b, eps, lin_flag=0)
        assert torch.equal(z_new, z_old) and torch.equal(z_new, z)


# ---------------------------------------------------------------------------------------
# 3. backward
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("D,K", SHAPES)
def test_mp_backward(name, D, K):
    c = mp_case(name, D, K)
    g = _graph(c, K)
    x, dz, W, b, eps = _dev(c, "x", "dz", "W", "b", "eps")
    E = c["ei"].size(1)
    runs = [Fn.mp_backward(dz, x, g, W, b, eps, edge_grad=True) for _ in range(2)]
    off = Fn.mp_backward(dz, x, g, W, b, eps)
    assert len(off) == 4 and len(runs[0]) == 5
    for a, r2, o in zip(runs[0][:4], runs[1][:4], off):
        assert torch.equal(a, r2) and torch.equal(a, o)      # run to run; EATTR on and off
    assert torch.equal(runs[0][4], runs[1][4])
    dx, dW, db, deps, dea = runs[0]
    g32, g64 = c["g32"], c["g64"]
    # same decisions, same order: bit-identical to CPU autograd (index_add_)
    assert torch.equal(dx.cpu(), g32["x"]), f"max diff {(dx.cpu() - g32['x']).abs().max()}"
    assert dea.shape == (E, K) and dW.numel() == D * K
    for nm, got, key in (("dW", dW.view(D, K), "W"), ("db", db, "b"), ("deps", deps, "eps"),
                         ("dea", dea, "ea")):
        ref32, ref64 = g32[key], g64[key]
        assert got.shape == ref32.shape, nm
        if ref32.numel() == 0:
            continue
        if ref64.abs().max() == 0:
            assert got.abs().max().item() == 0, nm
            continue
        assert_close_tiebreak(got.cpu(), ref32, ref64, TOL, nm)


def test_mp_backward_k1_matches_existing_kernel():
    """K = 1: the new backward on a plain graph has the existing kernel's dx bits and its
    parameter gradients within TOL (another block shape of the same fp64 sums)."""
    c = mp_case("knn500_k10_b2", 128, 1)
    plain = GineGraph(c["ei"].to(DEV), c["ea"].to(DEV), c["n"])
    x, dz, W, b, eps = _dev(c, "x", "dz", "W", "b", "eps")
    new = Fn.mp_backward(dz, x, plain, W.reshape(-1), b, eps, wide=True)
    old = Fn.mp_backward(dz, x, plain, W.reshape(-1), b, eps, lin_flag=0)
    assert torch.equal(new[0], old[0])
    for a, o, key in zip(new[1:], old[1:], ("W", "b", "eps")):
        assert_close_tiebreak(a.cpu().reshape(-1), o.cpu().reshape(-1),
                              c["g64"][key].reshape(-1), TOL, key)
    with pytest.raises(ValueError):
        Fn.mp_backward(dz, x, plain, W.reshape(-1), b, eps, edge_grad=True)  # no out_eid


def _make_pair(D, K, seed):
    torch.manual_seed(seed)
    mlp = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.BatchNorm1d(D), torch.nn.ReLU(),
                              torch.nn.Linear(D, D))
    conv = GINEConv(nn=mlp, train_eps=True, edge_dim=K)
    with torch.no_grad():
        conv.eps.fill_(0.125)
        mlp[1].weight.uniform_(0.5, 1.5)
        mlp[1].bias.uniform_(-0.2, 0.2)
        mlp[1].running_mean.uniform_(-0.1, 0.1)
        mlp[1].running_var.uniform_(0.5, 2.0)
    ref = O.OracleGINEConv(copy.deepcopy(mlp), train_eps=True, edge_dim=K)
    ref.load_state_dict(conv.state_dict())
    return conv.to(DEV), ref


def _oracle_layer(ref, x, ei, ea, epilogue, dtype):
    r = copy.deepcopy(ref).to(dtype)
    xx = x.detach().to(dtype).requires_grad_(True)
    aa = ea.detach().to(dtype).requires_grad_(True)
    o = r(xx, ei, aa)
    if epilogue == "relu":
        o = torch.relu(o)
    elif epilogue == "residual":
        o = xx + torch.relu(o)
    return r, xx, aa, o


def _check_layer(conv, ref, x, ei, ea, dy, epilogue):
    """Engine layer against the oracle: y and the x, edge_attr and parameter gradients."""
    outs = {}
    for dtype in (torch.float32, torch.float64):
        r, xx, aa, o = _oracle_layer(ref, x, ei, ea, epilogue, dtype)
        o.backward(dy.to(dtype))
        outs[dtype] = (r, xx, aa, o)
    xd = x.to(DEV).requires_grad_(True)
    ad = ea.to(DEV).requires_grad_(True)
    fn = {"none": conv.forward, "relu": conv.forward_relu,
          "residual": conv.forward_residual_relu}[epilogue]
    y = fn(xd, ei.to(DEV), ad)
    y.backward(dy.to(DEV))
    (r32, x32, a32, o32), (r64, x64, a64, o64) = outs[torch.float32], outs[torch.float64]
    assert_close_tiebreak(y.detach().cpu(), o32.detach(), o64.detach(), TOL, "y")
    assert_close_tiebreak(xd.grad.cpu(), x32.grad, x64.grad, TOL, "dx")
    assert ad.grad is not None and ad.grad.shape == ea.shape
    assert_close_tiebreak(ad.grad.cpu(), a32.grad, a64.grad, TOL, "d edge_attr")
    p_gpu = dict(conv.named_parameters())
    p32, p64 = dict(r32.named_parameters()), dict(r64.named_parameters())
    for name in p32:
        assert p_gpu[name].grad.shape == p32[name].grad.shape, name
        assert_close_tiebreak(p_gpu[name].grad.cpu(), p32[name].grad, p64[name].grad, TOL, name)
    return y


def test_edge_attr_gradient_at_k1_through_gineconv():
    ei, ea, n = GRAPHS["knn64_k4"]
    conv, ref = _make_pair(64, 1, seed=4)
    torch.manual_seed(5)
    x, dy = torch.randn(n, 64), torch.randn(n, 64)
    _check_layer(conv, ref, x, ei, ea, dy, "none")
    # [E] attributes: the gradient comes back in the caller's shape
    xd = x.to(DEV).requires_grad_(True)
    flat = ea.reshape(-1).to(DEV).requires_grad_(True)
    conv(xd, ei.to(DEV), flat).backward(dy.to(DEV))
    assert flat.grad.shape == flat.shape and bool(flat.grad.abs().max() > 0)


# ---------------------------------------------------------------------------------------
# 4. against torch's own Linear(K, D)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("K", [2, 8])
def test_forward_against_torch_linear(name, K):
    D = 128
    c = mp_case(name, D, K)
    z_ref = O.gine_aggregate(c["x"], c["ei"], c["ea"], c["W"], c["b"], c["eps"])
    z64 = O.gine_aggregate(c["x"].double(), c["ei"], c["ea"].double(), c["W"].double(),
                           c["b"].double(), c["eps"].double())
    x, W, b, eps = _dev(c, "x", "W", "b", "eps")
    z = Fn.mp_forward(x, _graph(c, K), W, b, eps)
    assert z.shape == (c["n"], D)
    assert_close_tiebreak(z.cpu(), z_ref, z64, TOL, "z")


# ---------------------------------------------------------------------------------------
# 5. the layer
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("epilogue", ["none", "relu", "residual"])
@pytest.mark.parametrize("training", [True, False])
def test_gine_layer_wide(D, K, epilogue, training):
    ei, ea, n = GRAPHS["knn500_k10_b2"]
    ea = widen(ea, K, seed=D + K)
    conv, ref = _make_pair(D, K, seed=D + K + len(epilogue))
    conv.train(training)
    ref.train(training)
    torch.manual_seed(D + K)
    x, dy = torch.randn(n, D), torch.randn(n, D)
    _check_layer(conv, ref, x, ei, ea, dy, epilogue)
    assert int(conv.nn[1].num_batches_tracked) == int(training)


def test_flat_gradient_buffer_path_has_the_plain_path_bits():
    from raincast_gnn.optim import FlatAdamW
    D, K = 128, 4
    ei, ea, n = GRAPHS["knn500_k10_b2"]
    ea = widen(ea, K, seed=9)
    conv, _ = _make_pair(D, K, seed=21)
    flat = copy.deepcopy(conv)
    opt = FlatAdamW(flat.parameters(), lr=1e-3)
    opt.zero_grad()
    torch.manual_seed(2)
    x, dy = torch.randn(n, D, device=DEV), torch.randn(n, D, device=DEV)
    res = []
    for m in (conv, flat):
        xd = x.clone().requires_grad_(True)
        ad = ea.to(DEV).requires_grad_(True)
        y = m.forward_residual_relu(xd, ei.to(DEV), ad)
        y.backward(dy)
        res.append((y.detach(), xd.grad, ad.grad, dict(m.named_parameters())))
    base = opt.flat_grad.data_ptr()
    for name, p in res[1][3].items():  # the kernels wrote the slices themselves
        assert base <= p.grad.data_ptr() < base + 4 * opt.numel, name
    opt.gather_grads()
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(a, b)
    for name, p in res[0][3].items():
        assert torch.equal(p.grad, res[1][3][name].grad), name


# ---------------------------------------------------------------------------------------
# 6. the model
# ---------------------------------------------------------------------------------------
def _model_batch(K):
    from raincast_gnn.data import synthetic_batch
    batch = synthetic_batch(500, 2, k=10, seed=7)
    if K > 1:
        batch.edge_attr = widen(batch.edge_attr, K, seed=8)
    return batch.to(DEV)


def _model(K):
    torch.manual_seed(3)
    return GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5, edge_dim=K)


def test_model_training_step_eager_and_captured():
    batch = _model_batch(3)
    base = _model(3)

    def step(m):
        for p in m.parameters():
            if p.grad is not None:
                p.grad.zero_()
        loss = m.loss_fn.crps(m(batch), batch.y)
        loss.backward()
        return loss

    m_e = copy.deepcopy(base).to(DEV).train()
    for _ in range(3):
        loss_e = step(m_e)
    for name, p in m_e.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        assert bool(torch.isfinite(p.grad).all()), name
    assert m_e.conv.convolutions[0].lin.weight.grad.shape == (128, 3)
    assert bool(m_e.conv.convolutions[1].lin.weight.grad.abs().max() > 0)

    m_g = copy.deepcopy(base).to(DEV).train()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(m_g)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_g = step(m_g)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for (name, pe), (_, pg) in zip(m_e.named_parameters(), m_g.named_parameters()):
        assert torch.equal(pe.grad, pg.grad), name
    for (name, be), (_, bg) in zip(m_e.named_buffers(), m_g.named_buffers()):
        assert torch.equal(be, bg), name


def test_predictor_matches_eval_forward_at_k3():
    from raincast_gnn.inference import Predictor, layer_eval_ok
    batch = _model_batch(3)
    model = _model(3).to(DEV).eval()
    with torch.no_grad():
        want = model(batch)
    graph = get_graph(batch.edge_index, batch.edge_attr, batch.num_nodes)
    assert graph.edge_dim == 3
    h = torch.zeros(batch.num_nodes, 128, device=DEV)
    assert not layer_eval_ok(model.conv.convolutions[0], h, graph)  # the forward_relu path
    assert torch.equal(Predictor(model, capture=False)(batch), want)
    pred = Predictor(model, capture=True, warmup=1)
    outs = [pred(batch).clone() for _ in range(3)]
    assert len(pred._graphs) == 1  # the later calls were replays
    for o in outs:
        assert torch.equal(o, want)


def test_edge_dim_1_keeps_its_dispatch(monkeypatch):
    """edge_dim = 1 without an edge_attr gradient: the plain builder, and the fused, window
    and one-launch forms are still chosen where they were."""
    from raincast_gnn.inference import Predictor, layer_eval_ok
    batch = _model_batch(1)
    model = _model(1).to(DEV).eval()
    graph = get_graph(batch.edge_index, batch.edge_attr, batch.num_nodes)
    assert graph.edge_dim == 1 and graph.out_eid is None and not Fn.is_wide(graph)
    assert graph.in_attr.shape == (graph.num_edges,)
    assert Fn.fused_forward_ok(graph, batch.num_nodes, 128)
    monkeypatch.setattr(options, "MP_WINDOW", "all")
    staged = GineGraph(batch.edge_index, batch.edge_attr, batch.num_nodes)
    assert staged.window_plan("out", 128) is not None
    assert staged.window_plan("in", 128) is not None
    wide = GineGraph(batch.edge_index, widen(batch.edge_attr.cpu(), 3).to(DEV), batch.num_nodes)
    assert wide.window_plan("out", 128) is None and wide.window_plan("in", 128) is None
    monkeypatch.undo()
    h = torch.zeros(batch.num_nodes, 128, device=DEV)
    assert layer_eval_ok(model.conv.convolutions[0], h, graph)
    with torch.no_grad():
        want = model(batch)
    assert torch.equal(Predictor(model, capture=False)(batch), want)
    # a K = 1 graph with out_eid is the same graph otherwise
    eid = GineGraph(batch.edge_index, batch.edge_attr, batch.num_nodes, with_eid=True)
    for a, b in ((eid.in_rowptr, graph.in_rowptr), (eid.in_src, graph.in_src),
                 (eid.in_attr, graph.in_attr), (eid.out_dst, graph.out_dst),
                 (eid.out_attr, graph.out_attr)):
        assert torch.equal(a.reshape(-1), b.reshape(-1))


# ---------------------------------------------------------------------------------------
# 7. errors, before any launch
# ---------------------------------------------------------------------------------------
def test_errors():
    ei, ea, n = GRAPHS["knn64_k4"]
    eid = ei.to(DEV)
    x = torch.randn(n, 64, device=DEV)

    def conv(D, K):
        mlp = torch.nn.Sequential(torch.nn.Linear(D, D), torch.nn.ReLU())
        return GINEConv(nn=mlp, train_eps=True, edge_dim=K).to(DEV)
    with pytest.raises(NotImplementedError, match="edge_dim=8"):
        conv(64, 9)(x, eid, widen(ea, 9).to(DEV))
    with pytest.raises(ValueError, match=r"\[E, 3\]"):
        conv(64, 3)(x, eid, widen(ea, 2).to(DEV))
    with pytest.raises(ValueError, match=r"\[E, 3\]"):
        conv(64, 3)(x, eid, ea.reshape(-1).to(DEV))
    with pytest.raises(ValueError, match=r"\[E, 1\]"):
        conv(64, 1)(x, eid, widen(ea, 2).to(DEV))
    with pytest.raises(ValueError, match="rows"):
        conv(64, 2)(x, eid, widen(ea, 2)[:-1].to(DEV))
    x260 = torch.randn(n, 260, device=DEV)
    with pytest.raises(NotImplementedError, match="256"):
        conv(260, 2)(x260, eid, widen(ea, 2).to(DEV))
    with pytest.raises(NotImplementedError, match="256"):
        conv(260, 1)(x260, eid, ea.to(DEV).requires_grad_(True))
    y = conv(260, 1)(x260, eid, ea.to(DEV))  # ... while K = 1 without the gradient runs
    assert y.shape == (n, 260)
    with pytest.raises(NotImplementedError):
        GINEConv(nn=torch.nn.Linear(64, 64)).to(DEV)(x, eid, torch.randn(ei.size(1), 64).to(DEV))
    with pytest.raises(NotImplementedError):
        GineGraph(eid, widen(ea, 9).to(DEV), n)
    g2 = GineGraph(eid, widen(ea, 2).to(DEV), n)
    with pytest.raises(NotImplementedError, match="256"):
        Fn.mp_forward(x260, g2, torch.zeros(260, 2, device=DEV), torch.zeros(260, device=DEV),
                      torch.zeros(1, device=DEV))
