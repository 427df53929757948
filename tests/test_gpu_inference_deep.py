"""GPU: the eval-mode GINE layer in one launch at any in-degree (gine_mp_fwd_layer_eval_deep)
and the Predictor on graphs past GINE_MP_FUSED_MAX_DEGREE, against the eval path GINEConv /
GNN.forward take -- same bits everywhere (torch.equal).

The graphs (tests/deep_cases.py; their in-degrees are checked on the CPU by
tests/test_inference_deep.py) put a row one slot into the second and the third 32-slot chunk,
on exactly two chunks, on four; rows below and above the old limit in one tile; pairs of rows
(r and r + 16 of a tile are summed together) with different chunk counts, 0 | 97 and 32 | 33
among them; N = 1; and a graph within the old limit."""
import pytest
import torch
from torch.nn import BatchNorm1d, Linear, ReLU, Sequential

import deep_cases
from helpers import knn_batch_graph, rel_err
from raincast_gnn import _lib, functional, inference
from raincast_gnn import head as fused_head
from raincast_gnn.graph import get_graph
from raincast_gnn.inference import (Predictor, layer_eval, layer_eval_deep, layer_eval_deep_ok,
                                    layer_eval_ok)
from raincast_gnn.models import GNN
from raincast_gnn.nn import GINEConv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPIS = (_lib.EPI_NONE, _lib.EPI_RELU, _lib.EPI_RESIDUAL_RELU)
ROUNDINGS = (0, _lib.GINE_MP_LIN_MULADD)
KINDS = (("NormalCRPS", "False"), ("MixedNormalCRPS", "False"), ("MixedLoss", "False"),
         ("MixedLoss", "True"))
DEEP = "gine_mp_fwd_layer_eval_deep"


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaNs compared as equal (and in the same places)."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(
        ((a == b) | (a.isnan() & b.isnan())).all())


def make_conv(seed=0, D=128):
    """tests/test_gpu_inference.py's: a GINEConv with the reference's node MLP, every parameter
    off its default and non-trivial running statistics; in eval mode."""
    torch.manual_seed(seed)
    mlp = Sequential(Linear(D, D), BatchNorm1d(D), ReLU(), Linear(D, D))
    conv = GINEConv(nn=mlp, train_eps=True, edge_dim=1).to(DEV)
    with torch.no_grad():
        conv.eps.fill_(0.37)
        mlp[1].weight.uniform_(0.5, 1.5)
        mlp[1].bias.uniform_(-0.5, 0.5)
        ei, ea, n = knn_batch_graph(64, 4, 1, seed=9)
        conv.train()
        for s in (1.0, 2.5):
            conv(s * torch.randn(n, D, device=DEV) + 0.3, ei.to(DEV), ea.to(DEV))
    return conv.eval()


def existing(conv, x, ei, ea, epi):
    """The eval path as it stands: GINEConv's own launches under no_grad."""
    with torch.no_grad():
        if epi == _lib.EPI_NONE:
            return conv(x, ei, ea)
        if epi == _lib.EPI_RELU:
            return conv.forward_relu(x, ei, ea)
        return conv.forward_residual_relu(x, ei, ea)


@pytest.fixture(scope="module")
def conv():
    return make_conv()


@pytest.fixture(params=ROUNDINGS, ids=("fma", "muladd"))
def rounding(request, monkeypatch):
    monkeypatch.setattr(functional, "_LIN_FLAG", request.param)
    return request.param


def put(ei, ea):
    return ei.to(DEV), ea.to(DEV)


@pytest.mark.parametrize("case", deep_cases.layer_graphs(), ids=lambda c: c[0])
def test_layer_bits(conv, rounding, case):
    """Three epilogues x both edge-linear roundings on every graph: y has the existing eval
    path's bits -- and layer_eval's on the graph within the old limit."""
    name, ei, ea, n, claim = case
    ei, ea = put(ei, ea)
    torch.manual_seed(n)
    x = torch.randn(n, 128, device=DEV)
    graph = get_graph(ei, ea.float(), n)
    assert graph.max_in_degree == claim[1]
    assert layer_eval_deep_ok(conv, x, graph), name
    assert layer_eval_ok(conv, x, graph) == (claim[1] <= _lib.MP_FUSED_MAX_DEGREE)
    for epi in EPIS:
        want = existing(conv, x, ei, ea, epi)
        got = layer_eval_deep(conv, x, graph, epi)
        assert torch.equal(got, want), (name, epi, rel_err(got, want))
        if claim[1] <= _lib.MP_FUSED_MAX_DEGREE:
            assert torch.equal(got, layer_eval(conv, x, graph, epi)), (name, epi)


@pytest.mark.parametrize("max_wg", (1, 2, 3, 0))
def test_rounds(conv, rounding, max_wg):
    """In-degrees 26 .. 113 on 7 tiles (the last with 8 rows), walked by 1, 2 and 3 workgroups
    in rounds of two tiles and by the kernel's own grid."""
    ei, ea, n = deep_cases.rounds_graph()
    ei, ea = put(ei, ea)
    torch.manual_seed(n)
    x = torch.randn(n, 128, device=DEV)
    graph = get_graph(ei, ea.float(), n)
    assert graph.max_in_degree == 113
    for epi in EPIS:
        want = existing(conv, x, ei, ea, epi)
        got = layer_eval_deep(conv, x, graph, epi, max_workgroups=max_wg)
        assert torch.equal(got, want), (epi, max_wg, rel_err(got, want))


@pytest.mark.parametrize("loss,grad_u", KINDS, ids=lambda v: str(v))
def test_head(conv, loss, grad_u):
    """As the last layer at in-degree 33 with each loss kind and targets holding NaNs: pred, raw
    and the valid-target counts equal head.head(...) on the existing layer's output, with y and
    with y = NULL; one workgroup walking both tiles as well."""
    kind = fused_head.loss_kind(loss, grad_u)
    K = fused_head.K_OF[kind]
    torch.manual_seed(K)
    lin = Linear(128, K).to(DEV)
    ei, ea, n = knn_batch_graph(40, 32, 1, seed=40)
    ei, ea = put(ei, ea)
    x = torch.randn(n, 128, device=DEV)
    tgt = torch.rand(n, device=DEV)
    tgt[::7] = float("nan")
    graph = get_graph(ei, ea.float(), n)
    assert graph.max_in_degree == 33
    epi = _lib.EPI_RESIDUAL_RELU
    h = existing(conv, x, ei, ea, epi)
    with torch.no_grad():
        want = fused_head.head(h, lin, kind, tgt)
    rec = fused_head.record_of(want)
    assert rec.count_parts is not None
    for with_y, max_wg in ((True, 0), (False, 0), (False, 1)):
        plan = fused_head.plan(x, lin, kind, tgt)
        y = layer_eval_deep(conv, x, graph, epi, head=plan, with_y=with_y,
                            max_workgroups=max_wg)
        assert (y is None) == (not with_y)
        if with_y:
            assert torch.equal(y, h)
        assert torch.equal(plan.pred, want), (with_y, max_wg)
        assert torch.equal(plan.raw, rec.raw)
        assert torch.equal(plan.parts, rec.count_parts)
        assert int(plan.parts.sum()) == int((~tgt.isnan()).sum())


def test_redo_path(conv, rounding):
    """One +inf and one NaN in x, each in a row that a hub of in-degree 47 reads from its second
    chunk (its last edge in CSR order): those waves' split-bf16 chains give NaN and are redone
    in fp32 -- same bits, NaNs in the same places."""
    ei, ea, n = deep_cases.redo_graph()
    ei, ea = put(ei, ea)
    torch.manual_seed(3)
    x = torch.randn(n, 128, device=DEV)
    graph = get_graph(ei, ea.float(), n)
    rowptr, src = graph.in_rowptr.cpu(), graph.in_src.cpu()
    for hub, last in deep_cases.REDO_HUBS:   # the hub's edge 46: slot 14 of its second chunk
        assert int(rowptr[hub + 1] - rowptr[hub]) == 47
        assert int(src[int(rowptr[hub]) + 46]) == last
    x[deep_cases.REDO_HUBS[0][1], 17] = float("inf")
    x[deep_cases.REDO_HUBS[1][1], 100] = float("nan")
    for epi in EPIS:
        want = existing(conv, x, ei, ea, epi)
        got = layer_eval_deep(conv, x, graph, epi)
        for hub, _ in deep_cases.REDO_HUBS:
            assert not want[hub].isfinite().all()
        assert not want.isnan().all()
        assert same_bits(got, want), epi


def _count_calls(monkeypatch):
    """Every _lib.call that launches, by name (test_no_side_effects_and_launch_count's way)."""
    names = []
    real = _lib.call

    def counting(name, *a):
        names.append(name)
        return real(name, *a)
    for mod in (_lib, functional, fused_head):
        monkeypatch.setattr(mod, "call", counting, raising=False)
    import raincast_gnn.chain
    import raincast_gnn.deepset
    for mod in (raincast_gnn.chain, raincast_gnn.deepset, inference, inference._lib):
        if hasattr(mod, "call"):
            monkeypatch.setattr(mod, "call", counting)
    return names


def _batches():
    from raincast_gnn.data import synthetic_batch
    return {"knn_k33": synthetic_batch(40, 2, k=33, seed=1).to(DEV),
            "radius_400km": synthetic_batch(300, 2, max_dist=400.0, seed=2).to(DEV),
            "within": synthetic_batch(60, 2, k=5, seed=1).to(DEV)}


@pytest.mark.parametrize("which", ("knn_k33", "radius_400km"))
def test_predictor(which, monkeypatch):
    """A 2-layer GNN on graphs past the old limit, eager and captured: model.eval()(batch)'s
    bits, and a forward is the front's two launches plus one deep launch per layer -- no
    gine_mp_fwd*, gine_mlp_fwd*, gine_bn_fwd* or head launch.  With the policy constant below
    N the layers run the existing path, still with the same bits."""
    monkeypatch.setattr(inference, "DEEP_MAX_NODES", None)
    batch = _batches()[which]
    torch.manual_seed(4)
    model = GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5).to(DEV)
    with torch.no_grad():
        model.train()
        model(batch)                    # running statistics off their defaults
        want = model.eval()(batch).clone()
    graph = get_graph(batch.edge_index, batch.edge_attr.float(), batch.x.size(0))
    assert graph.max_in_degree > _lib.MP_FUSED_MAX_DEGREE
    eager = Predictor(model, capture=False)
    captured = Predictor(model, capture=True, warmup=1)
    for _ in range(3):   # eager warm-up call, the capture, a replay
        assert torch.equal(eager(batch), want)
        assert torch.equal(captured(batch), want)
    assert len(captured._graphs) == 1
    names = _count_calls(monkeypatch)
    assert torch.equal(eager(batch), want)
    layers = [n for n in names if n == DEEP]
    front = [n for n in names if n.startswith(("gine_deepset_fwd", "gine_chain_fwd"))]
    others = [n for n in names if n not in layers and n not in front]
    assert len(layers) == 2 and len(front) == 2, names
    assert not [n for n in others if "fwd" in n or "head" in n or "mp_" in n], names
    # the policy: a limit at N still takes the deep launch, one below N does not
    for limit, deep_layers in ((batch.x.size(0), 2), (batch.x.size(0) - 1, 0)):
        monkeypatch.setattr(inference, "DEEP_MAX_NODES", limit)
        del names[:]
        assert torch.equal(eager(batch), want)
        assert names.count(DEEP) == deep_layers, (limit, names)
        assert "gine_mp_fwd_layer_eval" not in names


def test_predictor_within_the_limit_runs_the_existing_entry(monkeypatch):
    monkeypatch.setattr(inference, "DEEP_MAX_NODES", None)
    batch = _batches()["within"]
    torch.manual_seed(4)
    model = GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5).to(DEV)
    with torch.no_grad():
        want = model.eval()(batch).clone()
    pred = Predictor(model, capture=False)
    assert torch.equal(pred(batch), want)
    names = _count_calls(monkeypatch)
    assert torch.equal(pred(batch), want)
    assert names.count("gine_mp_fwd_layer_eval") == 2 and DEEP not in names, names
