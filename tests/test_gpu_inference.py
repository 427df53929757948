"""GPU: the eval-mode GINE layer in one launch (gine_mp_fwd_layer_eval) and the Predictor
against the eval path GINEConv / GNN.forward take today -- same bits everywhere.

Shapes are the smallest at which the kernel can go wrong: N = 1, one row short of / exactly /
one row past a 32-row tile, several tiles with a short last one, in-degree 0 and exactly 32,
no edges at all, and grids of 1, 2 and 3 workgroups walking 7 tiles in rounds of two."""
import pytest
import torch
from torch.nn import BatchNorm1d, Linear, ReLU, Sequential

from helpers import knn_batch_graph, rel_err, special_graphs
from oracle import gine_cpu as O
from raincast_gnn import _lib, functional
from raincast_gnn import head as fused_head
from raincast_gnn.graph import get_graph
from raincast_gnn.inference import Predictor, layer_eval, layer_eval_ok
from raincast_gnn.models import GNN
from raincast_gnn.nn import GINEConv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPIS = (_lib.EPI_NONE, _lib.EPI_RELU, _lib.EPI_RESIDUAL_RELU)
ROUNDINGS = (0, _lib.GINE_MP_LIN_MULADD)
KINDS = (("NormalCRPS", "False"), ("MixedNormalCRPS", "False"), ("MixedLoss", "False"),
         ("MixedLoss", "True"))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaNs compared as equal (and in the same places)."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(
        ((a == b) | (a.isnan() & b.isnan())).all())


def make_conv(seed=0, D=128, track=True):
    """A GINEConv with the reference's node MLP, every parameter off its default and (two
    training-mode calls on a 64-node graph) non-trivial running statistics; in eval mode."""
    torch.manual_seed(seed)
    mlp = Sequential(Linear(D, D), BatchNorm1d(D, track_running_stats=track), ReLU(),
                     Linear(D, D))
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


def graphs():
    out = [("knn%d_k6" % n, *knn_batch_graph(n, min(6, n - 1), 1, seed=n)[:2], n)
           for n in (31, 32, 33, 97, 200)]
    out.append(("one_node", torch.zeros(2, 3, dtype=torch.long), torch.rand(3, 1) + 0.5, 1))
    out.append(("knn37_k31_b3_degree32", *knn_batch_graph(37, 31, 3, seed=7)))
    out += [(name, ei, ea, n) for name, ei, ea, n in special_graphs()]
    return out


def put(ei, ea):
    return ei.to(DEV), ea.to(DEV)


@pytest.mark.parametrize("case", graphs(), ids=lambda c: c[0])
def test_layer_bits(conv, rounding, case):
    """Three epilogues x both edge-linear roundings on every graph: y has the existing eval
    path's bits; a graph past the degree limit is refused by layer_eval_ok instead."""
    name, ei, ea, n = case
    ei, ea = put(ei, ea)
    torch.manual_seed(n)
    x = torch.randn(n, 128, device=DEV)
    graph = get_graph(ei, ea.float(), n)
    if graph.max_in_degree > _lib.MP_FUSED_MAX_DEGREE:
        assert not layer_eval_ok(conv, x, graph)
        return
    assert layer_eval_ok(conv, x, graph), name
    for epi in EPIS:
        want = existing(conv, x, ei, ea, epi)
        got = layer_eval(conv, x, graph, epi)
        assert torch.equal(got, want), (name, epi, rel_err(got, want))


def test_degree_coverage():
    """The cases above do hold an isolated node, an in-degree of exactly 32 and no edges."""
    degs = {}
    for name, ei, ea, n in graphs():
        degs[name] = torch.bincount(ei[1], minlength=n) if ei.numel() else torch.zeros(n)
    assert any(int(d.max()) == 32 for d in degs.values())
    assert any(int(d.min()) == 0 and int(d.max()) > 0 for d in degs.values())
    assert any(int(d.max()) == 0 for d in degs.values())


@pytest.mark.parametrize("max_wg", (1, 2, 3, 0))
def test_rounds(conv, rounding, max_wg):
    """N = 200 (7 tiles, the last with 8 rows) on 1, 2, 3 workgroups and the kernel's own
    grid: 4, 2 and 2 rounds (a workgroup of three has no tile in the last), and one."""
    n = 200
    ei, ea = put(*knn_batch_graph(n, 6, 1, seed=n)[:2])
    torch.manual_seed(n)
    x = torch.randn(n, 128, device=DEV)
    graph = get_graph(ei, ea.float(), n)
    for epi in EPIS:
        want = existing(conv, x, ei, ea, epi)
        got = layer_eval(conv, x, graph, epi, max_workgroups=max_wg)
        assert torch.equal(got, want), (epi, max_wg, rel_err(got, want))


@pytest.mark.parametrize("loss,grad_u", KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("n", (33, 200))
def test_head(conv, loss, grad_u, n):
    """As the last layer with each loss kind and targets holding NaNs: pred, raw and the
    valid-target counts equal head.head(...) on the existing layer's output, with y and with
    y = NULL; one workgroup walking every round as well."""
    kind = fused_head.loss_kind(loss, grad_u)
    K = fused_head.K_OF[kind]
    torch.manual_seed(K)
    lin = Linear(128, K).to(DEV)
    ei, ea = put(*knn_batch_graph(n, 6, 1, seed=n)[:2])
    x = torch.randn(n, 128, device=DEV)
    tgt = torch.rand(n, device=DEV)
    tgt[::7] = float("nan")
    graph = get_graph(ei, ea.float(), n)
    epi = _lib.EPI_RESIDUAL_RELU
    h = existing(conv, x, ei, ea, epi)
    with torch.no_grad():
        want = fused_head.head(h, lin, kind, tgt)
    rec = fused_head.record_of(want)
    assert rec.count_parts is not None
    for with_y, max_wg in ((True, 0), (False, 0), (False, 1)):
        plan = fused_head.plan(x, lin, kind, tgt)
        y = layer_eval(conv, x, graph, epi, head=plan, with_y=with_y, max_workgroups=max_wg)
        assert (y is None) == (not with_y)
        if with_y:
            assert torch.equal(y, h)
        assert torch.equal(plan.pred, want), (with_y, max_wg)
        assert torch.equal(plan.raw, rec.raw)
        assert torch.equal(plan.parts, rec.count_parts)
        assert int(plan.parts.sum()) == int((~tgt.isnan()).sum())


def test_redo_path(conv, rounding):
    """One +inf and one NaN in x at N = 33: their waves' split-bf16 chains give NaN and are
    redone in fp32 -- same bits, NaNs in the same places."""
    n = 33
    ei, ea = put(*knn_batch_graph(n, 6, 1, seed=n)[:2])
    torch.manual_seed(3)
    x = torch.randn(n, 128, device=DEV)
    x[5, 17] = float("inf")
    x[32, 100] = float("nan")
    graph = get_graph(ei, ea.float(), n)
    for epi in EPIS:
        want = existing(conv, x, ei, ea, epi)
        got = layer_eval(conv, x, graph, epi)
        assert want.isnan().any() and not want.isnan().all()
        assert same_bits(got, want), epi


def _entry_status(x, graph, D, deg):
    f = _lib.load().gine_mp_fwd_layer_eval
    p = x.data_ptr()
    return f(p, graph.in_rowptr.data_ptr(), graph.in_src.data_ptr(), graph.in_attr.data_ptr(),
             *([p] * 9), 1e-5, p, p, p, x.size(0), D, deg, 0, 1, None, 0, None)


def test_fallbacks():
    """layer_eval_ok is false for in-degree 33, D = 64, a BatchNorm without running statistics
    and one left in training mode (the entry refuses the first two); the Predictor then runs
    the existing path for those layers and still equals model.eval()(batch)."""
    from raincast_gnn.data import synthetic_batch
    conv = make_conv()
    ei, ea, n = knn_batch_graph(40, 32, 1, seed=2)     # in-degree 33 (k + the self loop)
    ei, ea = put(ei, ea)
    graph = get_graph(ei, ea.float(), n)
    x = torch.randn(n, 128, device=DEV)
    assert graph.max_in_degree == 33
    assert not layer_eval_ok(conv, x, graph)
    assert _entry_status(x, graph, 128, 33) == _lib.GINE_ERR_INVALID
    ei, ea = put(*knn_batch_graph(40, 6, 1, seed=2)[:2])
    graph = get_graph(ei, ea.float(), 40)
    conv64 = make_conv(D=64)
    x64 = torch.randn(40, 64, device=DEV)
    assert not layer_eval_ok(conv64, x64, graph)
    assert _entry_status(x64, graph, 64, 7) == _lib.GINE_ERR_DIM
    assert not layer_eval_ok(make_conv(track=False), x, graph)
    assert layer_eval_ok(conv, x, graph)
    conv.nn[1].train()
    assert not layer_eval_ok(conv, x, graph)

    def check(model, batch):
        with torch.no_grad():
            want = model.eval()(batch)
        for capture in (False, True):
            pred = Predictor(model, capture=capture, warmup=0)
            assert torch.equal(pred(batch), want), capture
    torch.manual_seed(4)
    small = synthetic_batch(60, 2, k=5, seed=1).to(DEV)
    check(GNN(35, 64, 64, 2, loss="NormalCRPS").to(DEV), small)
    dense = synthetic_batch(40, 2, k=33, seed=1).to(DEV)   # in-degree past the limit
    check(GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5).to(DEV), dense)
    model = GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="True", u=1.71, xi=0.5).to(DEV)
    bn = model.conv.convolutions[1].nn[1]
    model.conv.convolutions[1].nn[1] = BatchNorm1d(128, track_running_stats=False).to(DEV)
    check(model, synthetic_batch(60, 2, k=5, seed=1).to(DEV))
    model.conv.convolutions[1].nn[1] = bn
    check(model, synthetic_batch(60, 2, k=5, seed=1).to(DEV))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """test_eval_mode_prediction_and_ensemble_match_oracle's set-up: two checkpoints after a
    few optimizer steps each, 300 stations x 2 graphs, k = 8."""
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.optim import FlatAdamW
    batches = [synthetic_batch(300, 2, k=8, seed=s).to(DEV) for s in (11, 12)]
    states = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        model = make_gnn().to(DEV)
        opt = FlatAdamW(model.parameters(), lr=1e-3)
        model.train()
        for b in batches:
            opt.zero_grad()
            model.loss_fn.crps(model(b), b.y).backward()
            opt.step()
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    return batches, states


def make_gnn():
    return GNN(35, 128, 128, 4, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)


def test_whole_model(trained):
    from raincast_gnn.evaluate import predict_ensemble
    batches, states = trained
    model = make_gnn().to(DEV)
    model.load_state_dict(states[0])
    with torch.no_grad():
        want = [[None, None], [None, None]]
        for c, st in enumerate(states):
            model.load_state_dict(st)
            want[c] = [model.eval()(b).clone() for b in batches]
    model.load_state_dict(states[0])
    eager = Predictor(model, capture=False)
    captured = Predictor(model, capture=True, warmup=1)
    for _ in range(3):   # eager warm-up call, the capture, a replay
        for b, w in zip(batches, want[0]):
            assert torch.equal(eager(b), w)
        # the batches share N but not the edge list: one capture per (edge_index object, N)
        for b, w in zip(batches, want[0]):
            assert torch.equal(captured(b), w)
    assert len(captured._graphs) == 2
    for b in batches:
        static = captured._graphs[(id(b.edge_index), b.x.size(0))][1]
        assert static.edge_index is b.edge_index and static.x is not b.x
    # the same edges in another tensor object: not what was captured, so the eager result
    import copy
    other = copy.copy(batches[0])
    other.edge_index = batches[0].edge_index.clone()
    assert torch.equal(captured(other), want[0][0])
    assert len(captured._graphs) == 2
    # in-place reload of the second checkpoint: the next replays see it, no re-capture
    ids_before = {k: id(v[0]) for k, v in captured._graphs.items()}
    model.load_state_dict(states[1])
    for b, w in zip(batches, want[1]):
        assert torch.equal(captured(b), w)
        assert torch.equal(eager(b), w)
    assert {k: id(v[0]) for k, v in captured._graphs.items()} == ids_before
    # the oracle in eval mode, at the bar the existing eval test uses
    ref = O.OracleGNN(35, 128, 4, "MixedLoss", "False", 1.71, 0.5)
    ref.load_state_dict({k: v.cpu() for k, v in states[1].items()})
    ref.eval()
    with torch.no_grad():
        r = ref(batches[0].to("cpu"))
    e_new, e_old = rel_err(captured(batches[0]), r), rel_err(want[1][0], r)
    print(f"rel_err vs oracle: predictor {e_new:.3e}, existing path {e_old:.3e}")
    assert e_new <= 1e-5
    # the checkpoint ensemble
    cpu_states = [{k: v.cpu() for k, v in st.items()} for st in states]
    a = predict_ensemble(make_gnn, cpu_states, batches, DEV)
    b = predict_ensemble(make_gnn, cpu_states, batches, DEV, fused=True)
    assert torch.equal(a, b)
    # a parameter whose storage moved drops the captures
    model.aggr.weight.data = model.aggr.weight.data.clone()
    assert torch.equal(captured(batches[0]), want[1][0])
    assert len(captured._graphs) == 0


def test_capture_owns_its_graph(trained):
    """A capture holds the GineGraph whose CSR pointers its launches carry: after the graph
    cache is cleared and the freed sizes are allocated again and overwritten, the replay still
    gives the eager bits; and the captures are bounded (max_captures, least recently used)."""
    import copy
    from raincast_gnn import graph_cache
    batches, states = trained
    model = make_gnn().to(DEV)
    model.load_state_dict(states[0])
    b0 = batches[0]
    with torch.no_grad():
        want = model.eval()(b0).clone()
    pred = Predictor(model, capture=True, warmup=0, max_captures=2)
    assert torch.equal(pred(b0), want)
    cap = pred._graphs[(id(b0.edge_index), b0.x.size(0))]
    held = cap[3]
    assert held and all(g.in_rowptr.is_cuda for g in held)
    sizes = [(t.numel(), t.dtype) for g in held for t in (g.in_rowptr, g.in_src, g.in_attr)]
    graph_cache.clear()
    torch.cuda.synchronize()
    # what the allocator would hand out had the CSRs been freed: same sizes, overwritten (with
    # in-bounds values: zero row pointers and indices would give other predictions, no fault)
    junk = [torch.full((n,), 0 if dt != torch.float32 else 7.0, dtype=dt, device=DEV)
            for n, dt in sizes for _ in range(4)]
    assert torch.equal(pred(b0), want)            # the replay
    assert pred._graphs[(id(b0.edge_index), b0.x.size(0))] is cap
    del junk
    # two more edge lists: the oldest capture leaves
    for _ in range(2):
        other = copy.copy(b0)
        other.edge_index = b0.edge_index.clone()
        assert torch.equal(pred(other), want)
    assert len(pred._graphs) == 2 and (id(b0.edge_index), b0.x.size(0)) not in pred._graphs


def test_no_side_effects_and_launch_count(trained, monkeypatch):
    """Parameters, running statistics and num_batches_tracked are bit-unchanged by Predictor
    calls, and a forward is front + 4 launches (every _lib.call that launches is counted)."""
    batches, states = trained
    model = make_gnn().to(DEV)
    model.load_state_dict(states[0])
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pred = Predictor(model, capture=False)
    pred(batches[0])                      # the graph's CSR is built here, not counted below
    names = []
    real = _lib.call

    def counting(name, *a):
        names.append(name)
        return real(name, *a)
    for mod in (_lib, functional, fused_head):
        monkeypatch.setattr(mod, "call", counting, raising=False)
    import raincast_gnn.chain
    import raincast_gnn.deepset
    import raincast_gnn.inference
    for mod in (raincast_gnn.chain, raincast_gnn.deepset, raincast_gnn.inference,
                raincast_gnn.inference._lib):
        if hasattr(mod, "call"):
            monkeypatch.setattr(mod, "call", counting)
    pred(batches[0])
    layers = [n for n in names if n == "gine_mp_fwd_layer_eval"]
    front = [n for n in names if n.startswith(("gine_deepset_fwd", "gine_chain_fwd"))]
    others = [n for n in names if n not in layers and n not in front]
    assert len(layers) == 4 and len(front) == 2, names
    assert not [n for n in others if "fwd" in n or "head" in n or "mp_" in n], names
    Predictor(model, capture=True, warmup=0)(batches[0])
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
