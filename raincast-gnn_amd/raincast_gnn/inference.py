"""Inference on the engine: the eval-mode GINE layer in one launch, and a captured forward.

In eval mode BatchNorm is a per-channel affine map known before the launch, so a whole GINE
layer -- message passing, Linear, BatchNorm, ReLU, Linear, ResGnn's epilogue and, on the last
layer, the output head -- is one launch of ``gine_mp_fwd_layer_eval`` with no grid barrier
(include/gine_hip.h).  It writes the layer's output (or only the predictions) and nothing a
backward would need, and gives the bits of the separate eval launches ``GINEConv`` makes.

* :func:`layer_eval` / :func:`layer_eval_ok` -- that launch for one ``GINEConv``, and whether
  it applies (every in-degree within GINE_MP_FUSED_MAX_DEGREE).
* :func:`layer_eval_deep` / :func:`layer_eval_deep_ok` -- ``gine_mp_fwd_layer_eval_deep``: the
  same launch at any in-degree (radius graphs, k = 32 plus the self loop), same bits.
* :class:`Predictor` -- ``model.eval()(batch)`` under ``no_grad`` with every layer on it
  (front + one launch per layer), captured into one HIP graph per batch shape.

``evaluate.predict_model(..., fused=True)`` and ``predict_ensemble(..., fused=True)`` run on a
``Predictor``; the ensemble loads every checkpoint into one model in place, so one capture
serves all of them.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from . import _lib
from . import head as fused_head
from .data import GraphBatch
from .functional import EPI_RELU, EPI_RESIDUAL_RELU, edge_linear_flag
from .graph import get_graph
from .linear import Linear as RowLinear

CHANNELS = 128  # gine_mp_fwd_layer_eval's only width
# The largest N at which the Predictor takes the deep launch by default (None: no limit).  Past
# some N each workgroup walks many rounds and stages W1 / W2 again in every one, and the
# separate launches win.  Measured with tools/infer_bench.py --force-deep --separate (DESIGN.md
# 6a, profiles/r08_infer_bench_*.txt): up to N = 40,000 (in-degree 33) the Predictor with the
# deep launch is faster than with the separate launches in both forms, and than
# model.eval()(batch) in at least one; at N = 64,000 (radius graph, in-degree <= 45) it is 2.5 %
# slower than the separate launches and at N = 80,000 (cfg5) it ties them.
DEEP_MAX_NODES = 40_000


def _layer_eval_common(conv, x: torch.Tensor, graph) -> bool:
    """Every condition of the one-launch eval layer but the in-degree."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2
            and x.dtype == torch.float32 and x.size(1) == CHANNELS):
        return False
    if not conv._fusable(x):
        return False
    lin = conv.lin
    if lin is None or lin.in_features != 1 or lin.out_features != CHANNELS or lin.bias is None:
        return False
    if (graph.in_attr is None or graph.max_in_degree is None
            or graph.num_nodes != x.size(0) or x.size(0) * CHANNELS * 4 >= 1 << 32):
        return False
    bn = conv.nn[1]
    return not bn.training and bn.running_mean is not None and bn.running_var is not None


def layer_eval_ok(conv, x: torch.Tensor, graph) -> bool:
    """``gine_mp_fwd_layer_eval`` applies to ``conv`` on ``x``: the fusable node MLP at D = 128
    on a HIP device, an edge Linear(1, D) and edge attributes, every in-degree within
    GINE_MP_FUSED_MAX_DEGREE, and a BatchNorm in eval mode that has running statistics."""
    return (_layer_eval_common(conv, x, graph)
            and graph.max_in_degree <= _lib.MP_FUSED_MAX_DEGREE)


def layer_eval_deep_ok(conv, x: torch.Tensor, graph) -> bool:
    """``gine_mp_fwd_layer_eval_deep`` applies: :func:`layer_eval_ok`'s conditions without the
    degree limit."""
    return _layer_eval_common(conv, x, graph)


def layer_eval(conv, x: torch.Tensor, graph, epilogue: int, head=None, max_workgroups: int = 0,
               with_y: bool = True):
    """One eval-mode layer of ``conv`` on ``x`` in one launch: ``y = epilogue(nn(z))`` with
    BatchNorm from its running statistics (no autograd; the caller checked
    :func:`layer_eval_ok`).  ``head``: a ``head.HeadPlan`` whose raw / pred (and valid-target
    counts) the launch also writes; then ``with_y=False`` skips ``y`` and returns None.
    ``max_workgroups``: a cap on the grid (0: the kernel's choice).  Allocates ``y`` only."""
    return _layer_launch("gine_mp_fwd_layer_eval", conv, x, graph, epilogue, head,
                         max_workgroups, with_y)


def layer_eval_deep(conv, x: torch.Tensor, graph, epilogue: int, head=None,
                    max_workgroups: int = 0, with_y: bool = True):
    """:func:`layer_eval` at any in-degree (``gine_mp_fwd_layer_eval_deep``; the caller checked
    :func:`layer_eval_deep_ok`): same arguments, same contract, same bits."""
    return _layer_launch("gine_mp_fwd_layer_eval_deep", conv, x, graph, epilogue, head,
                         max_workgroups, with_y)


def _layer_launch(entry: str, conv, x, graph, epilogue, head, max_workgroups, with_y):
    x = x.contiguous()
    N, D = x.shape
    y = torch.empty_like(x) if (with_y or head is None) else None
    if N == 0:
        return y
    l1, bn, _, l2 = conv.nn
    hargs = head.args(N, D, x.device) if head is not None else None
    if head is not None and hargs is None:
        raise ValueError("layer_eval: the head plan was made for another shape or device")
    # the operands as they lie in memory (host time: no views or copies of contiguous
    # parameters); the list keeps a rare contiguous copy alive until the launch is enqueued
    ops = [_dense(t) for t in (conv.lin.weight, conv.lin.bias, conv.eps, l1.weight, l1.bias,
                               bn.weight, bn.bias, bn.running_mean, bn.running_var, l2.weight,
                               l2.bias)]
    lw, lb, ep, w1, b1, g, bt, rm, rv, w2, b2 = (_lib.ptr(t) for t in ops)
    _lib.call(entry, x.data_ptr(), graph.in_rowptr.data_ptr(),
              graph.in_src.data_ptr(), graph.in_attr.data_ptr(), lw, lb, ep, w1, b1, g, bt, rm,
              rv, bn.eps, w2, b2, _lib.ptr(y), N, D, graph.max_in_degree, edge_linear_flag(),
              epilogue, ctypes.byref(hargs) if hargs is not None else None, max_workgroups,
              _lib.stream_handle(x.device))
    return y


def _dense(t):
    return t if t is None or t.is_contiguous() else t.detach().contiguous()


class Predictor:
    """``predictor(batch)`` = ``model.eval()(batch)`` under ``no_grad``: the ``[N, K]``
    predictions in the batch's stored order, with the same bits.

    The front runs on the DeepSet and chain kernels ``GNN`` uses; every GINE layer is one
    ``gine_mp_fwd_layer_eval`` launch, the last one carrying the output head (front + one launch
    per layer).  On a graph past that launch's degree limit the layers run
    ``gine_mp_fwd_layer_eval_deep`` instead, up to ``DEEP_MAX_NODES`` nodes.  A layer or head
    neither launch covers runs the path ``GNN.forward`` takes, and a model that is not on a HIP
    device is simply called.

    ``capture=True`` (HIP devices): after ``warmup`` eager calls with one (``edge_index``
    object, N), the forward for it is captured into one HIP graph and replayed with ``x`` and
    ``ensemble`` copied into its static inputs.  The edge list is recognised by identity, so a
    loader has to hand out the same device-resident ``edge_index`` / ``edge_attr`` tensors again
    to be replayed (``batching.DeviceDataset`` does; host batches moved with ``.to(device)`` are
    new tensors every time and always run eager).  At most ``max_captures`` edge lists are
    tracked, least recently used first out.  A capture owns what it reads: its static inputs
    and the ``GineGraph`` CSRs, whatever the graph cache does later.  The graphs read the
    parameters' storage, so ``load_state_dict`` (an in-place copy) is seen by the next replay;
    if any parameter's or buffer's storage pointer changed, the captures are dropped."""

    def __init__(self, model: torch.nn.Module, capture: bool = True, warmup: int = 1,
                 max_captures: int = 8):
        self.model = model.eval()
        self.capture, self.warmup, self.max_captures = capture, warmup, max_captures
        # (id(edge_index), N) -> [edge_index, edge_attr, calls, capture | None]; the slot holds
        # the tensors, so an id stays theirs while it is a key
        self._slots: OrderedDict = OrderedDict()
        self._ptrs = None

    @property
    def _graphs(self) -> dict:
        """The live captures: key -> (HIP graph, static batch, output, GineGraphs held)."""
        return {k: s[3] for k, s in self._slots.items() if s[3] is not None}

    # -- the forward ---------------------------------------------------------------------
    def _forward(self, batch, keep: list | None = None) -> torch.Tensor:
        """``keep``: a list the GineGraphs this forward reads are appended to."""
        m = self.model
        if not batch.x.is_cuda or not self._is_gnn():
            return m(batch)
        stack = m.conv.convolutions
        x = m._front(batch).float()
        ei, ea = batch.edge_index, batch.edge_attr.float()
        kind = fused_head.loss_kind(m.postprocess.loss, m.postprocess.grad_u)
        head_ok = (type(m.aggr) in (RowLinear, torch.nn.Linear)  # (GNN.forward's condition)
                   and fused_head.fusable(x, m.aggr, kind))
        last = len(stack) - 1
        by_flow = {}  # one cache lookup per forward, not per layer
        for i, conv in enumerate(stack):
            epi = EPI_RELU if i == 0 else EPI_RESIDUAL_RELU
            graph = None
            if conv.lin is not None:
                graph = by_flow.get(conv.flow)
                if graph is None:
                    graph = by_flow[conv.flow] = get_graph(ei, ea, x.size(0), conv.flow)
                    if keep is not None:
                        keep.append(graph)
            run = None
            if graph is not None:
                if layer_eval_ok(conv, x, graph):
                    run = layer_eval
                elif ((DEEP_MAX_NODES is None or x.size(0) <= DEEP_MAX_NODES)
                      and layer_eval_deep_ok(conv, x, graph)):
                    run = layer_eval_deep
            if run is not None:
                if i == last and head_ok:  # predictions only: the last layer's y is not stored
                    plan = fused_head.plan(x, m.aggr, kind, None)
                    run(conv, x, graph, epi, head=plan, with_y=False)
                    return plan.pred
                x = run(conv, x, graph, epi)
            elif i == 0:
                x = conv.forward_relu(x, ei, ea)
            else:
                x = conv.forward_residual_relu(x, ei, ea)
        if head_ok:
            return fused_head.head(x, m.aggr, kind, None)
        return m.postprocess(m.aggr(x))

    def _is_gnn(self) -> bool:
        """The model has models.GNN's parts (front, GINE stack, aggr, postprocess)."""
        m = self.model
        return (getattr(getattr(m, "conv", None), "convolutions", None) is not None
                and all(hasattr(m, a) for a in ("_front", "aggr", "postprocess")))

    def _storage_ptrs(self) -> tuple:
        m = self.model
        return tuple(t.data_ptr() for t in m.parameters()) + tuple(
            t.data_ptr() for t in m.buffers())

    @torch.no_grad()
    def __call__(self, batch: GraphBatch) -> torch.Tensor:
        self.model.eval()
        if not self.capture or not batch.x.is_cuda or not self._is_gnn():
            return self._forward(batch)  # (another model's forward is never captured)
        ptrs = self._storage_ptrs()
        if ptrs != self._ptrs:  # a parameter moved: what was captured reads freed storage
            self._slots.clear()
            self._ptrs = ptrs
        key = (id(batch.edge_index), batch.x.size(0))
        slot = self._slots.get(key)
        if slot is None or slot[0] is not batch.edge_index or slot[1] is not batch.edge_attr:
            slot = self._slots[key] = [batch.edge_index, batch.edge_attr, 0, None]
            while len(self._slots) > max(self.max_captures, 1):
                self._slots.popitem(last=False)
        self._slots.move_to_end(key)
        slot[2] += 1
        if slot[2] <= self.warmup:
            return self._forward(batch)
        if slot[3] is None:
            slot[3] = self._capture(batch)
        graph, static, out, _ = slot[3]
        if static.x.shape != batch.x.shape or static.ensemble.shape != batch.ensemble.shape:
            return self._forward(batch)  # not what was captured
        static.x.copy_(batch.x)
        static.ensemble.copy_(batch.ensemble)
        graph.replay()
        return out.clone()

    @torch.no_grad()
    def bind(self, batch: GraphBatch) -> "BoundForward":
        """A handle on the forward of ``batch``'s (``edge_index`` object, N): its static ``x``
        and ``ensemble`` are written in place by the caller and ``run()`` returns the static
        output, so a loop that assembles its own batches pays no copy around the replay.  The
        warm-up calls and the capture happen here if they have not happened yet; the capture is
        the one ``predictor(batch)`` replays for this edge list, so a call to it overwrites the
        handle's inputs."""
        self.model.eval()
        return BoundForward(self, batch)

    def _bound_capture(self, batch, static=None) -> tuple | None:
        """The live capture for ``batch`` -- warmed up and captured now if need be, into
        ``static``'s tensors when given -- or None where ``__call__`` would not capture."""
        if not self.capture or not batch.x.is_cuda or not self._is_gnn():
            return None
        ptrs = self._storage_ptrs()
        if ptrs != self._ptrs:
            self._slots.clear()
            self._ptrs = ptrs
        key = (id(batch.edge_index), batch.x.size(0))
        slot = self._slots.get(key)
        if slot is None or slot[0] is not batch.edge_index or slot[1] is not batch.edge_attr:
            slot = self._slots[key] = [batch.edge_index, batch.edge_attr, 0, None]
            while len(self._slots) > max(self.max_captures, 1):
                self._slots.popitem(last=False)
        self._slots.move_to_end(key)
        while slot[2] < self.warmup:
            self._forward(batch)
            slot[2] += 1
        if slot[3] is None or static is not None:
            slot[3] = self._capture(batch, static)
        return slot[3]

    def _capture(self, batch, static=None) -> tuple:
        if static is None:
            static = GraphBatch(batch.x.clone(), batch.ensemble.clone(), batch.edge_index,
                                batch.edge_attr, batch.y, batch.batch, batch.ptr,
                                batch.num_graphs, dict(batch.extra))
        self._forward(static)  # the graph's CSR and every size query exist before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        held: list = []  # the GineGraphs whose CSR pointers the captured launches carry
        with torch.cuda.graph(graph):
            out = self._forward(static, held)
        return graph, static, out, held


class BoundForward:
    """What :meth:`Predictor.bind` returns: ``x [N, F]`` and ``ensemble [N, M, F]`` are the
    forward's inputs, to be filled in place; ``run()`` computes ``predictor(batch)`` of what they
    hold and returns the output tensor itself, valid until the next ``run``.

    On a captured forward ``run()`` is one graph replay.  With ``capture=False``, or a model the
    Predictor does not capture, the handle owns plain buffers and ``run()`` calls the forward on
    them.  When a parameter's or buffer's storage has moved since the capture, ``run()`` captures
    again into the same input tensors first (an in-place ``load_state_dict`` needs nothing)."""

    def __init__(self, predictor: Predictor, batch: GraphBatch):
        self._predictor = predictor
        cap = predictor._bound_capture(batch)
        if cap is not None and (cap[1].x.shape != batch.x.shape
                                or cap[1].ensemble.shape != batch.ensemble.shape):
            raise ValueError("bind: this edge list was captured with inputs of another shape")
        self._set(cap)
        if cap is None:
            self._static = GraphBatch(batch.x.clone(), batch.ensemble.clone(), batch.edge_index,
                                      batch.edge_attr, batch.y, batch.batch, batch.ptr,
                                      batch.num_graphs, dict(batch.extra))
            self.out = None

    def _set(self, cap) -> None:
        self._cap = cap
        if cap is not None:
            self._graph, self._static, self.out = cap[0], cap[1], cap[2]
            self._ptrs = self._predictor._ptrs

    @property
    def captured(self) -> bool:
        return self._cap is not None

    @property
    def x(self) -> torch.Tensor:
        return self._static.x

    @property
    def ensemble(self) -> torch.Tensor:
        return self._static.ensemble

    @torch.no_grad()
    def run(self) -> torch.Tensor:
        p = self._predictor
        p.model.eval()
        if self._cap is None:
            self.out = p._forward(self._static)
            return self.out
        if p._storage_ptrs() != self._ptrs:  # what was captured reads freed storage
            self._set(p._bound_capture(self._static, self._static))
        self._graph.replay()
        return self.out


def predictor_for(model: torch.nn.Module) -> Predictor:
    """The model's own :class:`Predictor` (made on first use and kept on the model, outside its
    state_dict), so that repeated ``predict_model(..., fused=True)`` calls share its captures."""
    pred = model.__dict__.get("_raincast_predictor")
    if pred is None or pred.model is not model:
        pred = model.__dict__["_raincast_predictor"] = Predictor(model)
    return pred
