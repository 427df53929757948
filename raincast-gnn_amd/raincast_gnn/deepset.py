"""Fused DeepSet phi head: ``sum_m relu(phi[0](ens[:, m]))`` on one HIP kernel pair.

models/gnn.py:48-68 evaluates ``phi = Sequential(Linear(F, H), ReLU(), Linear(H, H))`` on
every (station, member) row and sums over members.  :class:`~raincast_gnn.models.
DeepSetEncoder` moves the member sum before ``phi[2]`` (a Linear commutes with a sum); what
remains, ``r = sum_m relu(ens W1^T + b1)``, is the ``[N, M, H]`` activation the reference
materialises three times per training step (90 MB each at the 24h_mixed benchmark shape).
``gine_deepset_fwd`` keeps it in MFMA accumulators and writes only ``r [N, H]``;
the forward also records its ReLU pattern as bits (2.8 MB instead of 90 MB), from which
``gine_deepset_bwd`` produces dW1/db1 directly (csrc/gine_deepset.hip).  The ensemble tensor is data (never requires grad in the
reference); a caller that needs d/d(ens) gets the unfused torch path.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import gradbuf
from .gradbuf import grad_out

HIDDEN = (32, 64, 128, 256)
MAX_FEATURES = 64


def fusable(ens: torch.Tensor, weight: torch.Tensor, bias) -> bool:
    return (ens.is_cuda and ens.dim() == 3 and ens.dtype == torch.float32
            and weight.dtype == torch.float32 and bias is not None
            and weight.size(0) in HIDDEN and 0 < weight.size(1) <= MAX_FEATURES
            and ens.size(2) == weight.size(1) and ens.size(1) > 0
            and not ens.requires_grad)


class _PhiSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ens, weight, bias, fold=None):
        """``fold`` = weight, bias of rho[2], dim_red, rho[0], phi[2]: the same launch also
        folds the dense chain's weights (gine_deepset_fwd_fold2) and the function returns
        (r, wfold), wfold = [W' | b' | W'^T] then [Wf | bf], not differentiable."""
        ens = ens.contiguous()
        weight, bias = weight.contiguous(), bias.contiguous()
        N, M, Fdim = ens.shape
        H = weight.size(0)
        r = torch.empty(N, H, dtype=torch.float32, device=ens.device)
        mask = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            nbytes = ctypes.c_size_t(0)
            _lib.call("gine_deepset_mask_bytes", N, M, H, ctypes.byref(nbytes))
            mask = torch.empty(nbytes.value, dtype=torch.uint8, device=ens.device)
        ctx.save_for_backward(ens, mask)
        ctx.params = (weight, bias)
        ctx.hidden = H
        stream = _lib.stream_handle(ens.device)
        if fold is None:
            _lib.call("gine_deepset_fwd", _lib.ptr(ens), _lib.ptr(weight), _lib.ptr(bias),
                      _lib.ptr(r), _lib.ptr(mask), N, M, Fdim, H, stream)
            return r
        wr1, br1, wdr, bdr, wr0, br0, wp2, bp2 = (t.detach().contiguous() for t in fold)
        F = wdr.size(1) - H
        n1 = 2 * H * (F + H) + H
        P = _lib.ptr
        wfold = torch.empty(n1 + H * H + H, dtype=torch.float32, device=ens.device)
        _lib.call("gine_deepset_fwd_fold2", P(ens), P(weight), P(bias), P(r), P(mask), N, M,
                  Fdim, H, P(wr1), P(br1), P(wdr), P(bdr), P(wfold), F, P(wr0), P(br0),
                  P(wp2), P(bp2), P(wfold[n1:]), stream)
        ctx.mark_non_differentiable(wfold)
        # no zero-filled gradient for wfold in the backward (a fill launch per step)
        ctx.set_materialize_grads(False)
        return r, wfold

    @staticmethod
    def backward(ctx, dr, *unused):
        ens, mask = ctx.saved_tensors
        if dr is None:  # (grads are not materialised in the folding form)
            return None, None, None, None
        N, M, Fdim = ens.shape
        H = ctx.hidden
        dr = dr.contiguous()
        parts = ctypes.c_int32(0)
        _lib.call("gine_deepset_bwd_num_partials", N, H, ctypes.byref(parts))
        slab = torch.empty(parts.value * (H * Fdim + H), dtype=torch.float32, device=dr.device)
        dw = grad_out(ctx.params[0], (H, Fdim), dr.device)
        db = grad_out(ctx.params[1], (H,), dr.device)
        defer = gradbuf.deferrable(dw, db)  # slab reduced in the end-of-backward batch
        _lib.call("gine_deepset_bwd", _lib.ptr(ens), _lib.ptr(mask), _lib.ptr(dr),
                  _lib.ptr(slab), None if defer else _lib.ptr(dw),
                  None if defer else _lib.ptr(db), N, M, Fdim, H,
                  _lib.stream_handle(dr.device))
        if defer:
            job = _lib.GradJob()
            _lib.call("gine_deepset_bwd_grad_job", N, Fdim, H, _lib.ptr(slab), _lib.ptr(dw),
                      _lib.ptr(db), ctypes.byref(job))
            gradbuf.defer(job, dr.device, (slab,))
        return None, dw, db, None


class EncLink:
    """What the two autograd nodes of the fused encoder backward (``chain.encoder``) share:
    the DeepSet node's operands for the chain node, whose backward launch
    (gine_deepset_bwd_chain) also produces phi[0]'s gradients, and those gradients on their
    way back to the DeepSet node, which returns them to autograd."""

    def __init__(self):
        self.ens = self.mask = self.params = None
        self._grads = None

    def put(self, dw, db):
        self._grads = (dw, db)

    def take(self):
        g, self._grads = self._grads, None
        return g


class _PhiSumEncFn(_PhiSumFn):
    """:class:`_PhiSumFn` in its folding form, as the DeepSet node of the fused encoder
    backward: the chain node (``chain._ChainFolded2FnEnc``) runs the backward launch for both
    and leaves dW1 / db1 in ``link``; this node gets no dr and only hands them on.  A dr that
    does arrive without them (the chain node did not run) takes the DeepSet backward launch."""

    @staticmethod
    def forward(ctx, ens, weight, bias, fold, link):
        out = _PhiSumFn.forward(ctx, ens, weight, bias, fold)
        ctx.link = link
        link.ens, link.mask = ctx.to_save
        link.params = ctx.params
        assert link.mask is not None
        return out

    @staticmethod
    def backward(ctx, dr, *unused):
        grads = ctx.link.take()
        if grads is None:
            return (*_PhiSumFn.backward(ctx, dr, *unused), None)
        if dr is not None:
            raise RuntimeError("r of the fused encoder has a consumer beside the chain")
        return None, grads[0], grads[1], None, None


def phi_sum(ens: torch.Tensor, lin1: torch.nn.Linear, fold=None):
    """``relu(lin1(ens)).sum(dim=1)`` for ens [N, M, F] on the fused kernels; with
    ``fold`` = the (rho[2], dim_red, rho[0], phi[2]) Linears, (r, wfold) for the dense chain
    (:func:`raincast_gnn.chain.chain`)."""
    if fold is None:
        return _PhiSumFn.apply(ens, lin1.weight, lin1.bias)
    if len(fold) != 4:
        raise ValueError("fold = (rho[2], dim_red, rho[0], phi[2])")
    return _PhiSumFn.apply(ens, lin1.weight, lin1.bias,
                           tuple(t for m in fold for t in (m.weight, m.bias)))
