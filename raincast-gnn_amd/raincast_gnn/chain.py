"""Fused dense layers between the DeepSet member sum and the GINE stack.

models/gnn.py:132-135 computes ``dim_red(cat([x, DeepSetEncoder(ensemble)], 1))``; after the
fused member sum ``r = sum_m relu(phi[0](ens_m))`` (:mod:`.deepset`) what remains is four
dense Linears and a ReLU on [N, D] rows::

    s = phi[2](r) (bias x M)  ->  u = relu(rho[0](s))  ->  e = rho[2](u)  ->  h0 = dim_red([x | e])

Only the ReLU separates them, so the chain runs doubly folded (csrc/gine_chain.hip)::

    u = relu(r Wf^T + bf)  ->  h0 = [x | u] W'^T + b'

with ``Wf = Wr0 Wp2``, ``bf = M Wr0 bp2 + br0``, ``W' = [Wdr_x | Wdr_e Wr1]`` and
``b' = Wdr_e br1 + bdr`` folded from the current weights by the DeepSet launch
(``deepset.phi_sum(..., fold=...)``).  ``FOLD = False`` runs the unfolded chain instead
(``gine_chain_fwd`` / ``gine_chain_bwd``: two 2-stage kernels each way, four weight-gradient
products): slower, kept as the comparator of the tests.  Modules, parameters and state_dict
keys are the reference's; this is only the execution of ``GNN.forward``'s first half.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, deepset, gradbuf
from .gradbuf import grad_out

HIDDEN = (64, 128)
MAX_FEATURES = 64


def fusable(r: torch.Tensor, x: torch.Tensor, lins) -> bool:
    return r.is_cuda and r.dtype == torch.float32 and fusable_dims(r.size(1), x, lins)


def fusable_dims(D: int, x: torch.Tensor, lins) -> bool:
    """The chain's conditions on everything but r (r [N, D] fp32 on the device)."""
    p2, r0, r1, dr = lins
    F = x.size(1)
    shapes = ((p2, D, D), (r0, D, D), (r1, D, D), (dr, F + D, D))
    return (x.is_cuda and x.dtype == torch.float32
            and D in HIDDEN and 0 < F <= MAX_FEATURES and not x.requires_grad
            and all(isinstance(m, torch.nn.Linear) and m.bias is not None
                    and m.weight.dtype == torch.float32 and m.in_features == i
                    and m.out_features == o for m, i, o in shapes))


class _ChainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, x, wp2, bp2, wr0, br0, wr1, br1, wdr, bdr, members):
        r = r.contiguous()
        x = x.contiguous()
        N, D = r.shape
        F = x.size(1)
        dev = r.device
        ws = [t.detach().contiguous() for t in (wp2, bp2, wr0, br0, wr1, br1, wdr, bdr)]
        s, u, e, h0 = (torch.empty(N, D, dtype=torch.float32, device=dev) for _ in range(4))
        P = _lib.ptr
        _lib.call("gine_chain_fwd", P(r), P(x), P(ws[0]), P(ws[1]), float(members), P(ws[2]),
                  P(ws[3]), P(ws[4]), P(ws[5]), P(ws[6]), P(ws[7]), P(s), P(u), P(e), P(h0),
                  N, D, F, _lib.stream_handle(dev))
        ctx.save_for_backward(r, x, s, u, e, ws[0], ws[2], ws[4], ws[6])
        ctx.params = (wp2, bp2, wr0, br0, wr1, br1, wdr, bdr)
        ctx.members = float(members)
        return h0

    @staticmethod
    def backward(ctx, dh0):
        r, x, s, u, e, wp2, wr0, wr1, wdr = ctx.saved_tensors
        N, D = r.shape
        F = x.size(1)
        dev = r.device
        dh0 = dh0.contiguous()
        de, dt, ds, dr = (torch.empty(N, D, dtype=torch.float32, device=dev) for _ in range(4))
        floats = ctypes.c_size_t(0)
        _lib.call("gine_chain_bwd_slab_floats", N, D, F, ctypes.byref(floats))
        slab = torch.empty(floats.value, dtype=torch.float32, device=dev)
        p = ctx.params
        g = [grad_out(p[0], (D, D), dev), grad_out(p[1], (D,), dev),
             grad_out(p[2], (D, D), dev), grad_out(p[3], (D,), dev),
             grad_out(p[4], (D, D), dev), grad_out(p[5], (D,), dev),
             grad_out(p[6], (D, F + D), dev), grad_out(p[7], (D,), dev)]
        P = _lib.ptr
        # input gradients (de, dt, ds -> dr) on the current stream: the DeepSet backward
        # needs dr next ...
        _lib.call("gine_chain_bwd", P(dh0), P(x), P(r), P(s), P(u), P(e), P(wp2), P(wr0),
                  P(wr1), P(wdr), P(de), P(dt), P(ds), P(dr), None, None, None, ctx.members,
                  None, None, None, None, None, None, N, D, F, _lib.stream_handle(dev))
        members = ctx.members
        if gradbuf.deferrable(*g):
            # the engine leaves its slab; the end-of-backward batch reduces it
            _lib.call("gine_chain_wgrad", P(dh0), P(x), P(r), P(s), P(u), P(e), P(de),
                      P(dt), P(ds), P(slab), None, None, members, None, None, None, None,
                      None, None, N, D, F, _lib.stream_handle(dev))
            job = _lib.GradJob()
            _lib.call("gine_chain_wgrad_grad_job", N, D, F, P(slab), members, P(g[0]),
                      P(g[1]), P(g[2]), P(g[3]), P(g[4]), P(g[5]), P(g[6]), P(g[7]),
                      ctypes.byref(job))
            gradbuf.defer(job, dev, (slab,))
            return (dr, None, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], None)
        # ... else the four weight gradients reduced in the same call
        _lib.call("gine_chain_wgrad", P(dh0), P(x), P(r), P(s), P(u), P(e), P(de), P(dt),
                  P(ds), P(slab), P(g[0]), P(g[1]), members, P(g[2]), P(g[3]), P(g[4]),
                  P(g[5]), P(g[6]), P(g[7]), N, D, F, _lib.stream_handle(dev))
        return (dr, None, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], None)


class _ChainFolded2Fn(torch.autograd.Function):
    """The doubly folded chain (gine_chain_fwd_folded2, include/gine_hip.h).  Neither s, e
    nor their gradients are formed: one 2-stage launch forward (u, h0), one backward
    (dt, dr), two weight-gradient products (G = dh0^T [x | u], G2 = dt^T r) unfolded into
    all eight chain gradients by one launch."""

    @staticmethod
    def forward(ctx, r, x, wp2, bp2, wr0, br0, wr1, br1, wdr, bdr, members, wfold):
        r = r.contiguous()
        x = x.contiguous()
        N, D = r.shape
        F = x.size(1)
        dev = r.device
        n1 = 2 * D * (F + D) + D
        wf1, wf2 = wfold[:n1], wfold[n1:]
        u, h0 = (torch.empty(N, D, dtype=torch.float32, device=dev) for _ in range(2))
        P = _lib.ptr
        _lib.call("gine_chain_fwd_folded2", P(r), P(x), P(wf1), P(wf2), P(u), P(h0), N, D, F,
                  _lib.stream_handle(dev))
        ws = [t.detach().contiguous() for t in (wp2, bp2, wr0, wr1, br1, wdr)]
        ctx.save_for_backward(r, x, u, wfold, *ws)
        ctx.params = (wp2, bp2, wr0, br0, wr1, br1, wdr, bdr)
        ctx.members = float(members)
        return h0

    @staticmethod
    def backward(ctx, dh0):
        r, x, u, wfold, wp2, bp2, wr0, wr1, br1, wdr = ctx.saved_tensors
        N, D = r.shape
        F = x.size(1)
        dev = r.device
        n1 = 2 * D * (F + D) + D
        wf1, wf2 = wfold[:n1], wfold[n1:]
        dh0 = dh0.contiguous()
        dt, dr = (torch.empty(N, D, dtype=torch.float32, device=dev) for _ in range(2))
        floats = ctypes.c_size_t(0)
        _lib.call("gine_chain_bwd_slab_floats", N, D, F, ctypes.byref(floats))
        slab = torch.empty(floats.value, dtype=torch.float32, device=dev)
        gf = torch.empty(D * (F + D) + D + D * D + D, dtype=torch.float32, device=dev)
        gfold, g2fold = gf[:D * (F + D) + D], gf[D * (F + D) + D:]
        p = ctx.params
        g = [grad_out(p[0], (D, D), dev), grad_out(p[1], (D,), dev),
             grad_out(p[2], (D, D), dev), grad_out(p[3], (D,), dev),
             grad_out(p[4], (D, D), dev), grad_out(p[5], (D,), dev),
             grad_out(p[6], (D, F + D), dev), grad_out(p[7], (D,), dev)]
        P = _lib.ptr
        stream = _lib.stream_handle(dev)
        # the input gradients (dt -> dr) first: the DeepSet backward needs dr next
        _lib.call("gine_chain_bwd_folded2", P(dh0), P(u), P(wf1), P(wf2), P(dt), P(dr), N, D, F,
                  stream)
        # raw pointers only: a reference to a gradient tensor held past this function would
        # stop autograd adopting it as param.grad (it copies a shared tensor)
        ptrs = (P(gfold), P(wr1), P(br1), P(wdr), P(g[6]), P(g[7]), P(g[4]), P(g[5]),
                P(g2fold), P(wp2), P(bp2), P(wr0), P(g[2]), P(g[3]), P(g[0]), P(g[1]),
                ctx.members)

        def unfold(st):
            _lib.call("gine_chain_unfold_grads2", *ptrs, D, F, st)

        if gradbuf.deferrable(*g):
            # the engine leaves its slab; the end-of-backward batch reduces it into G | G2,
            # then unfolds them
            _lib.call("gine_chain_wgrad_folded2", P(dh0), P(x), P(r), P(u), P(dt), P(slab), None,
                      None, N, D, F, stream)
            job = _lib.GradJob()
            _lib.call("gine_chain_wgrad_folded2_grad_job", N, D, F, P(slab), P(gfold),
                      P(g2fold), ctypes.byref(job))
            gradbuf.defer(job, dev, (slab, gf, wp2, bp2, wr0, wr1, br1, wdr), post=unfold)
        else:
            _lib.call("gine_chain_wgrad_folded2", P(dh0), P(x), P(r), P(u), P(dt), P(slab),
                      P(gfold), P(g2fold), N, D, F, stream)
            unfold(stream)
        return (dr, None, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], None, None)


class _ChainFolded2FnEnc(_ChainFolded2Fn):
    """:class:`_ChainFolded2Fn` for the shapes where the encoder's backward is one launch
    (``options.ENC_BWD_FUSED``, gine_deepset_bwd_chain).  Same forward and saved tensors; the
    backward makes dt and, on chip, dr inside the DeepSet backward launch, so it also
    produces phi[0]'s gradients: they reach the DeepSet node (``deepset._PhiSumEncFn``, which
    returns them to autograd) through ``link`` and r gets no gradient tensor.  The
    weight-gradient engine, which needs dt, follows the fused launch.  Same bits as the two
    Functions."""

    @staticmethod
    def forward(ctx, r, x, wp2, bp2, wr0, br0, wr1, br1, wdr, bdr, members, wfold, link):
        ctx.link = link
        return _ChainFolded2Fn.forward(ctx, r, x, wp2, bp2, wr0, br0, wr1, br1, wdr, bdr,
                                       members, wfold)

    @staticmethod
    def backward(ctx, dh0):
        r, x, u, wfold, wp2, bp2, wr0, wr1, br1, wdr = ctx.saved_tensors
        link = ctx.link
        ens, mask = link.ens, link.mask
        N, M, Fe = ens.shape
        D, F = r.size(1), x.size(1)
        dev = r.device
        n1 = 2 * D * (F + D) + D
        wf1, wf2 = wfold[:n1], wfold[n1:]
        dh0 = dh0.contiguous()
        dt = torch.empty(N, D, dtype=torch.float32, device=dev)
        floats = ctypes.c_size_t(0)
        _lib.call("gine_chain_bwd_slab_floats", N, D, F, ctypes.byref(floats))
        slab = torch.empty(floats.value, dtype=torch.float32, device=dev)
        gf = torch.empty(D * (F + D) + D + D * D + D, dtype=torch.float32, device=dev)
        gfold, g2fold = gf[:D * (F + D) + D], gf[D * (F + D) + D:]
        p = ctx.params
        g = [grad_out(p[0], (D, D), dev), grad_out(p[1], (D,), dev),
             grad_out(p[2], (D, D), dev), grad_out(p[3], (D,), dev),
             grad_out(p[4], (D, D), dev), grad_out(p[5], (D,), dev),
             grad_out(p[6], (D, F + D), dev), grad_out(p[7], (D,), dev)]
        parts = ctypes.c_int32(0)
        _lib.call("gine_deepset_bwd_num_partials", N, D, ctypes.byref(parts))
        ds_slab = torch.empty(parts.value * (D * Fe + D), dtype=torch.float32, device=dev)
        dw = grad_out(link.params[0], (D, Fe), dev)
        db = grad_out(link.params[1], (D,), dev)
        P = _lib.ptr
        stream = _lib.stream_handle(dev)
        ds_defer = gradbuf.deferrable(dw, db)  # slab reduced in the end-of-backward batch
        # dt (to memory, for the engine below) and dr (on chip) per 32-node group, then that
        # group's DeepSet weight-gradient partials: one launch
        _lib.call("gine_deepset_bwd_chain", P(ens), P(mask), P(dh0), P(u), P(wf1), P(wf2), P(dt),
                  P(ds_slab), None if ds_defer else P(dw), None if ds_defer else P(db), N, M,
                  Fe, D, F, stream)
        # raw pointers only: a reference to a gradient tensor held past this function would
        # stop autograd adopting it as param.grad (it copies a shared tensor)
        ptrs = (P(gfold), P(wr1), P(br1), P(wdr), P(g[6]), P(g[7]), P(g[4]), P(g[5]),
                P(g2fold), P(wp2), P(bp2), P(wr0), P(g[2]), P(g[3]), P(g[0]), P(g[1]),
                ctx.members)

        def unfold(st):
            _lib.call("gine_chain_unfold_grads2", *ptrs, D, F, st)

        if gradbuf.deferrable(*g):
            _lib.call("gine_chain_wgrad_folded2", P(dh0), P(x), P(r), P(u), P(dt), P(slab), None,
                      None, N, D, F, stream)
            job = _lib.GradJob()
            _lib.call("gine_chain_wgrad_folded2_grad_job", N, D, F, P(slab), P(gfold),
                      P(g2fold), ctypes.byref(job))
            gradbuf.defer(job, dev, (slab, gf, wp2, bp2, wr0, wr1, br1, wdr), post=unfold)
        else:
            _lib.call("gine_chain_wgrad_folded2", P(dh0), P(x), P(r), P(u), P(dt), P(slab),
                      P(gfold), P(g2fold), N, D, F, stream)
            unfold(stream)
        if ds_defer:
            job = _lib.GradJob()
            _lib.call("gine_deepset_bwd_grad_job", N, Fe, D, P(ds_slab), P(dw), P(db),
                      ctypes.byref(job))
            gradbuf.defer(job, dev, (ds_slab,))
        link.put(dw, db)
        del dw, db
        return (None, None, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], None, None, None)


def encoder_fusable(ens: torch.Tensor, x: torch.Tensor, lin1) -> bool:
    """True where :func:`encoder` applies: gradients are being recorded for phi[0] and the
    library takes the shape (gine_deepset_bwd_chain_ok).  The callers have checked
    ``deepset.fusable`` and :func:`fusable_dims`."""
    if not (FOLD and torch.is_grad_enabled() and lin1.weight.requires_grad
            and lin1.bias.requires_grad):
        return False
    ok = ctypes.c_int32(0)
    _lib.call("gine_deepset_bwd_chain_ok", ens.size(0), lin1.out_features, ens.size(2),
              x.size(1), ctypes.byref(ok))
    return bool(ok.value)


def encoder(ens: torch.Tensor, x: torch.Tensor, lin1, lins) -> torch.Tensor:
    """``dim_red(cat([x, rho(phi(ens) summed over members)]))``: ``deepset.phi_sum`` with the
    fold, then :func:`chain`, as two autograd nodes that share one backward launch
    (gine_deepset_bwd_chain) plus the weight-gradient engine: one launch fewer than the two
    Functions' backward.  ``lins`` = (phi[2], rho[0], rho[2], dim_red)."""
    p2, r0, r1, dr = lins
    link = deepset.EncLink()
    r, wfold = deepset._PhiSumEncFn.apply(
        ens, lin1.weight, lin1.bias,
        tuple(t for m in (r1, dr, r0, p2) for t in (m.weight, m.bias)), link)
    return _ChainFolded2FnEnc.apply(r, x, p2.weight, p2.bias, r0.weight, r0.bias, r1.weight,
                                    r1.bias, dr.weight, dr.bias, ens.size(1), wfold, link)


# False: the unfolded chain (four GEMM stages forward, s and e materialised); measured slower
# (cfg2 0.5749 vs 0.5595 ms per step against the single fold, r02_s38), kept for the tests
# that compare the two
FOLD = True


def chain(r: torch.Tensor, x: torch.Tensor, lins, members: int, wfold=None) -> torch.Tensor:
    """``dim_red(cat([x, rho(phi[2](r) summed over members)]))`` on the fused kernels.
    ``lins`` = (phi[2], rho[0], rho[2], dim_red); ``wfold`` = their folded weights
    [W' | b' | W'^T | Wf | bf] from ``deepset.phi_sum(ens, lin1, fold=...)`` on the same
    weights and ``members`` (required unless ``FOLD`` is off)."""
    p2, r0, r1, dr = lins
    if not FOLD:
        return _ChainFn.apply(r, x, p2.weight, p2.bias, r0.weight, r0.bias, r1.weight, r1.bias,
                              dr.weight, dr.bias, members)
    D, F = r.size(1), x.size(1)
    if wfold is None or wfold.numel() != 2 * D * (F + D) + D + D * D + D:
        raise ValueError(f"the folded chain needs wfold with [W' | b' | W'^T | Wf | bf] for "
                         f"D={D}, F={F}")
    return _ChainFolded2Fn.apply(r, x, p2.weight, p2.bias, r0.weight, r0.bias, r1.weight,
                                 r1.bias, dr.weight, dr.bias, members, wfold)
