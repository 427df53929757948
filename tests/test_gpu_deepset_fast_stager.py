"""GPU: the DeepSet kernels' full-tile stager (csrc/gine_deepset.hip FastStager: 16-byte loads,
no per-element range tests) against the generic stager, the in-tree reference that
gine_testing_deepset_generic_stager forces, on the same inputs.

Only the way operands reach LDS differs, so r, the mask words, the slab, dW1 and db1 -- and dt
of the fused encoder backward -- must be the same bits.  The fast stager is taken per launch
when every tile of every walk is full (16-node halves, N % 32 == 0, H in {64, 128}) and ens is
on a 16-byte boundary; the shapes are the smallest that reach each side of those conditions
(16-node halves need N > 8,192 at H = 128 and N > 16,384 at H = 64).
"""
import ctypes

import pytest
import torch

from raincast_gnn import _lib
from test_gpu_enc_bwd_fused import _Case, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = _lib.ptr


@pytest.fixture(autouse=True)
def _switch_back():
    yield
    _lib.call("gine_testing_deepset_generic_stager", 0)


def _inputs(N, M, F, H, seed, offset=0):
    """ens [N, M, F] (a view `offset` floats into its buffer), W1, b1, dr."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = torch.zeros(N * M * F + offset, device=DEV)
    ens = buf[offset:].view(N, M, F)
    ens.copy_(torch.randn(N, M, F, generator=g))
    w = (torch.randn(H, F, generator=g) * F ** -0.5).to(DEV)
    b = (torch.randn(H, generator=g) * 0.1).to(DEV)
    dr = torch.randn(N, H, generator=g).to(DEV)
    return ens, w, b, dr


def _run(ens, w, b, dr, generic):
    """Forward then backward -> r, mask words, slab, dW1, db1."""
    N, M, F = ens.shape
    H = w.shape[0]
    _lib.call("gine_testing_deepset_generic_stager", 1 if generic else 0)
    st = _lib.stream_handle(DEV)
    nbytes = ctypes.c_size_t(0)
    _lib.call("gine_deepset_mask_bytes", N, M, H, ctypes.byref(nbytes))
    mask = torch.zeros(nbytes.value, dtype=torch.uint8, device=DEV)
    parts = ctypes.c_int32(0)
    _lib.call("gine_deepset_bwd_num_partials", N, H, ctypes.byref(parts))
    r = torch.empty(N, H, device=DEV)
    slab = torch.empty(parts.value * (H * F + H), device=DEV)
    dw, db = torch.empty(H, F, device=DEV), torch.empty(H, device=DEV)
    _lib.call("gine_deepset_fwd", P(ens), P(w), P(b), P(r), P(mask), N, M, F, H, st)
    _lib.call("gine_deepset_bwd", P(ens), P(mask), P(dr), P(slab), P(dw), P(db), N, M, F, H, st)
    torch.cuda.synchronize()
    _lib.call("gine_testing_deepset_generic_stager", 0)
    return r, mask, slab, dw, db


NAMES = ("r", "mask", "slab", "dW1", "db1")


def _takes_full_tiles(ens, H):
    """Which stager a launch on this ens takes (gine_testing_deepset_stager)."""
    full = ctypes.c_int32(-1)
    _lib.call("gine_testing_deepset_stager", P(ens), ens.shape[0], H, ctypes.byref(full))
    return bool(full.value)


FULL = {"full": True, "short1": False, "F36": True, "F33": True, "M1": True, "H64": True,
        "N64": False, "N1000": False}


@pytest.mark.parametrize("N,M,F,H", [
    (8224, 11, 35, 128),    # all tiles full: the fast walk
    (8193, 11, 35, 128),    # last group holds one node: the launch stays generic
    (8224, 11, 36, 128),    # F a multiple of 4
    (8224, 11, 33, 128),    # another odd F
    (8224, 1, 35, 128),     # M = 1: a group is one tile, every row a node of its own
    (16416, 11, 35, 64),    # H = 64 at 16-node groups
    (64, 11, 35, 128),      # 4-node groups: unchanged path still agrees
    (1000, 11, 35, 128),    # 4-node groups
], ids=["full", "short1", "F36", "F33", "M1", "H64", "N64", "N1000"])
def test_fast_and_generic_stagers_same_bits(N, M, F, H, request):
    x = _inputs(N, M, F, H, seed=N + M + F + H)
    # the comparison below is between the two stagers only where the full-tile one is taken
    assert _takes_full_tiles(x[0], H) == FULL[request.node.callspec.id]
    _lib.call("gine_testing_deepset_generic_stager", 1)
    assert not _takes_full_tiles(x[0], H)
    _lib.call("gine_testing_deepset_generic_stager", 0)
    fast, ref = _run(*x, generic=False), _run(*x, generic=True)
    for name, a, b in zip(NAMES, fast, ref):
        assert torch.equal(a, b), name
    r, mask, _, dw, _ = fast
    assert torch.isfinite(r).all() and torch.isfinite(dw).all()
    assert r.abs().max() > 0 and dw.abs().max() > 0 and mask.any()


def test_unaligned_view_runs_generic_and_agrees():
    """ens one float into a larger buffer is off the 16-byte boundary: the launch must stay on
    the generic stager, and give what the aligned copy gives on the fast one."""
    N, M, F, H = 8224, 11, 35, 128
    ens, w, b, dr = _inputs(N, M, F, H, seed=21, offset=1)
    assert ens.data_ptr() % 16 == 4
    assert not _takes_full_tiles(ens, H) and _takes_full_tiles(ens.clone(), H)
    got, ref = _run(ens, w, b, dr, generic=False), _run(ens, w, b, dr, generic=True)
    aligned = _run(ens.clone(), w, b, dr, generic=False)
    for name, a, b_, c in zip(NAMES, got, ref, aligned):
        assert torch.equal(a, b_) and torch.equal(a, c), name


def test_non_finite_ens_same_r_both_ways():
    """A NaN and an inf in ens: the waves that see them redo their tiles on the fp32 chain
    from memory; r (NaN pattern and every other value), the mask words and the backward's
    outputs agree."""
    N, M, F, H = 8224, 11, 35, 128
    ens, w, b, dr = _inputs(N, M, F, H, seed=22)
    ens[1234, 5, 17] = float("nan")
    ens[7000, 0, 34] = float("inf")
    assert _takes_full_tiles(ens, H)
    fast, ref = _run(ens, w, b, dr, generic=False), _run(ens, w, b, dr, generic=True)
    assert torch.equal(fast[1], ref[1]), "mask"
    for name, a, b_ in zip(NAMES, fast, ref):
        if name != "mask":
            assert _same(a, b_), name
    r = fast[0]
    assert r[1234].isnan().any() and not torch.isfinite(r[7000]).all()
    rows = torch.ones(N, dtype=torch.bool, device=DEV)
    rows[1234] = rows[7000] = False
    assert torch.isfinite(r[rows]).all()


def test_fused_encoder_backward_same_bits():
    """k_deepset_bwd_chain with the fast stager allowed against the forced generic run."""
    c = _Case(8224, 11, 128, seed=23)
    assert _takes_full_tiles(c.ens, 128)
    _lib.call("gine_testing_deepset_generic_stager", 0)
    fast = c.fused()
    _lib.call("gine_testing_deepset_generic_stager", 1)
    ref = c.fused()
    torch.cuda.synchronize()
    for name, a, b in zip(("dt", "slab", "dW1", "db1"), fast, ref):
        assert torch.equal(a, b), name
    assert torch.isfinite(fast[2]).all() and fast[2].abs().max() > 0
