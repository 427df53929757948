"""Precision helpers for the split-bf16 matrix products (csrc/gine_bf16x3.hpp): the
componentwise error measure, probe operands whose exact product is an fp32 number, and a
torch emulator of the documented algorithm.  No tests are collected from this module and
nothing here needs a GPU; tests/test_precision_model.py pins on the CPU that the two checks
of tests/test_gpu_precision.py can fail.

The two checks ("Precision contract of the split-bf16 products"):

* Check A, probes: operands built so that every output element is a sum of at most four
  nonzero products and every partial sum, in any order and of any subset of the six plane
  products, is a multiple of one unit below 2^24 units -- an fp32 number.  A correct
  evaluation therefore returns the exact product; the bound is PROBE_BOUND = 2^-22 of
  (|A||B|)_ij, 16x under the smallest defect the probes are built to show (one dropped
  l.h plane product, 2^-18) and 4 units of fp32 roundoff over exact.
* Check B, random operands: compwise(kernel) <= RATIO x compwise(fp32 CPU matmul) with
  RATIO = 3 (the emulated algorithm sits at 0.55-0.65x, its mildest defect at >= 5.4x).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

PROBE_BOUND = 2.0 ** -22
RATIO = 3.0
# (A plane, B plane) of the six partial products, in the order mfma_bf16x3 issues them
SIX = ("lh", "hl", "mm", "mh", "hm", "hh")

_M3 = 1.0 + 2.0 ** -9 + 2.0 ** -18   # planes h = 1, m = 2^-9, l = 2^-18
_M2 = 1.0 + 2.0 ** -9                # planes h = 1, m = 2^-9


# ---------------------------------------------------------------------------------------
# componentwise error
# ---------------------------------------------------------------------------------------
def compwise_ref(got: torch.Tensor, ref64: torch.Tensor, scale: torch.Tensor) -> float:
    """max_ij |got - ref64|_ij / scale_ij over the elements with scale > 0.  Elements whose
    scale is 0 must be exactly 0 in ``got``: inf otherwise, which no bound admits."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    err = (got - ref64).abs()
    zero = scale == 0
    if not bool((got[zero] == 0).all()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / scale[~zero]).max())


def product64(A, B, bias=None):
    """(ref64, scale) of A B + bias: the product and |A||B| + |bias| in fp64."""
    A, B = A.detach().double().cpu(), B.detach().double().cpu()
    ref, scale = A @ B, A.abs() @ B.abs()
    if bias is not None:
        b = bias.detach().double().cpu()
        ref, scale = ref + b, scale + b.abs()
    return ref, scale


def compwise(got, A, B, bias=None) -> float:
    """max_ij |got - ref64|_ij / (|A||B| + |bias|)_ij, reference and scale in fp64."""
    ref, scale = product64(A, B, bias)
    return compwise_ref(got, ref, scale)


# ---------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------
@dataclass
class Probe:
    name: str
    A: torch.Tensor       # [M, K] fp32
    B: torch.Tensor       # [K, J] fp32
    exact: torch.Tensor   # [M, J] fp32: the exact product
    scale: torch.Tensor   # [M, J] fp64: |A||B|


def _support(M: int, K: int, J: int):
    """Boolean supports SA [M, K], SB [K, J] such that every output (i, j) meets at most four
    k with both nonzero and every k is met by at least one output.
    4M >= K: row i of A holds k = 4i .. 4i+3 (mod K) and B is dense.
    4M <  K (the contraction runs over many rows: the weight gradients): column k of A holds
    row k mod M only, the k of one row fall into S = ceil(K / M) layers k div M, and column j
    of B keeps the four layers 4j .. 4j+3 (mod S)."""
    k = torch.arange(K)
    SA = torch.zeros(M, K, dtype=torch.bool)
    if 4 * M >= K:
        q = min(4, K)
        rows = torch.arange(M).repeat_interleave(q)
        SA[rows, (4 * rows + torch.arange(q).repeat(M)) % K] = True
        SB = torch.ones(K, J, dtype=torch.bool)
    else:
        S = -(-K // M)
        if 4 * J < S:
            raise ValueError(f"no probe for M={M} K={K} J={J}: 4*M*J outputs slots < K")
        SA[k % M, k] = True
        SB = ((k // M)[:, None] - 4 * torch.arange(J)[None, :]) % S < 4
    return SA, SB


def _values(shape, exps, mant, signed, gen):
    e = torch.tensor(exps, dtype=torch.float64)[torch.randint(len(exps), shape, generator=gen)]
    v = torch.exp2(e) * mant
    if signed:
        v = v * (2.0 * torch.randint(2, shape, generator=gen).double() - 1.0)
    return v


def _keep(v, support):
    return torch.where(support, v, torch.zeros((), dtype=v.dtype))


def _finish(name, A64, B64, unit_exp):
    """fp32 operands and the exact product, with the generator's own assertions."""
    A, B = A64.float(), B64.float()
    assert torch.equal(A.double(), A64) and torch.equal(B.double(), B64)
    ref, scale = A64 @ B64, A64.abs() @ B64.abs()
    exact = ref.float()
    assert torch.equal(exact.double(), ref), f"{name}: the exact product is not an fp32 number"
    # every partial sum of plane products, in any order, is an fp32 number: all are multiples
    # of one unit and none exceeds the sum of the magnitudes, itself below 2^24 units
    unit = 2.0 ** unit_exp
    assert bool((scale < 2.0 ** 24 * unit).all()), name
    for t in (A64, B64):
        assert torch.equal(torch.round(t / 2.0 ** -20) * 2.0 ** -20, t), name
    assert torch.equal(torch.round(ref / unit) * unit, ref), name
    met = (A64 != 0).float() @ (B64 != 0).float()
    assert float(met.max()) <= 4, f"{name}: an output sums more than four products"
    return Probe(name, A, B, exact, scale)


def _assert_k_covered(name, multi, other, k_axis):
    """Every k carries a nonzero of the multi-plane operand that meets a nonzero of the other
    operand, i.e. shows in at least one output."""
    a = (multi != 0).any(1 - k_axis)
    b = (other != 0).any(k_axis)
    assert bool((a & b).all()), f"{name}: a k index carries no visible multi-plane value"


def three_plane_A(M, K, J, seed=0, signed_a=True, signed_b=True) -> Probe:
    """A (sparse) = +-2^e (1 + 2^-9 + 2^-18), e in {0, 1}: planes h, m, l all nonzero at the
    same k.  B = +-2^e(k, j), e in {-1, 0, 1}, drawn per (k, j), so a plane paired with the
    wrong k gives another number.  Shows ah.bh, am.bh, al.bh."""
    gen = torch.Generator().manual_seed(1000 + seed)
    SA, SB = _support(M, K, J)
    A = _keep(_values((M, K), (0.0, 1.0), _M3, signed_a, gen), SA)
    B = _keep(_values((K, J), (-1.0, 0.0, 1.0), 1.0, signed_b, gen), SB)
    _assert_k_covered("three_plane_A", A, B, 1)
    return _finish("three_plane_A", A, B, -19)


def three_plane_B(M, K, J, seed=0, signed_a=True, signed_b=True) -> Probe:
    """The mirror image: B (sparse) carries the three planes, A the powers of two.  Shows
    ah.bm, ah.bl."""
    p = three_plane_A(J, K, M, seed + 1, signed_a=signed_b, signed_b=signed_a)
    A, B = p.B.t().contiguous(), p.A.t().contiguous()
    return Probe("three_plane_B", A, B, p.exact.t().contiguous(), p.scale.t().contiguous())


def two_plane(M, K, J, seed=0, signed_a=True, signed_b=True) -> Probe:
    """A (sparse) = +-2^e (1 + 2^-9), B = +-2^e (1 + 2^-9): each product is
    2^e (1 + 2^-8 + 2^-18), whose last bit is am.bm."""
    gen = torch.Generator().manual_seed(2000 + seed)
    SA, SB = _support(M, K, J)
    A = _keep(_values((M, K), (0.0, 1.0), _M2, signed_a, gen), SA)
    B = _keep(_values((K, J), (-1.0, 0.0, 1.0), _M2, signed_b, gen), SB)
    _assert_k_covered("two_plane", A, B, 1)
    return _finish("two_plane", A, B, -19)


FAMILIES = {"three_plane_A": three_plane_A, "three_plane_B": three_plane_B,
            "two_plane": two_plane}
# the operand that carries more than one plane, per family (for the permutation tests)
MULTI_PLANE = {"three_plane_A": "A", "three_plane_B": "B", "two_plane": "A"}


def probe_error(got: torch.Tensor, p: Probe):
    """(max |got - exact| / (|A||B|), number of elements that are not bit-exact)."""
    got = got.detach().cpu().reshape(p.exact.shape)
    inexact = int((got != p.exact).sum())
    return compwise_ref(got, p.exact.double(), p.scale), inexact


def random_operands(M, K, J, seed=0, nonneg_a=False, nonneg_b=False):
    """Check B's operands: A = randn(M, K), B = randn(K, J) / sqrt(K), seeded (absolute
    values where the site applies a ReLU to that operand)."""
    gen = torch.Generator().manual_seed(3000 + seed)
    A = torch.randn(M, K, generator=gen)
    B = torch.randn(K, J, generator=gen) / K ** 0.5
    return (A.abs() if nonneg_a else A), (B.abs() if nonneg_b else B)


# ---------------------------------------------------------------------------------------
# DeepSet forward: r[n, :] = sum_m relu(ens[n, m, :] W1^T + b1)
# ---------------------------------------------------------------------------------------
@dataclass
class DeepSetProbe:
    name: str
    ens: torch.Tensor     # [N, M, F] fp32
    w1: torch.Tensor      # [H, F] fp32
    exact: torch.Tensor   # [N, H] fp32
    scale: torch.Tensor   # [N, H] fp64: sum_m |ens||W1|^T


def deepset_reference(ens, w1, b1=None):
    """(ref64, scale) of the member sum of relu(ens W1^T + b1): relu is exact on exact
    values, so this is the exact result of the fused launch."""
    e, w = ens.detach().double().cpu(), w1.detach().double().cpu()
    pre, scale = e @ w.t(), e.abs() @ w.abs().t()
    if b1 is not None:
        b = b1.detach().double().cpu()
        pre, scale = pre + b, scale + b.abs()
    return torch.relu(pre).sum(1), scale.sum(1)


def deepset_probe(family, N, M, F, H, seed=0) -> DeepSetProbe:
    """The probe families for the DeepSet forward.  An output r[n, h] sums over members and
    features, so the at-most-four rule holds per node over all its members:
    three_plane_A / two_plane: node n holds four nonzeros, feature (4n + q) mod F of member
    (n + q) mod M, and W1 is dense; three_plane_B: node n holds one dense member n mod M and
    row h of W1 the four features (4h + q) mod F.  Every feature k < F -- the last one sits
    in a 16-k block that is otherwise zero padding when F % 16 == 1 -- carries a nonzero of
    the multi-plane operand."""
    gen = torch.Generator().manual_seed(4000 + seed)
    q = min(4, F)
    ens = torch.zeros(N, M, F, dtype=torch.float64)
    if family == "three_plane_B":
        n = torch.arange(N)
        ens[n, n % M, :] = _values((N, F), (-1.0, 0.0, 1.0), 1.0, True, gen)
        S = torch.zeros(H, F, dtype=torch.bool)
        h = torch.arange(H).repeat_interleave(q)
        S[h, (4 * h + torch.arange(q).repeat(H)) % F] = True
        w1 = _keep(_values((H, F), (0.0, 1.0), _M3, True, gen), S)
        multi = w1
    else:
        mant = _M3 if family == "three_plane_A" else _M2
        n = torch.arange(N).repeat_interleave(q)
        qq = torch.arange(q).repeat(N)
        ens[n, (n + qq) % M, (4 * n + qq) % F] = _values((N * q,), (0.0, 1.0), mant, True, gen)
        w1 = _values((H, F), (-1.0, 0.0, 1.0), 1.0 if family == "three_plane_A" else _M2,
                     True, gen)
        multi = ens.reshape(N * M, F)
    assert bool((multi != 0).any(0).all()), f"{family}: a feature carries no multi-plane value"
    assert bool((w1 != 0).any(0).all()) and bool((ens != 0).any(0).any(0).all())
    met = (ens != 0).float().reshape(N, M * F) @ (w1 != 0).float().t().repeat(M, 1)
    assert float(met.max()) <= 4, f"{family}: an output sums more than four products"
    ens32, w32 = ens.float(), w1.float()
    assert torch.equal(ens32.double(), ens) and torch.equal(w32.double(), w1)
    ref, scale = deepset_reference(ens32, w32)
    exact = ref.float()
    assert torch.equal(exact.double(), ref), f"{family}: the exact result is not an fp32 number"
    unit = 2.0 ** -19
    assert bool((scale < 2.0 ** 24 * unit).all())
    assert torch.equal(torch.round(ref / unit) * unit, ref)
    return DeepSetProbe(family, ens32, w32, exact, scale)


# ---------------------------------------------------------------------------------------
# the documented algorithm, emulated (the detector's self-test model, not a GPU reference)
# ---------------------------------------------------------------------------------------
def split3(x: torch.Tensor):
    """x = h + m + l: each plane the round-to-nearest-even bf16 of what the planes before it
    leave (the subtractions are exact in fp32)."""
    x = x.float()
    h = x.bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    return {"h": h, "m": m, "l": l}


def emulate(A, B, terms=SIX, perm=None) -> torch.Tensor:
    """A B as gine_bf16x3.hpp documents it: RNE planes, k in blocks of 16 (zero padded), per
    block the plane products of ``terms`` in mfma_bf16x3's order, each a 16-term dot product
    added to the fp32 accumulator with one rounding.  ``perm`` = (operand "A" | "B", plane
    "h" | "m" | "l", p): that plane of that operand reads k = 8 (k div 8) + p[k mod 8]
    instead of k -- a fragment assembled in the wrong order."""
    A, B = A.detach().float().cpu(), B.detach().float().cpu()
    M, K = A.shape
    Kp = -(-K // 16) * 16
    A = torch.nn.functional.pad(A, (0, Kp - K))
    B = torch.nn.functional.pad(B, (0, 0, 0, Kp - K))
    pa, pb = split3(A), split3(B)
    if perm is not None:
        operand, plane, p = perm
        k = torch.arange(Kp)
        idx = (k // 8) * 8 + torch.as_tensor(p)[k % 8]
        if operand == "A":
            pa[plane] = pa[plane][:, idx]
        else:
            pb[plane] = pb[plane][idx, :]
    acc = torch.zeros(M, B.shape[1], dtype=torch.float32)
    for k0 in range(0, Kp, 16):
        for t in SIX:
            if t in terms:
                part = pa[t[0]][:, k0:k0 + 16].double() @ pb[t[1]][k0:k0 + 16].double()
                acc = (acc.double() + part).float()
    return acc
