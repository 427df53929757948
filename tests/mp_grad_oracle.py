"""Exact oracle of the message-passing backward's parameter and edge gradients (numpy,
``math.fsum`` and ``fractions.Fraction``; no torch, no autograd).

What every launch form of the backward computes (csrc/gine_edge.hpp bwd_edge, gine_mp.hip
k_mp_bwd, gine_mpwin.hip k_mp_bwd_win, gine_mpek.hip k_mp_bwd_ek):

* per source node i, over its out-edges e in out-CSR order, in fp32::

      pre_e  = x_i + lin(a_e)                     lin: b, then fma(a_e[k], W[:, k], .) for k
                                                  ascending ("fma"); fl(fl(a W) + b) ("muladd")
      dm_e   = (pre_e <= 0) ? 0 : dz[dst_e]       (a NaN pre_e keeps dz)
      acc_i  = fl(acc_i + dm_e)
      accw_i[k] = fma(dm_e, a_e[k], accw_i[k])    one rounding

* across nodes, ``(double) acc_i`` and ``(double) accw_i`` are added up in fp64 in an order
  that depends on the form (lanes, waves, workgroups, tiles, the finish kernel), and the
  total is cast to fp32 once: ``db = fl32(sum_i acc_i)``, ``dW[:, k] = fl32(sum_i accw_i[k])``;
* ``deps = fl32(sum_{i, c} dz[i, c] x[i, c])``: the products are exact in fp64 (24 x 24
  bits), their sum runs in fp64, cast once;
* ``d a_e[k]`` (gine_mpek.hip edge_grad_ek), in fp32 with contraction off: each lane of four
  channels ``(dm0 W0k + dm1 W1k) + (dm2 W2k + dm3 W3k)``, then an xor butterfly over the
  L = pow2ceil(D / 4) lanes of the row group, padding lanes adding 0.  Both operands of every
  butterfly add are the two halves' sums in either order, and fp32 addition commutes, so
  lane 0 holds the balanced pairwise tree of the L lane values.

:func:`node_sums` restates the per-node part bit for bit, :func:`exact` gives the exact sum
``S`` of the per-node fp32 values (``math.fsum``: correctly rounded) and the sum ``A`` of
their absolute values, and :func:`bound` is the derived (not measured) error bound of the
cross-node part.

Derivation of ``bound(S, A, n) = 2^-24 |S| + gamma_n(2^-53) A + 2^-149``,
``gamma_n(u) = n u / (1 - n u)``.  The fp64 total T of n terms t_i, added in any order,
satisfies ``|T - S| <= gamma_(n-1)(2^-53) A`` (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 4.2: any summation order).  The one cast to fp32 adds at most
``2^-24 |T|`` for a normal result and half the subnormal spacing, ``2^-150``, otherwise, and
``|T| <= |S| + gamma_(n-1) A``.  Together ``2^-24 |S| + (1 + 2^-24) gamma_(n-1) A + 2^-150``,
and ``(1 + 2^-24) gamma_(n-1) <= gamma_n`` while ``(n - 1) 2^-77 <= 2^-53``, that is for
``n <= 2^24``.  The first-order form therefore assumes: n <= 2^24 (:data:`MAX_TERMS`), every
term finite, and ``|S| + A`` far below the fp32 overflow threshold (:data:`MAX_MAGNITUDE`);
the fp32 x fp32 products of ``deps`` can neither overflow nor underflow in fp64.
:func:`check_ranges` asserts these for a case.

The fused multiply-add is rounded once.  ``fl32(fl64(a b + c))`` rounds twice, which differs
from the fma where the fp64 sum lands on an fp32 midpoint that the exact sum does not.
:func:`fma32` forms the exact product in fp64, adds with TwoSum (Knuth) to get the fp64 sum
and its exact error, turns the fp64 sum into the round-to-odd value of the exact sum, and
rounds that to fp32: rounding to odd at p + 2 or more bits followed by rounding to nearest
at p bits is rounding to nearest once (Boldo and Melquiond, 2008), and 53 >= 24 + 2 also
for fp32 subnormals.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24
U64 = 2.0 ** -53
MAX_TERMS = 2 ** 24
MAX_MAGNITUDE = 2.0 ** 100


# ---------------------------------------------------------------------------------------
# fp32 arithmetic, one rounding per operation
# ---------------------------------------------------------------------------------------
def _round_odd(s: np.ndarray, e: np.ndarray) -> np.ndarray:
    """fp64 ``s`` = RN(v) and ``e`` = v - s exactly -> the round-to-odd fp64 value of v."""
    s = np.ascontiguousarray(s, dtype=np.float64)
    even = (s.view(np.int64) & 1) == 0
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
    return np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def fma32(a, b, c) -> np.ndarray:
    """fl32(a * b + c) with a single rounding, elementwise with broadcasting."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
        c = np.asarray(c, F32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)          # TwoSum: s + e == p + c exactly
        return _round_odd(s, e).astype(F32)


def fma32_fraction(a, b, c) -> np.float32:
    """The same for three scalars, through exact rationals (the proof's reference)."""
    return round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def round32(v: Fraction) -> np.float32:
    """Round an exact rational to the nearest fp32, ties to even (finite range only)."""
    if v == 0:
        return F32(0.0)
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1                                # 2^e <= v < 2^(e+1)
    q = max(e, -126) - 23                     # exponent of the last kept bit
    scaled = v / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F32(sign * math.ldexp(float(n), q))


def lin32(attr: np.ndarray, W: np.ndarray, b: np.ndarray, mode: str) -> np.ndarray:
    """[n, K] attributes -> [n, D] values of the edge Linear in the kernel's rounding."""
    if mode == "fma":
        e = np.broadcast_to(b.astype(F32), (attr.shape[0], b.shape[0]))
        for k in range(W.shape[1]):
            e = fma32(attr[:, k:k + 1], W[None, :, k], e)
        return e
    assert mode == "muladd" and W.shape[1] == 1, mode
    with np.errstate(all="ignore"):
        return (attr[:, :1] * W[None, :, 0]).astype(F32) + b[None, :].astype(F32)


# ---------------------------------------------------------------------------------------
# per-node sums, bit for bit
# ---------------------------------------------------------------------------------------
def node_sums(x, dz, rowptr, dst, attr, W, b, mode="fma") -> dict:
    """``x``, ``dz`` [N, D]; out-CSR ``rowptr`` [N + 1], ``dst`` [E]; ``attr`` [E, K] in
    out-CSR order; ``W`` [D, K]; ``b`` [D]; ``mode`` "fma" | "muladd".

    Returns ``on`` [E, D] (the kernel's ReLU decisions, out-CSR order), ``dm`` [E, D] fp32,
    ``acc`` [N, D] fp32 and ``accw`` [N, D, K] fp32.  The loop runs over the edge position
    within a node and is vectorised over nodes and channels: max out-degree iterations."""
    x, dz = np.ascontiguousarray(x, F32), np.ascontiguousarray(dz, F32)
    W = np.asarray(W, F32).reshape(x.shape[1], -1)
    attr = np.asarray(attr, F32).reshape(len(dst), W.shape[1])
    b = np.asarray(b, F32)
    rowptr = np.asarray(rowptr, np.int64)
    dst = np.asarray(dst, np.int64)
    N, D = x.shape
    K = W.shape[1]
    deg = np.diff(rowptr)
    acc = np.zeros((N, D), F32)
    accw = np.zeros((N, D, K), F32)
    on = np.zeros((len(dst), D), bool)
    dm = np.zeros((len(dst), D), F32)
    with np.errstate(all="ignore"):
        for j in range(int(deg.max()) if N else 0):
            nodes = np.nonzero(deg > j)[0]
            e = rowptr[nodes] + j
            a = attr[e]
            pre = x[nodes] + lin32(a, W, b, mode)
            keep = ~(pre <= 0)
            d = np.where(keep, dz[dst[e]], F32(0.0))
            on[e], dm[e] = keep, d
            acc[nodes] = acc[nodes] + d
            accw[nodes] = fma32(d[:, :, None], a[:, None, :], accw[nodes])
    return {"on": on, "dm": dm, "acc": acc, "accw": accw}


def dx32(acc, dz, eps, self_term=True, dres=None) -> np.ndarray:
    """dx = acc [+ fl((1 + eps) dz)] [+ dres], each step rounded to fp32."""
    with np.errstate(all="ignore"):
        o = np.asarray(acc, F32)
        if self_term:
            ope = F32(1.0) + F32(eps)
            o = o + ope * np.asarray(dz, F32)
        if dres is not None:
            o = o + np.asarray(dres, F32)
        return o


# ---------------------------------------------------------------------------------------
# exact cross-node sums and their bound
# ---------------------------------------------------------------------------------------
def fsum_round32(vals) -> tuple:
    """(S, fl32 of the exact sum) of fp64 values: S = fsum (correctly rounded to fp64), and
    the fp32 rounding of the exact sum itself (not of S: the sign of the exact remainder,
    again by fsum, gives S's round-to-odd value first)."""
    vals = [float(v) for v in vals]
    S = math.fsum(vals)
    rem = math.fsum(vals + [-S])
    odd = _round_odd(np.array([S]), np.array([rem]))
    with np.errstate(all="ignore"):
        return S, odd.astype(F32)[0]


def _columns(mat: np.ndarray) -> tuple:
    """[n, m] fp64 terms -> per column (S, A, fl32(exact sum)).  A column with a non-finite
    term has no exact sum: S is then the fp64 sum's NaN / inf, which no order changes (a NaN
    or both infinities give NaN, one infinity stays), and A is inf."""
    n, m = mat.shape
    S, A, R = np.zeros(m), np.zeros(m), np.zeros(m, F32)
    finite = np.isfinite(mat).all(axis=0)
    with np.errstate(all="ignore"):
        for c in range(m):
            col = mat[:, c]
            if finite[c]:
                S[c], R[c] = fsum_round32(col.tolist())
                A[c] = math.fsum(np.abs(col).tolist())
            else:
                S[c] = col.sum()
                A[c] = np.inf
                R[c] = F32(S[c])
    return S, A, R


def exact(ns: dict, x, dz, rows=None, cols=None) -> dict:
    """Per output ``dW`` [D, K], ``db`` [D] and ``deps`` [1]: ``S`` (exact sum of the per-node
    fp32 values; for deps, of the exact products), ``A`` (sum of absolute values), ``r32``
    (the correctly rounded fp32 result) and ``n`` (terms per sum).  ``rows`` = (n0, n1)
    restricts the sums to those nodes and ``cols`` = (c0, c1) deps to those channels: the
    window form's per-tile, per-slice partial rows."""
    n0, n1 = rows if rows is not None else (0, ns["acc"].shape[0])
    acc = ns["acc"][n0:n1].astype(np.float64)
    accw = ns["accw"][n0:n1].astype(np.float64)
    n, D, K = accw.shape
    out = {}
    S, A, R = _columns(acc)
    out["db"] = {"S": S, "A": A, "r32": R, "n": n}
    S, A, R = _columns(accw.reshape(n, D * K))
    out["dW"] = {"S": S.reshape(D, K), "A": A.reshape(D, K), "r32": R.reshape(D, K), "n": n}
    c0, c1 = cols if cols is not None else (0, D)
    with np.errstate(all="ignore"):
        prod = (np.asarray(dz, F32)[n0:n1, c0:c1].astype(np.float64)
                * np.asarray(x, F32)[n0:n1, c0:c1].astype(np.float64))
    S, A, R = _columns(prod.reshape(-1, 1))
    out["deps"] = {"S": S, "A": A, "r32": R, "n": prod.size}
    return out


def gamma(n: int, u: float = U64) -> float:
    return n * u / (1.0 - n * u)


def bound(S, A, n: int):
    """|fl32(fp64 sum of n terms in any order) - S| <= this (module docstring)."""
    return U32 * np.abs(S) + gamma(n) * A + 2.0 ** -149


def bound64(S, A, n: int):
    """The same before the cast to fp32 (the window form's fp64 partial rows), plus the
    half-ulp by which S itself, an fp64 number, may differ from the exact sum."""
    return gamma(n) * A + U64 * np.abs(S)


def check_ranges(ex: dict) -> None:
    """The assumptions of :func:`bound`'s first-order form, for the finite sums of a case."""
    for name, o in ex.items():
        assert 0 <= o["n"] <= MAX_TERMS, (name, o["n"])
        fin = np.isfinite(o["A"])
        assert (np.abs(o["S"][fin]) + o["A"][fin] < MAX_MAGNITUDE).all(), name


# ---------------------------------------------------------------------------------------
# the edge_attr gradient
# ---------------------------------------------------------------------------------------
def pow2ceil(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


def edge_grad(dm, W, L: int) -> tuple:
    """``dm`` [E, D] fp32, ``W`` [D, K], ``L`` = pow2ceil(D / 4) lanes per row group.

    Returns (the kernel's fp32 value [E, K], bit for bit; the value in fp64; sum_c |dm_c W_ck|;
    the fp64 value's own error bound).  The fp32 value is within ``(log2 L + 3) 2^-24`` of the
    sum of absolute products: three roundings in the lane (product, pair sum, sum of pairs)
    and one per butterfly level; the linear form ``h u sum |t|`` holds without higher-order
    terms for a summation tree of height h (Jeannerod and Rump, 2013), underflow aside.  The
    fp64 value is a plain fp64 sum of D exact products: within ``D 2^-53`` of the same sum."""
    dm = np.asarray(dm, F32)
    W = np.asarray(W, F32).reshape(dm.shape[1], -1)
    E, D = dm.shape
    K = W.shape[1]
    assert D % 4 == 0 and L == pow2ceil(D // 4)
    got = np.zeros((E, K), F32)
    ref = np.zeros((E, K))
    mag = np.zeros((E, K))
    with np.errstate(all="ignore"):
        for k in range(K):
            p = (dm * W[None, :, k]).astype(F32).reshape(E, D // 4, 4)
            lane = (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])
            s = np.zeros((E, L), F32)
            s[:, :D // 4] = lane
            while s.shape[1] > 1:
                s = s[:, 0::2] + s[:, 1::2]
            got[:, k] = s[:, 0]
            p64 = dm.astype(np.float64) * W[None, :, k].astype(np.float64)
            ref[:, k] = p64.sum(axis=1)
            mag[:, k] = np.abs(p64).sum(axis=1)
    return got, ref, mag, D * U64 * mag


def edge_grad_bound(mag, L: int):
    return (int(math.log2(L)) + 3) * U32 * mag


# ---------------------------------------------------------------------------------------
# comparison helpers shared by the CPU and the device tests
# ---------------------------------------------------------------------------------------
def same_bits(a, b) -> bool:
    """fp32 arrays equal value for value (+0 / -0 apart), NaN matching NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def held(got, o: dict) -> tuple:
    """``got`` (fp32 output) against one entry of :func:`exact`: (ok, worst error / bound over
    the finite sums, outputs that are not the correctly rounded S).  A sum with a non-finite
    term must reproduce the oracle's NaN / infinity exactly."""
    got = np.asarray(got, np.float64).reshape(o["S"].shape)
    fin = np.isfinite(o["A"])
    ok = same_bits(got[~fin].astype(F32), o["S"][~fin].astype(F32))
    with np.errstate(all="ignore"):
        ratio = np.abs(got[fin] - o["S"][fin]) / bound(o["S"][fin], o["A"][fin], o["n"])
    ok = ok and bool(np.isfinite(got[fin]).all()) and bool((ratio <= 1.0).all())
    worst = float(ratio.max()) if ratio.size else 0.0
    misrounded = int((got[fin].astype(F32) != o["r32"][fin]).sum())
    return ok, worst, misrounded
