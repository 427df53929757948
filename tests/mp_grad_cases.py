"""Cases of the message-passing gradient oracle tests (tests/test_mp_grad_oracle.py on the
CPU, tests/test_gpu_mp_grads.py on the device), as small as still reach each branch of the
kernels, and the oracle of each case computed once (tests/mp_grad_oracle.py).

A case is a dict: ``ei`` [2, E] and ``ea`` [E, K] (the caller's edge list, unsorted), ``n``,
``x``, ``dz``, ``dres`` [N, D], ``W`` [D, K], ``b`` [D], ``eps`` (float), ``mode`` ("fma" |
"muladd"), all numpy.  :func:`out_csr` is the stable source-sorted CSR the engine's graph
build produces (held to that by the graph-build tests).
"""
from __future__ import annotations

import functools

import numpy as np

import mp_grad_oracle as MO
from edge_dim_cases import SHAPES
from helpers import special_graphs

F32 = np.float32
EPS = 0.25

# neighbour rows in flight per lane (the full-batch / tail split of the edge loop)
GATHER_D = (4, 36, 64, 128, 256, 260, 516)
WIN_U = 6                                       # gine_mpwin.hip kWinUnroll
WIN_SHAPES = ((128, 32), (48, 16))              # (D, slice_channels): DPP / shuffle reduction
CAP_N, CAP_D, CAP_K, CAP_PARTIALS = 8205, 256, 3, 1024


def gather_shape(D: int) -> tuple:
    """(L, C, U) of gine_mp.hip at D channels: pick_shape and MpUnrollBwd."""
    d4 = D // 4
    if d4 <= 64:
        return MO.pow2ceil(d4), 1, 6
    C = (d4 + 63) // 64
    return 64, C, 4 if C == 2 else 2


def ek_shape(D: int, K: int) -> tuple:
    """(L, KB, U) of gine_mpek.hip: pick_group, bucket and EkUnroll."""
    KB = 1 if K <= 1 else 2 if K <= 2 else 4 if K <= 4 else 8
    return MO.pow2ceil(D // 4), KB, 6 if KB <= 4 else 4


def planted_degrees(U: int, L: int) -> list:
    return sorted({d for d in (0, 1, U - 1, U, U + 1, L - 1, L, L + 1, 2 * L + 1) if d >= 0})


@functools.lru_cache(maxsize=None)
def planted_graph(U: int, L: int):
    """Multigraph whose out-degrees are exactly planted_degrees(U, L) (node i has the i-th),
    plus two nodes that only receive; every node with an out-edge has a self-loop, every node
    with three or more a duplicated edge; the edge list is shuffled (unsorted)."""
    degs = planted_degrees(U, L)
    rng = np.random.default_rng(1000 * U + L)
    n = len(degs) + 2
    src = np.repeat(np.arange(len(degs)), degs)
    dst = rng.integers(0, n, src.size)
    start = 0
    for i, d in enumerate(degs):
        if d >= 1:
            dst[start] = i
        if d >= 3:
            dst[start + 2] = dst[start + 1]
        start += d
    perm = rng.permutation(src.size)
    ei = np.stack([src[perm], dst[perm]]).astype(np.int64)
    ea = rng.uniform(0.5, 4.0, (src.size, 1)).astype(F32)
    return ei, ea, n


@functools.lru_cache(maxsize=None)
def helper_graphs() -> dict:
    return {name: (ei.numpy().astype(np.int64), ea.numpy().astype(F32).reshape(-1, 1), n)
            for name, ei, ea, n in special_graphs()}


@functools.lru_cache(maxsize=None)
def capped_graph():
    """8,205 nodes, in-degree about 5: at D = 256 (4 nodes per workgroup) 2,052 tiles, the
    last one partial (one node), on a grid capped at 1,024 workgroups."""
    rng = np.random.default_rng(8205)
    E = 5 * CAP_N
    ei = np.stack([rng.integers(0, CAP_N, E), rng.integers(0, CAP_N, E)]).astype(np.int64)
    return ei, rng.uniform(0.5, 4.0, (E, 1)).astype(F32), CAP_N


def out_csr(ei: np.ndarray, n: int) -> tuple:
    """(rowptr [n + 1], perm [E]): slot s of the out-CSR holds the caller's edge perm[s]."""
    perm = np.argsort(ei[0], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int64)
    return rowptr, perm


def _base(graph, D: int, K: int, mode: str, seed: int) -> dict:
    ei, ea, n = graph
    rng = np.random.default_rng(seed)
    E = ei.shape[1]
    ea = np.concatenate([ea.reshape(E, 1), rng.standard_normal((E, K - 1)).astype(F32)], axis=1)
    return {"ei": ei, "ea": ea, "n": n, "mode": mode, "eps": EPS,
            "x": rng.standard_normal((n, D)).astype(F32),
            "dz": rng.standard_normal((n, D)).astype(F32),
            "dres": rng.standard_normal((n, D)).astype(F32),
            "W": (0.5 * rng.standard_normal((D, K))).astype(F32),
            "b": (0.5 * rng.standard_normal(D)).astype(F32)}


def _sums(c: dict) -> dict:
    rowptr, perm = out_csr(c["ei"], c["n"])
    return MO.node_sums(c["x"], c["dz"], rowptr, c["ei"][1][perm], c["ea"][perm], c["W"], c["b"],
                        c["mode"])


def _scaled(c: dict) -> dict:
    """Channel c carries the scale 2^(-20 + 40 c / (D - 1)) (x, W, b and dz: powers of two, so
    the decisions are those of the unscaled case and every scaling is exact)."""
    D = c["x"].shape[1]
    s = np.exp2(np.round(np.linspace(-20.0, 20.0, D))).astype(F32)
    c = dict(c)
    c["x"], c["dz"], c["b"] = c["x"] * s, c["dz"] * s, c["b"] * s
    c["W"] = c["W"] * s[:, None]
    c["scales"] = s
    return c


def _cancelling(c: dict) -> dict:
    """dz planted so that db of the first D / 2 channels cancels: db_c = sum_v dz[v, c]
    cnt[v, c] with cnt the number of in-edges of v whose decision is on (no function of dz),
    and nodes are paired (v1, v2) with dz = (t cnt[v2], -t cnt[v1]), t a 12-bit value, so the
    exact terms cancel and what is left of S is the per-node fp32 rounding."""
    c = dict(c)
    on = _sums(c)["on"]
    rowptr, perm = out_csr(c["ei"], c["n"])
    dst = c["ei"][1][perm]
    D = c["x"].shape[1]
    cnt = np.zeros((c["n"], D), np.int64)
    np.add.at(cnt, dst, on.astype(np.int64))
    rng = np.random.default_rng(77)
    dz = c["dz"].copy()
    planted = np.arange(D // 2)
    for ch in planted:
        vs = np.nonzero(cnt[:, ch])[0]
        rng.shuffle(vs)
        for v1, v2 in zip(vs[0::2], vs[1::2]):
            t = F32(rng.integers(1, 4096)) * F32(2.0 ** -10)
            dz[v1, ch], dz[v2, ch] = t * F32(cnt[v2, ch]), -t * F32(cnt[v1, ch])
        if len(vs) % 2:
            dz[vs[-1], ch] = F32(2.0 ** -30)
    c["dz"], c["planted"] = dz, planted
    return c


def _nonfinite(c: dict) -> dict:
    c = dict(c)
    x, dz = c["x"].copy(), c["dz"].copy()
    x[3, 5] = np.nan
    x[10, :7] = np.inf
    x[20, 40:] = -np.inf
    x[33, 1] = np.nan
    dz[7, 2] = np.nan
    dz[12, 9], dz[13, 9] = np.inf, -np.inf
    dz[30, 20] = np.inf
    dz[41, 50] = -np.inf
    c["x"], c["dz"] = x, dz
    return c


# ---------------------------------------------------------------------------------------
# the case tables: name -> builder
# ---------------------------------------------------------------------------------------
def _gather_table() -> dict:
    t = {}
    for D in GATHER_D:
        L, C, U = gather_shape(D)
        for mode in ("fma", "muladd"):
            t[f"planted_D{D}_{mode}"] = functools.partial(
                lambda D, U, L, mode: _base(planted_graph(U, L), D, 1, mode, 11 * D), D, U, L, mode)
    for i, name in enumerate(helper_graphs()):
        for D in (36, 128):
            t[f"{name}_D{D}"] = functools.partial(
                lambda name, D, i: _base(helper_graphs()[name], D, 1, "fma", 500 + 7 * i + D),
                name, D, i)
    knn64 = lambda: _base(helper_graphs()["knn64_k4"], 64, 1, "fma", 64)  # noqa: E731
    t["scaled_D64"] = lambda: _scaled(knn64())
    t["cancelling_D64"] = lambda: _cancelling(knn64())
    t["nonfinite_D64"] = lambda: _nonfinite(knn64())
    t["capped_D256"] = lambda: _base(capped_graph(), CAP_D, 1, "fma", 8205)
    return t


def _ek_table() -> dict:
    t = {}
    for D, K in SHAPES:
        L, KB, U = ek_shape(D, K)
        t[f"planted_D{D}_K{K}"] = functools.partial(
            lambda D, K, U, L: _base(planted_graph(U, L), D, K, "fma", 13 * D + K), D, K, U, L)
    for i, name in enumerate(helper_graphs()):
        t[f"{name}_D36_K3"] = functools.partial(
            lambda name, i: _base(helper_graphs()[name], 36, 3, "fma", 900 + i), name, i)
    knn64 = lambda: _base(helper_graphs()["knn64_k4"], 64, 3, "fma", 643)  # noqa: E731
    t["scaled_D64_K3"] = lambda: _scaled(knn64())
    t["cancelling_D64_K3"] = lambda: _cancelling(knn64())
    t["nonfinite_D64_K3"] = lambda: _nonfinite(knn64())
    t["capped_D256_K3"] = lambda: _base(capped_graph(), CAP_D, CAP_K, "fma", 8206)
    return t


def _win_table() -> dict:
    t = {}
    for D, cs in WIN_SHAPES:
        for mode in ("fma", "muladd"):
            t[f"planted_D{D}_{mode}"] = functools.partial(
                lambda D, mode: _base(planted_graph(WIN_U, 32), D, 1, mode, 17 * D), D, mode)
        for name in ("knn500_k10_b2", "hubs_unsorted", "no_edges"):
            t[f"{name}_D{D}"] = functools.partial(
                lambda name, D: _base(helper_graphs()[name], D, 1, "fma", 300 + D), name, D)
    return t


TABLES = {"gather": _gather_table(), "ek": _ek_table(), "win": _win_table()}
GATHER, EK, WIN = (tuple(TABLES[k]) for k in ("gather", "ek", "win"))
# the cases the CPU tests rebuild by brute force or autograd: the small ones
SMALL = {"gather": tuple(n for n in GATHER if not n.startswith(("capped", "hubs", "knn500"))),
         "ek": tuple(n for n in EK if not n.startswith(("capped", "hubs", "knn500")))}


@functools.lru_cache(maxsize=None)
def case(form: str, name: str) -> dict:
    return TABLES[form][name]()


@functools.lru_cache(maxsize=None)
def oracle(form: str, name: str) -> dict:
    """node_sums, exact and (K-wide form) edge_grad of a case, computed once and shared.
    ``dea`` = (fp32 restatement, fp64 value, sum |dm W|, the fp64 value's own error) in the
    caller's edge order."""
    c = case(form, name)
    ns = _sums(c)
    out = {"ns": ns, "ex": MO.exact(ns, c["x"], c["dz"])}
    if form == "ek":
        D = c["x"].shape[1]
        _, perm = out_csr(c["ei"], c["n"])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        out["dea"] = tuple(a[inv] for a in MO.edge_grad(ns["dm"], c["W"], MO.pow2ceil(D // 4)))
    return out
