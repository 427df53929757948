"""Shared restatement and inputs of the edge_dim > 1 tests (tests/test_edge_dim.py on the
CPU, tests/test_gpu_edge_dim.py on the device).

The engine's definition of the K-wide edge Linear is a chain of K fused multiply-adds,
``e = b; e = fma(a[k], W[:, k], e)`` for k = 0 .. K-1, one fp32 rounding per term.
:func:`chain_lin` restates it in torch: the product of two fp32 values is exact in fp64 and
the sum is rounded once to fp32 (differentiable through the casts).  With fp64 inputs the
same code is the fp64 reference.  :func:`aggregate_chain` is ``oracle.gine_cpu.gine_aggregate``
with that Linear in place of ``F.linear`` (a BLAS sgemm whose summation order is its own for
K > 1, so torch's CPU Linear is only close to it, not bit-equal).
"""
from __future__ import annotations

import functools

import torch

from helpers import special_graphs


def chain_lin(ea: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[E, K] x [D, K] (lin.weight's layout) + [D] -> [E, D], one rounding to ``b.dtype`` per
    term, k ascending."""
    e = b.expand(ea.size(0), -1)
    for k in range(W.size(1)):
        e = (ea[:, k:k + 1].double() * W[:, k].double() + e.double()).to(b.dtype)
    return e


def aggregate_chain(x, ei, ea, W, b, eps):
    """z = scatter_add(relu(x[src] + chain_lin(a)), dst) + (1 + eps) * x (PyG's op sequence,
    as oracle.gine_cpu.gine_aggregate)."""
    src, dst = ei[0], ei[1]
    m = (x.index_select(0, src) + chain_lin(ea.reshape(-1, W.size(1)), W, b)).relu()
    agg = x.new_zeros(x.size(0), m.size(1)).scatter_add_(0, dst.view(-1, 1).expand_as(m), m)
    return agg + (1 + eps) * x


def widen(ea: torch.Tensor, K: int, seed: int = 0) -> torch.Tensor:
    """[E, 1] attributes -> [E, K]: the graph's own column, then K - 1 seeded randn columns."""
    ea = ea.reshape(-1, 1).float()
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.cat([ea, torch.randn(ea.size(0), K - 1, generator=g)], dim=1)


def mp_params(D: int, K: int, seed: int = 0, eps: float = 0.25):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(D, K, generator=g) * 0.5
    b = torch.randn(D, generator=g) * 0.5
    return W, b, torch.tensor([eps])


GRAPHS = {name: (ei, ea, n) for name, ei, ea, n in special_graphs()}
GRAPH_NAMES = tuple(GRAPHS)
# (D, K): D = 4 is one lane per node, 36 a 16-lane group with padding lanes, 256 the widest
SHAPES = ((4, 2), (36, 3), (64, 8), (128, 1), (128, 2), (128, 5), (256, 8))


@functools.lru_cache(maxsize=None)
def mp_case(name: str, D: int, K: int) -> dict:
    """Inputs and the CPU references of one message-passing case, computed once: z, and the
    fp32 / fp64 autograd gradients of (z * dz).sum() through :func:`aggregate_chain`."""
    ei, ea, n = GRAPHS[name]
    ea = widen(ea, K, seed=D + K)
    g = torch.Generator().manual_seed(7 * D + K)
    x = torch.randn(n, D, generator=g)
    dz = torch.randn(n, D, generator=g)
    W, b, eps = mp_params(D, K, seed=D + 3 * K)
    out = {"ei": ei, "ea": ea, "n": n, "x": x, "dz": dz, "W": W, "b": b, "eps": eps}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        leaves = [t.detach().to(dt).requires_grad_(True) for t in (x, ea, W, b, eps)]
        z = aggregate_chain(leaves[0], ei, leaves[1], leaves[2], leaves[3], leaves[4])
        z.backward(dz.to(dt))
        grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]
        out["z" + tag] = z.detach()
        out["g" + tag] = dict(zip(("x", "ea", "W", "b", "eps"), grads))
    return out
