"""The graphs of the any-in-degree eval layer's tests (gine_mp_fwd_layer_eval_deep), shared by
tests/test_gpu_inference_deep.py (which runs them) and tests/test_inference_deep.py (which
checks on the CPU that they hold the in-degrees they are named for)."""
from __future__ import annotations

import torch

from helpers import knn_batch_graph, radius_graph

# In-degree of every row of the ladder graph.  The gather role sums rows r and r + 16 of a
# 32-row tile as a pair, walking max(chunks of r, chunks of r + 16) chunks of 32 slots, so the
# pairs here are: no chunk | four (0 | 97), exactly one | one slot into the second (32 | 33),
# 1 | 65, 31 | 64, 63 | 0, 64 | 33, 65 | 1 and 97 | 97; a second tile of 8 rows follows.
LADDER_TILE0 = {0: 0, 16: 97, 1: 32, 17: 33, 2: 1, 18: 65, 3: 31, 19: 64, 4: 63, 20: 0,
                5: 64, 21: 33, 6: 65, 22: 1, 7: 97, 23: 97}
LADDER_TILE1 = {32: 33, 33: 0, 34: 70, 39: 32}
LADDER_NODES = 40
LADDER_PAIRS = ((0, 97), (32, 33), (1, 65), (31, 64), (63, 0))
LADDER_DEGREES = (0, 1, 31, 32, 33, 63, 64, 65, 97)


def ladder_degrees() -> list[int]:
    deg = [3] * LADDER_NODES
    for table in (LADDER_TILE0, LADDER_TILE1):
        for row, d in table.items():
            deg[row] = d
    return deg


def ladder_graph():
    """A multigraph with the in-degrees above: random sources (self loops and repeats among
    them), random attributes, the edges in shuffled order."""
    g = torch.Generator().manual_seed(11)
    deg = torch.tensor(ladder_degrees())
    dst = torch.repeat_interleave(torch.arange(LADDER_NODES), deg)
    src = torch.randint(0, LADDER_NODES, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)
    ea = torch.rand(dst.numel(), 1, generator=g) * 3.5 + 0.5
    return torch.stack([src, dst])[:, perm].contiguous(), ea[perm].contiguous(), LADDER_NODES


def one_node_graph(loops: int = 40):
    g = torch.Generator().manual_seed(5)
    return torch.zeros(2, loops, dtype=torch.long), torch.rand(loops, 1, generator=g) + 0.5, 1


def layer_graphs():
    """(name, edge_index, edge_attr, N, (least, largest) in-degree the name claims)."""
    out = []
    for n, k in ((40, 32), (70, 63), (70, 64), (130, 96)):
        ei, ea, nn = knn_batch_graph(n, k, 1, seed=n)
        out.append(("knn%d_k%d" % (n, k), ei, ea, nn, (k + 1, k + 1)))
    out.append(("radius300_400km", *radius_graph(300, 400.0, seed=2), (17, 83)))
    out.append(("ladder", *ladder_graph(), (0, 97)))
    out.append(("one_node_40_loops", *one_node_graph(40), (40, 40)))
    ei, ea, nn = knn_batch_graph(33, 6, 1, seed=33)
    out.append(("knn33_k6_within_limit", ei, ea, nn, (7, 7)))
    return out


def rounds_graph():
    """7 tiles (the last with 8 rows), in-degrees 26 .. 113."""
    return radius_graph(200, 600.0, seed=2)


REDO_HUBS = ((5, 68), (40, 69))   # (hub row, the source its last in-edge comes from)


def redo_graph():
    """knn(70, 6) (in-degree 7) with 40 more in-edges on rows 5 and 40 (in-degree 47), the last
    of them -- slot 14 of the row's second chunk, the CSR keeps the edge order within a row --
    from node 68 and 69: what few rows read, so a NaN there leaves most of the output finite."""
    ei, ea, n = knn_batch_graph(70, 6, 1, seed=70)
    g = torch.Generator().manual_seed(13)
    extra = []
    for hub, last in REDO_HUBS:
        src = torch.cat([torch.randint(0, 60, (39,), generator=g), torch.tensor([last])])
        extra.append(torch.stack([src, torch.full((40,), hub)]))
    ei = torch.cat([ei] + extra, 1)
    ea = torch.cat([ea, torch.rand(80, 1, generator=g) * 3.5 + 0.5])
    return ei, ea, n


def in_degrees(ei: torch.Tensor, n: int) -> torch.Tensor:
    return torch.bincount(ei[1], minlength=n) if ei.numel() else torch.zeros(n, dtype=torch.long)
