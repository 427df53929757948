"""CPU: the ABI of the eval-mode layer at any in-degree (gine_mp_fwd_layer_eval_deep) and the
in-degrees of the graphs tests/test_gpu_inference_deep.py runs it on."""
import ctypes
import os
import re

import torch

import deep_cases
from conftest import ROOT
from raincast_gnn import _lib

NAME = "gine_mp_fwd_layer_eval_deep"


def test_header_binding_and_library_export_the_deep_eval_layer():
    text = open(os.path.join(ROOT, "include", "gine_hip.h")).read()
    assert re.search(r"^int\s+%s\s*\(" % NAME, text, re.M)
    assert re.search(r"#define GINE_ABI_VERSION 10\b", text)       # additive: still ABI 10
    assert NAME in _lib.EXPORTED_SYMBOLS and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert hasattr(lib, NAME) and lib.gine_abi_version() == 10
    assert len(_lib._SIGNATURES[NAME]) == 25
    assert _lib._SIGNATURES[NAME] == _lib._SIGNATURES["gine_mp_fwd_layer_eval"]


def test_deep_eval_layer_validates_without_device():
    """test_eval_layer_validates_without_device's rejections, each before any HIP call, except
    the degree one: 33 and 1 << 20 are not refused on that ground (shown with N = 0, which
    returns OK after the validation and before any HIP call), -1 is."""
    f = getattr(_lib.load(), NAME)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    deg = _lib.MP_FUSED_MAX_DEGREE

    def call(ptrs=None, bn_eps=1e-5, n=100, d=128, degree=5, flags=0, epi=1, head=None, wg=0):
        a = list(ptrs) if ptrs is not None else [p] * 16
        return f(*a[:13], bn_eps, *a[13:16], n, d, degree, flags, epi, head, wg, None)

    def without(i):
        a = [p] * 16
        a[i] = None
        return a
    assert call(d=64) == _lib.GINE_ERR_DIM
    assert call(d=256) == _lib.GINE_ERR_DIM
    assert call(degree=-1) == _lib.GINE_ERR_INVALID
    assert call(degree=-1, n=0) == _lib.GINE_ERR_INVALID
    for degree in (deg, deg + 1, 1 << 20):
        assert call(degree=degree, n=0) == _lib.GINE_OK
        # the degree is no ground for refusal: another argument's error is what comes back
        assert call(degree=degree, n=1 << 23) == _lib.GINE_ERR_TOO_LARGE
    # ... while the entry with the limit does refuse it
    old = _lib.load().gine_mp_fwd_layer_eval
    assert old(*([p] * 13), 1e-5, p, p, p, 0, 128, deg + 1, 0, 1, None, 0,
               None) == _lib.GINE_ERR_INVALID
    assert call(flags=8) == _lib.GINE_ERR_INVALID
    assert call(flags=1) == _lib.GINE_ERR_INVALID
    assert call(epi=3) == _lib.GINE_ERR_INVALID
    assert call(epi=-1) == _lib.GINE_ERR_INVALID
    assert call(without(3)) == _lib.GINE_ERR_INVALID           # no edge attributes
    assert call(without(11)) == _lib.GINE_ERR_INVALID          # no running mean
    assert call(without(12)) == _lib.GINE_ERR_INVALID          # no running var
    assert call(without(15)) == _lib.GINE_ERR_INVALID          # y = NULL without a head
    assert call(n=-1) == _lib.GINE_ERR_INVALID
    assert call(wg=-1) == _lib.GINE_ERR_INVALID
    head = _lib.LayerHead(p, p, p, p, None, None, 7)
    assert call(head=ctypes.byref(head)) == _lib.GINE_ERR_INVALID   # unknown loss kind
    head = _lib.LayerHead(p, p, p, p, None, p, _lib.LOSS_MIXED)
    assert call(head=ctypes.byref(head)) == _lib.GINE_ERR_INVALID   # counts without targets
    assert call(n=1 << 23) == _lib.GINE_ERR_TOO_LARGE               # N * 512 B >= 2^32
    assert call(n=0) == _lib.GINE_OK
    assert call(without(9), n=0) == _lib.GINE_OK                    # gamma may be NULL
    head = _lib.LayerHead(p, p, p, p, None, None, _lib.LOSS_MIXED)
    assert call(without(15), n=0, head=ctypes.byref(head)) == _lib.GINE_OK  # y NULL with a head


def test_deep_degree_coverage():
    """The GPU test's graphs hold the in-degrees they are named for: 33, 64, 65 and 97
    everywhere, 17 .. 83, the ladder's nine degrees with its pairs at rows r and r + 16 of one
    tile, 40 self loops on one node, 7 within the old limit; 26 .. 113 over 7 tiles for the
    rounds."""
    cases = {name: (ei, n, claim) for name, ei, _, n, claim in deep_cases.layer_graphs()}
    for name, (ei, n, claim) in cases.items():
        d = deep_cases.in_degrees(ei, n)
        assert (int(d.min()), int(d.max())) == claim, (name, int(d.min()), int(d.max()))
        assert int(ei.max()) < n and int(ei.min()) >= 0
    assert {c[2][1] for c in cases.values()} >= {33, 64, 65, 97, 83, 40, 7}
    assert cases["knn130_k96"][1] == 130                       # five tiles, the last with two rows
    ei, n, _ = cases["radius300_400km"]
    d = deep_cases.in_degrees(ei, n)                           # below and above the limit in one tile
    assert any(int(t.min()) <= 32 < int(t.max()) for t in d.split(32))
    ei, n, _ = cases["ladder"]
    d = deep_cases.in_degrees(ei, n).tolist()
    assert d == deep_cases.ladder_degrees()
    assert set(deep_cases.LADDER_DEGREES) <= set(d)
    pairs = {(d[r], d[r + 16]) for r in range(16)}
    assert set(deep_cases.LADDER_PAIRS) <= pairs
    assert (0, 97) in pairs and (32, 33) in pairs
    assert cases["one_node_40_loops"][1] == 1
    ei, _, n = deep_cases.redo_graph()
    d = deep_cases.in_degrees(ei, n)
    assert all(int(d[hub]) == 47 for hub, _ in deep_cases.REDO_HUBS)
    assert int(d.max()) == 47 and int((d > 32).sum()) == 2
    for hub, last in deep_cases.REDO_HUBS:     # the marked source is the hub's last edge
        assert int(ei[0][ei[1] == hub][-1]) == last
    ei, _, n = deep_cases.rounds_graph()
    d = deep_cases.in_degrees(ei, n)
    assert (int(d.min()), int(d.max())) == (26, 113) and (n + 31) // 32 == 7 and n % 32 == 8


def test_deep_predicate_and_policy_constant_exist():
    from raincast_gnn import inference
    assert callable(inference.layer_eval_deep) and callable(inference.layer_eval_deep_ok)
    assert hasattr(inference, "DEEP_MAX_NODES")
    assert inference.DEEP_MAX_NODES is None or inference.DEEP_MAX_NODES > 0
