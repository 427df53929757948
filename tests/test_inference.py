"""CPU: the eval-mode layer's ABI (gine_mp_fwd_layer_eval) and raincast_gnn.inference /
evaluate(fused=True) on a model that runs on the CPU (the oracle's GNN: a CPU model is simply
called, so the Predictor and the in-place checkpoint ensemble must change nothing)."""
import ctypes
import os
import re

import torch

from conftest import ROOT
from oracle import gine_cpu as O
from raincast_gnn import _lib
from raincast_gnn.data import synthetic_batch
from raincast_gnn.evaluate import predict_ensemble, predict_model
from raincast_gnn.inference import Predictor

NAME = "gine_mp_fwd_layer_eval"


def _make():
    return O.OracleGNN(35, 128, 2, "MixedLoss", "False", 1.71, 0.5)


def _states(batches):
    """Two checkpoints with different weights and non-trivial running statistics."""
    out = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        m = _make().train()
        with torch.no_grad():
            for b in batches:
                m(b)  # train mode: the BatchNorms' running statistics move
        out.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    return out


def test_header_binding_and_library_export_the_eval_layer():
    text = open(os.path.join(ROOT, "include", "gine_hip.h")).read()
    assert re.search(r"^int\s+%s\s*\(" % NAME, text, re.M)
    assert re.search(r"#define GINE_ABI_VERSION 10\b", text)
    assert NAME in _lib.EXPORTED_SYMBOLS and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert hasattr(lib, NAME) and lib.gine_abi_version() == 10
    assert len(_lib._SIGNATURES[NAME]) == 25


def test_eval_layer_validates_without_device():
    """Every rejection comes before any HIP call: channels, degree, flag, epilogue, NULL edge
    attributes / running statistics / y without a head, N < 0; N = 0 is ok."""
    f = _lib.load().gine_mp_fwd_layer_eval
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
    assert call(degree=deg + 1) == _lib.GINE_ERR_INVALID
    assert call(degree=-1) == _lib.GINE_ERR_INVALID
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


def test_predictor_on_a_cpu_model_is_the_model():
    batches = [synthetic_batch(40, 2, k=4, seed=s) for s in (3, 4)]
    model = _make()
    model.load_state_dict(_states(batches)[0])
    model.train()
    pred = Predictor(model)
    assert not model.training                       # the Predictor puts it in eval mode
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for b in batches:
        got = pred(b)
        with torch.no_grad():
            want = model.eval()(b)
        assert not got.requires_grad and torch.equal(got, want)
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)   # no side effects
    assert torch.equal(predict_model(model, batches, "cpu", fused=True),
                       predict_model(model, batches, "cpu"))


def test_fused_ensemble_equals_default_and_reloads_in_place():
    batches = [synthetic_batch(40, 2, k=4, seed=s) for s in (3, 4)]
    states = _states(batches)
    made = []

    def make():
        made.append(_make())
        return made[-1]
    want = predict_ensemble(make, states, batches, "cpu")
    assert len(made) == 2
    del made[:]
    got = predict_ensemble(make, states, batches, "cpu", fused=True)
    assert torch.equal(got, want)
    assert len(made) == 1                           # one model, every checkpoint loaded into it
    last = made[0].state_dict()
    assert all(torch.equal(last[k], states[-1][k]) for k in states[-1])
    assert not torch.equal(states[0]["aggr.weight"], states[1]["aggr.weight"])
