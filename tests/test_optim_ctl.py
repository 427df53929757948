"""CPU: the device-controlled AdamW step (gine_grad_sumsq / gine_adamw_step_ctl, DESIGN.md
6d) as far as it goes without a device: the symbols, the host-side argument validation (which
returns before any HIP call), the host restatement of the schedule and the optional
``params.json`` keys.  The kernels themselves: tests/test_gpu_optim_ctl.py."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from raincast_gnn import _lib
from raincast_gnn.params import EXPERIMENTS, load_params

NEW = ("gine_grad_sumsq_num_partials", "gine_grad_sumsq", "gine_adamw_step_ctl",
       "gine_adamw_ctl_bytes")


def _aligned(nbytes=256):
    """A host buffer and a 16-byte aligned address inside it (never dereferenced)."""
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_symbols_declared_exported_bound_and_abi_still_10():
    header = open(os.path.join(ROOT, "include", "gine_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", header, re.M), name
        assert name in _lib._SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define GINE_ABI_VERSION 10\b", header)
    assert lib.gine_abi_version() == _lib.ABI_VERSION == 10
    cb, rb = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.gine_adamw_ctl_bytes(ctypes.byref(cb), ctypes.byref(rb)) == 0
    assert cb.value == ctypes.sizeof(_lib.AdamWCtl) == 28
    assert rb.value == ctypes.sizeof(_lib.AdamWReport) == 16
    assert lib.gine_adamw_ctl_bytes(None, ctypes.byref(rb)) == 1


def test_num_partials_is_monotone_and_capped():
    lib = _lib.load()
    num = ctypes.c_int32(-1)
    assert lib.gine_grad_sumsq_num_partials(-1, ctypes.byref(num)) == 1
    assert lib.gine_grad_sumsq_num_partials(8, None) == 1
    last = 0
    for n in (0, 1, 4, 1024, 1025, 3 * 1024 + 3, 13 * 1024 - 40, 209_800, 512 * 1024,
              512 * 1024 + 1, 600_000, 10 ** 6, 2 ** 31 + 5):
        assert lib.gine_grad_sumsq_num_partials(n, ctypes.byref(num)) == 0
        assert last <= num.value <= 512, n
        assert num.value == min(512, -(-(-(-n // 4)) // 256)), n   # the step's grid rule
        last = num.value
    assert last == 512


def test_grad_sumsq_validates_before_any_hip_call():
    lib = _lib.load()
    keep, p = _aligned()
    f = lib.gine_grad_sumsq
    assert f(None, 0, None, 0, None) == 0             # nothing to do, nothing launched
    assert f(p, -1, p, 0, None) == 1
    assert f(None, 1000, p, 1, None) == 1
    assert f(p, 1000, None, 1, None) == 1
    assert f(p + 4, 1000, p, 1, None) == 1            # float4 loads
    assert f(p, 1000, p + 8, 1, None) == 1            # 16-byte partial rows
    assert f(p, 1000, p, 2, None) == 1                # 1000 elements: one partial
    assert f(p, 2000, p, 1, None) == 1                # 2000 elements: two
    assert f(p, 0, p, 1, None) == 1
    del keep


def test_adamw_step_ctl_validates_before_any_hip_call():
    lib = _lib.load()
    keep, p = _aligned()
    f = lib.gine_adamw_step_ctl
    tail = (0.9, 0.999, 1e-8, 0.01, None)

    def call(param=p, grad=p, m=p, v=p, step=p, n=1000, ctl=p, partials=p, num=1, report=p):
        return f(param, grad, m, v, step, n, ctl, partials, num, report, *tail)

    assert call(n=-1) == 1
    for name in ("param", "grad", "m", "v", "step", "ctl", "report"):
        assert call(**{name: None}) == 1, name
    for name in ("param", "grad", "m", "v", "partials"):
        assert call(**{name: p + 4}) == 1, name       # float4 / double2 accesses
    assert call(ctl=p + 2) == 1 and call(report=p + 1) == 1
    assert call(num=2) == 1 and call(num=0) == 1      # must be the query's count
    assert call(n=2000, num=1) == 1
    assert call(partials=None, num=1) == 1            # no partials: the count is 0
    del keep


def test_lr_at_follows_the_schedule():
    from raincast_gnn.optim import Schedule, lr_at
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    lr, W, T, r = 3e-3, 3, 8, 0.1
    base = f32(lr)
    assert lr_at(None, lr, 5) == base
    assert lr_at(Schedule("constant", W, T, r), lr, 1) == base
    assert lr_at(Schedule("constant"), lr, 10 ** 6) == base
    for kind in ("cosine", "linear"):
        s = Schedule(kind, W, T, r)
        assert lr_at(s, lr, 1) == f32(base * 1.0 / 3.0)            # warm-up: lr * t / W
        assert lr_at(s, lr, W) == base                              # its last step: full
        x = 1.0 / 5.0                                               # t = W + 1
        shape = 0.5 * (1.0 + math.cos(math.pi * x)) if kind == "cosine" else 1.0 - x
        rr = f32(r)
        assert lr_at(s, lr, W + 1) == f32(base * (rr + (1.0 - rr) * shape))
        assert lr_at(s, lr, W + 1) < base
        floor = f32(base * rr)
        assert abs(lr_at(s, lr, T) - floor) <= np.spacing(np.float32(floor))
        assert lr_at(s, lr, T) == lr_at(s, lr, T + 1) == lr_at(s, lr, 10 * T)
        rates = [lr_at(s, lr, t) for t in range(W, T + 1)]
        assert all(a > b for a, b in zip(rates, rates[1:]))         # decays from W to T
    # no warm-up and T <= W: the rate sits at its floor from the first step
    assert lr_at(Schedule("cosine", 0, 0, 0.0), lr, 1) == pytest.approx(0.0, abs=1e-18)
    # every result is an fp32 value
    for t in range(1, 12):
        v = lr_at(Schedule("cosine", W, T, r), lr, t)
        assert v == f32(v)
    with pytest.raises(ValueError):
        Schedule("exponential")


def test_load_params_takes_the_optional_keys_and_leaves_reference_files_alone(tmp_path):
    path = tmp_path / "params.json"
    assert len(EXPERIMENTS) == 12
    for name, cfg in EXPERIMENTS.items():
        path.write_text(json.dumps(cfg))
        got = load_params(str(path))
        assert got == cfg and "max_grad_norm" not in got and "lr_schedule" not in got, name
    cfg = dict(EXPERIMENTS["24h_mixed"], max_grad_norm=1.5,
               lr_schedule={"kind": "cosine", "warmup_steps": 10, "min_lr_ratio": 0.05})
    path.write_text(json.dumps(cfg))
    assert load_params(str(path)) == cfg
    for bad in ({"max_grad_norm": 0}, {"max_grad_norm": "1"}, {"lr_schedule": "cosine"},
                {"lr_schedule": {"kind": "step"}}, {"lr_schedule": {"warmup_steps": 3}},
                {"lr_schedule": {"kind": "linear", "gamma": 0.1}},
                {"lr_schedule": {"kind": "linear", "warmup_steps": -1}}):
        path.write_text(json.dumps(dict(EXPERIMENTS["24h_mixed"], **bad)))
        with pytest.raises(ValueError, match="params.json"):
            load_params(str(path))


def test_train_cli_has_the_new_flags(capsys):
    from raincast_gnn import train as T
    with pytest.raises(SystemExit):
        T.main(["--help"])
    text = capsys.readouterr().out
    for flag in ("--max-grad-norm", "--schedule", "--warmup-steps", "--resume"):
        assert flag in text
    assert T.opt_state_path("/x/models/run_7-best.ckpt") == "/x/models/run_7-best.opt"
