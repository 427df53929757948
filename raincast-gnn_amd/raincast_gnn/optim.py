"""Flat-buffer AdamW for the benchmarked training step (train.py:67-69).

The reference steps ``torch.optim.AdamW(model.parameters(), lr=params["lr"])`` (train.py:185)
over ~40 small parameter tensors (209,800 fp32 values for 24h_mixed): on a GPU that is a
few hundred tiny launches per step.  :class:`FlatAdamW` re-points every parameter at a view
of ONE contiguous buffer (and every ``.grad`` at a view of one contiguous gradient buffer --
the same buffer the data-parallel all-reduce uses), then updates all of them with one HIP
kernel (``gine_adamw_step``, include/gine_hip.h) that reproduces torch's AdamW arithmetic.

Control mode (any of ``max_grad_norm``, ``schedule``, ``skip_nonfinite``, ``device_control``
given): the learning rate, its schedule, the clipping bound and the skip switch live in a
device control block that ``gine_adamw_step_ctl`` reads on every launch, so a captured step
follows :meth:`FlatAdamW.set_lr` / :meth:`FlatAdamW.set_max_grad_norm` and the schedule on
its next replay; ``gine_grad_sumsq`` supplies the gradient's norm and non-finite count
(DESIGN.md 6d).  Without those arguments nothing changes: one ``gine_adamw_step`` launch with
host scalars.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import asdict, dataclass

import torch

from . import _lib, gradbuf

_KINDS = {"constant": _lib.LR_CONSTANT, "cosine": _lib.LR_COSINE, "linear": _lib.LR_LINEAR}


@dataclass(frozen=True)
class Schedule:
    """Learning-rate schedule evaluated on the device from the step count: ``kind`` is
    "constant", "cosine" or "linear" (the latter two after a linear warm-up of
    ``warmup_steps`` steps, reaching ``min_lr_ratio * lr`` at ``total_steps``)."""
    kind: str = "constant"
    warmup_steps: int = 0
    total_steps: int = 0
    min_lr_ratio: float = 0.0

    def __post_init__(self):
        if self.kind not in _KINDS:
            raise ValueError(f"schedule kind {self.kind!r}: expected one of {sorted(_KINDS)}")
        if self.warmup_steps < 0 or self.total_steps < 0:
            raise ValueError("warmup_steps and total_steps must be >= 0")


def _f32(v: float) -> float:
    return ctypes.c_float(v).value


def lr_at(schedule: Schedule | None, base_lr: float, t: int) -> float:
    """The rate of step ``t`` (1-based): gine_adamw_step_ctl's formula (include/gine_hip.h)
    restated in Python floats on the control block's fp32 fields, rounded to fp32 at the end."""
    lr = _f32(base_lr)
    if schedule is None or schedule.kind == "constant":
        return lr
    t = float(t)
    W, T, r = _f32(schedule.warmup_steps), _f32(schedule.total_steps), \
        _f32(schedule.min_lr_ratio)
    if t <= W:
        return _f32(lr * t / W)
    s = min(1.0, (t - W) / max(1.0, T - W))
    if schedule.kind == "cosine":
        return _f32(lr * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * s))))
    return _f32(lr * (r + (1.0 - r) * (1.0 - s)))


class ReduceOnPlateau:
    """Host-driven policy on top of :meth:`FlatAdamW.set_lr`: ``step(val_loss)`` once per
    epoch multiplies the rate by ``factor`` (not below ``min_lr``) after more than
    ``patience`` epochs without a new best validation loss."""

    def __init__(self, opt, factor: float = 0.1, patience: int = 10, min_lr: float = 0.0):
        if not 0.0 < factor < 1.0:
            raise ValueError("factor must be in (0, 1)")
        self.opt, self.factor, self.patience, self.min_lr = opt, factor, patience, min_lr
        self.best, self.bad_epochs = float("inf"), 0

    def step(self, val_loss: float) -> float:
        if val_loss < self.best:
            self.best, self.bad_epochs = float(val_loss), 0
        else:
            self.bad_epochs += 1
        if self.bad_epochs > self.patience:
            self.bad_epochs = 0
            new = max(self.opt.lr * self.factor, self.min_lr)
            if new < self.opt.lr:
                self.opt.set_lr(new)
        return self.opt.lr


class FlatAdamW:
    ALIGN = 64  # floats: parameter offsets in the flat buffers
    _CTL_WORDS, _REPORT_WORDS = 7, 4  # gine_adamw_ctl / gine_adamw_report, 4-byte fields

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *,
                 max_grad_norm=None, schedule=None, skip_nonfinite=None, device_control=False):
        self._ctl = None  # default mode until the buffers below exist
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        dev = self.params[0].device
        _lib.require_device(self.params[0], "FlatAdamW")
        if any(p.dtype != torch.float32 or p.device != dev for p in self.params):
            raise TypeError("FlatAdamW needs fp32 parameters on one device")
        self._lr, self.betas, self.eps, self.weight_decay = float(lr), betas, float(eps), \
            float(weight_decay)
        # every parameter starts on a 256-byte boundary (the kernels' weight fragment loads
        # use 16-byte vectors when a weight is aligned); the gaps stay zero in all four flat
        # buffers, which AdamW leaves at zero while eps > 0 (eps = 0 turns a gap's 0 / 0 into
        # NaN, as torch's AdamW does to a parameter with a zero gradient: DESIGN.md 6d)
        self._offsets = []
        off = 0
        for p in self.params:
            self._offsets.append(off)
            off = -(-(off + p.numel()) // self.ALIGN) * self.ALIGN
        n = off
        self.flat_param = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(self.params, self._offsets):
                k = p.numel()
                view = self.flat_param[off:off + k].view_as(p)
                view.copy_(p)
                p.data = view
                gradbuf.register(p, self.flat_grad, off)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        # [count, ticket, -, 8 sub-tickets at 32 + 32 g]: gine_adamw_step bumps the count in
        # its last workgroup (two-level ticket, include/gine_hip.h)
        floats = ctypes.c_int64(0)
        _lib.call("gine_adamw_state_floats", ctypes.byref(floats))
        control = (device_control or max_grad_norm is not None or schedule is not None
                   or skip_nonfinite is not None)
        # control mode: the report sits behind the step state, so stats() is one readback
        self._state_buf = torch.zeros(int(floats.value) + (self._REPORT_WORDS if control else 0),
                                      dtype=torch.float32, device=dev)
        self._step_state = self._state_buf[:int(floats.value)]
        self.step_count = self._step_state[:1]
        self.schedule = schedule
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(control if skip_nonfinite is None else skip_nonfinite)
        self._partials = None
        if control:
            self._init_control(dev)

    def _init_control(self, dev) -> None:
        cb, rb = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.call("gine_adamw_ctl_bytes", ctypes.byref(cb), ctypes.byref(rb))
        if (cb.value, rb.value) != (4 * self._CTL_WORDS, 4 * self._REPORT_WORDS):
            raise _lib.GineError("gine_adamw_ctl / gine_adamw_report layout mismatch")
        self._report = self._state_buf[self._step_state.numel():]
        # the norm launch is part of the step only when something reads it; a captured step
        # keeps whichever form it was built with
        if self.max_grad_norm is not None or self.skip_nonfinite:
            num = ctypes.c_int32(0)
            _lib.call("gine_grad_sumsq_num_partials", self.numel, ctypes.byref(num))
            self._partials = torch.zeros(int(num.value), 2, dtype=torch.float64, device=dev)
        # host mirror in pinned memory: set_lr & co. copy from it asynchronously
        self._ctl_host = torch.zeros(self._CTL_WORDS, dtype=torch.float32).pin_memory()
        self._ctl_copied = torch.cuda.Event()
        self._ctl = torch.zeros(self._CTL_WORDS, dtype=torch.float32, device=dev)
        self._upload_ctl(self._control_words())

    def _control_words(self) -> dict:
        sch = self.schedule or Schedule()
        return {"lr": self._lr, "max_norm": self.max_grad_norm or 0.0,
                "schedule": _KINDS[sch.kind], "warmup_steps": float(sch.warmup_steps),
                "total_steps": float(sch.total_steps), "min_lr_ratio": float(sch.min_lr_ratio),
                "skip_nonfinite": int(self.skip_nonfinite)}

    _CTL_FIELDS = [name for name, _ in _lib.AdamWCtl._fields_]

    def _upload_ctl(self, words: dict) -> None:
        """Write control fields: host mirror, then an asynchronous copy on the current
        stream (ordered before whatever is launched or replayed on it next)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the control block is written outside a capture (the copy "
                               "would be frozen into the graph)")
        self._ctl_copied.synchronize()  # the previous copy has read the pinned words
        ints = self._ctl_host.view(torch.int32)
        lo, hi = self._CTL_WORDS, 0
        for name, value in words.items():
            i = self._CTL_FIELDS.index(name)
            if name in ("schedule", "skip_nonfinite"):
                ints[i] = int(value)
            else:
                self._ctl_host[i] = float(value)
            lo, hi = min(lo, i), max(hi, i + 1)
        with torch.cuda.device(self._ctl.device):
            self._ctl[lo:hi].copy_(self._ctl_host[lo:hi], non_blocking=True)
            self._ctl_copied.record()

    @property
    def device_control(self) -> bool:
        return self._ctl is not None

    @property
    def lr(self) -> float:
        """The base learning rate (host mirror; the schedule scales it on the device)."""
        return self._lr

    @lr.setter
    def lr(self, value: float) -> None:
        self.set_lr(value)

    def set_lr(self, value: float) -> None:
        """Change the base rate.  Control mode: the next launch or replay on the current
        stream uses it.  Default mode: the rate is a launch argument, so a captured step is
        recaptured by :class:`raincast_gnn.train.StepRunner` when it sees the change."""
        self._lr = float(value)
        if self._ctl is not None:
            self._upload_ctl({"lr": self._lr})

    def set_max_grad_norm(self, value: float | None) -> None:
        """Change the clipping bound (None, <= 0 or inf: no clipping).  Control mode only,
        and only when the step computes the norm (built with ``max_grad_norm`` or
        ``skip_nonfinite``): a captured step cannot grow a launch."""
        if self._ctl is None or self._partials is None:
            raise RuntimeError("set_max_grad_norm needs a control-mode FlatAdamW whose step "
                               "computes the gradient norm (pass max_grad_norm=float('inf') "
                               "to start without clipping)")
        self.max_grad_norm = None if value is None else float(value)
        self._upload_ctl({"max_norm": self.max_grad_norm or 0.0})

    def hyper(self) -> tuple:
        """The host scalars that a default-mode launch (and so a capture of it) bakes in."""
        return (self._lr, tuple(self.betas), self.eps, self.weight_decay)

    @torch.no_grad()
    def stats(self) -> dict:
        """One readback: the last step's rate, gradient norm and clip coefficient, the number
        of skipped steps so far and the step count (``grad_norm`` / ``clip_coef`` are None
        where the step does not compute the norm)."""
        buf = self._state_buf.cpu()
        out = {"lr": self._lr, "grad_norm": None, "clip_coef": None, "skipped_steps": 0,
               "step": int(buf[0].item())}
        if self._ctl is not None:
            rep = buf[self._step_state.numel():]
            out["lr"] = rep[0].item()
            out["skipped_steps"] = int(rep.view(torch.int32)[3].item())
            if self._partials is not None:
                out["grad_norm"], out["clip_coef"] = rep[1].item(), rep[2].item()
        return out

    def state_dict(self) -> dict:
        """Moments, step count, control block, skipped counter, hyper-parameters and the
        layout of the flat buffers (host copies)."""
        buf = self._state_buf.cpu()
        ctl = None
        skipped = 0
        if self._ctl is not None:
            ctl = self._control_words()
            skipped = int(buf[self._step_state.numel():].view(torch.int32)[3].item())
        return {"exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(),
                "step": float(buf[0].item()), "control": ctl, "skipped": skipped,
                "hyper": {"lr": self._lr, "betas": tuple(self.betas), "eps": self.eps,
                          "weight_decay": self.weight_decay,
                          "max_grad_norm": self.max_grad_norm,
                          "schedule": None if self.schedule is None else asdict(self.schedule),
                          "skip_nonfinite": self.skip_nonfinite},
                "offsets": list(self._offsets), "numel": self.numel}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Copy a :meth:`state_dict` INTO the existing storage (captured graphs hold its
        pointers); the ticket words are left at 0.  Raises on another parameter layout.  A
        control-mode optimizer takes the saved control block when there is one (the norm
        launch stays as this optimizer was built); otherwise only the hyper-parameters."""
        if list(state["offsets"]) != list(self._offsets) or int(state["numel"]) != self.numel:
            raise ValueError("optimizer state of another parameter layout "
                             f"({state['numel']} values, {len(state['offsets'])} parameters; "
                             f"this optimizer: {self.numel}, {len(self._offsets)})")
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self._state_buf.zero_()
        self.step_count.fill_(float(state["step"]))
        h = state["hyper"]
        self._lr, self.betas, self.eps, self.weight_decay = float(h["lr"]), tuple(h["betas"]), \
            float(h["eps"]), float(h["weight_decay"])
        if self._ctl is not None:
            if state.get("control") is not None:
                self.schedule = None if h["schedule"] is None else Schedule(**h["schedule"])
                self.skip_nonfinite = bool(h["skip_nonfinite"]) and self._partials is not None
                self.max_grad_norm = h["max_grad_norm"] if self._partials is not None else None
                self._report.view(torch.int32)[3] = int(state["skipped"])
            self._upload_ctl(self._control_words())

    @property
    def numel(self) -> int:
        return self.flat_param.numel()

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Release the gradients.  The HIP backward kernels then write each parameter's
        gradient straight into its slice of ``flat_grad`` (raincast_gnn/gradbuf.py);
        ``set_to_none=False`` instead keeps ``.grad`` as slice views and zeroes them
        (gradients are then accumulated by autograd, one add per parameter)."""
        if set_to_none:
            for p in self.params:
                p.grad = None
            gradbuf.new_step(self.params)
        else:
            for p, off in zip(self.params, self._offsets):
                if p.grad is None or p.grad.data_ptr() != self.flat_grad[off:].data_ptr():
                    p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
            self.flat_grad.zero_()

    @torch.no_grad()
    def gather_grads(self) -> None:
        """Make ``flat_grad`` hold every gradient: parameters whose ``.grad`` is not their
        slice (a CPU-side or generic-torch backward produced it) are copied in, unused ones
        zeroed.  Host-side pointer checks only when everything already landed in place."""
        base = self.flat_grad.data_ptr()
        for p, off in zip(self.params, self._offsets):
            g = p.grad
            if g is not None and g.data_ptr() == base + 4 * off:
                continue
            sl = self.flat_grad[off:off + p.numel()]
            if g is None:
                sl.zero_()
            else:
                sl.copy_(g.reshape(-1))
            p.grad = sl.view_as(p)

    @torch.no_grad()
    def step(self) -> None:
        self.gather_grads()
        b1, b2 = self.betas
        stream = _lib.stream_handle(self.flat_param.device)
        if self._ctl is None:
            _lib.call("gine_adamw_step", _lib.ptr(self.flat_param), _lib.ptr(self.flat_grad),
                      _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                      _lib.ptr(self._step_state), self.numel, self._lr, float(b1), float(b2),
                      self.eps, self.weight_decay, stream)
            return
        num = 0
        if self._partials is not None:
            num = self._partials.size(0)
            _lib.call("gine_grad_sumsq", _lib.ptr(self.flat_grad), self.numel,
                      _lib.ptr(self._partials), num, stream)
        _lib.call("gine_adamw_step_ctl", _lib.ptr(self.flat_param), _lib.ptr(self.flat_grad),
                  _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(self._step_state),
                  self.numel, _lib.ptr(self._ctl), _lib.ptr(self._partials), num,
                  _lib.ptr(self._report), float(b1), float(b2), self.eps, self.weight_decay,
                  stream)

    def views_intact(self) -> bool:
        """True while every parameter and gradient still aliases the flat buffers."""
        pb, gb = self.flat_param.data_ptr(), self.flat_grad.data_ptr()
        end_p, end_g = pb + 4 * self.numel, gb + 4 * self.numel
        return all(pb <= p.data_ptr() < end_p and p.grad is not None
                   and gb <= p.grad.data_ptr() < end_g for p in self.params)
