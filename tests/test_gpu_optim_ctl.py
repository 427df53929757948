"""GPU: the device-controlled AdamW step: gine_grad_sumsq and
gine_adamw_step_ctl against gine_adamw_step bit for bit, the norm against fp64 on the host,
clipping against clip_grad_norm_ + torch.optim.AdamW, the schedule against optim.lr_at,
skipped steps, captured replays that follow set_lr, recapture in the default mode, resume and
fit.

The kernel-level tests call the C ABI on buffers of exactly n elements: FlatAdamW pads its
flat buffers to 64 floats, so only that way do n = 1, 7, 3075 reach the n % 4 tail.  Sizes:
tail only; one workgroup with a tail; several workgroups; ragged ticket groups (13
workgroups over 8 sub-tickets); and 600,000, past the capped 512 x 1,024-element grid (the
grid-stride loops take a second trip)."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import rel_err
from raincast_gnn import _lib
from raincast_gnn import train as T
from raincast_gnn.optim import FlatAdamW, ReduceOnPlateau, Schedule, lr_at

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 7, 3 * 1024 + 3, 13 * 1024 - 40, 600_000]
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.01


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def within_ulp(a, b, ulps=1):
    return abs(a - b) <= ulps * float(np.spacing(np.float32(abs(b))))


class Raw:
    """The four flat buffers of exactly n elements plus the step state, control block,
    report and partials, stepped through the C ABI."""

    def __init__(self, n, seed=0, partials=True):
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, generator=gen).to(DEV)
        self.g = torch.zeros(n, device=DEV)
        self.m = torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV)
        floats = ctypes.c_int64(0)
        _lib.call("gine_adamw_state_floats", ctypes.byref(floats))
        self.state = torch.zeros(floats.value, device=DEV)
        self.ctl = torch.zeros(7, device=DEV)
        self.report = torch.zeros(4, device=DEV)
        num = ctypes.c_int32(0)
        _lib.call("gine_grad_sumsq_num_partials", n, ctypes.byref(num))
        # NaN-filled: nothing has to be zeroed, every row is overwritten
        self.partials = (torch.full((num.value, 2), float("nan"), dtype=torch.float64,
                                    device=DEV) if partials else None)
        self.set_ctl(1e-3)

    def set_ctl(self, lr, max_norm=0.0, schedule=0, warmup=0.0, total=0.0, ratio=0.0, skip=1):
        c = _lib.AdamWCtl(lr, max_norm, schedule, warmup, total, ratio, skip)
        self.ctl.copy_(torch.frombuffer(bytearray(bytes(c)), dtype=torch.float32))

    def buffers(self):
        return _lib.ptr(self.p), _lib.ptr(self.g), _lib.ptr(self.m), _lib.ptr(self.v), \
            _lib.ptr(self.state), self.n

    def step_default(self, lr):
        _lib.call("gine_adamw_step", *self.buffers(), lr, B1, B2, EPS, WD,
                  _lib.stream_handle(DEV))

    def sumsq(self):
        _lib.call("gine_grad_sumsq", _lib.ptr(self.g), self.n, _lib.ptr(self.partials),
                  self.partials.size(0), _lib.stream_handle(DEV))

    def step_ctl(self):
        num = 0
        if self.partials is not None:
            num = self.partials.size(0)
            self.sumsq()
        _lib.call("gine_adamw_step_ctl", *self.buffers(), _lib.ptr(self.ctl),
                  _lib.ptr(self.partials), num, _lib.ptr(self.report), B1, B2, EPS, WD,
                  _lib.stream_handle(DEV))

    def rep(self):
        r = self.report.cpu()
        return {"lr": r[0].item(), "norm": r[1].item(), "coef": r[2].item(),
                "skipped": int(r.view(torch.int32)[3].item()), "step": self.state[0].item()}

    def tickets_zero(self):
        return int(bits(self.state)[1:].abs().sum()) == 0

    def same_state(self, other):
        return (same_bits(self.p, other.p) and same_bits(self.m, other.m)
                and same_bits(self.v, other.v) and same_bits(self.state[:1], other.state[:1]))


def host_norm(g):
    return float(np.float32(math.sqrt(g.double().cpu().square().sum().item())))


# -- 1. neutral control mode == the existing kernel -------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_neutral_control_block_equals_adamw_step(n):
    """No clipping, constant schedule: param, both moments and the step count carry the bits
    of gine_adamw_step, with the norm launch and without it; the tickets are re-armed."""
    ref, a, b = Raw(n), Raw(n), Raw(n, partials=False)
    gen = torch.Generator().manual_seed(n)
    for _ in range(5):
        g = torch.randn(n, generator=gen).to(DEV)
        for r in (ref, a, b):
            r.g.copy_(g)
        ref.step_default(1e-3)
        a.step_ctl()
        b.step_ctl()
    torch.cuda.synchronize()
    assert ref.state[0].item() == 5
    for r in (a, b):
        assert r.same_state(ref)
        assert r.tickets_zero()
        assert r.rep()["coef"] == 1.0 and r.rep()["lr"] == float(np.float32(1e-3))
        assert r.rep()["skipped"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_flat_adamw_neutral_control_mode_equals_default_mode(n):
    torch.manual_seed(2)
    p = torch.nn.Parameter(torch.randn(n, device=DEV))
    q = torch.nn.Parameter(p.detach().clone())
    ctl = FlatAdamW([p], lr=1e-3, weight_decay=0.01, device_control=True)
    ref = FlatAdamW([q], lr=1e-3, weight_decay=0.01)
    assert ctl.device_control and not ref.device_control and ctl.skip_nonfinite
    assert ref._partials is None and ref._state_buf.numel() == ref._step_state.numel()
    for _ in range(5):
        g = torch.randn(n, device=DEV)
        for opt, w in ((ctl, p), (ref, q)):
            opt.zero_grad(set_to_none=False)
            w.grad.copy_(g)
            opt.step()
    for x, y in ((ctl.flat_param, ref.flat_param), (ctl.exp_avg, ref.exp_avg),
                 (ctl.exp_avg_sq, ref.exp_avg_sq), (ctl.step_count, ref.step_count)):
        assert same_bits(x, y)
    assert int(bits(ctl._step_state)[1:].abs().sum()) == 0
    st = ctl.stats()
    assert st["step"] == 5 and st["skipped_steps"] == 0 and st["clip_coef"] == 1.0


# -- 2. the norm ------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_is_the_fp64_norm_and_reproducible(n):
    """The fp64 sum of at most 10^6 squares is exact far below fp32 resolution: only the
    final rounding can differ from the host's, so 1 fp32 ulp; same input, same bits."""
    r = Raw(n)
    gen = torch.Generator().manual_seed(10 + n)
    r.g.copy_(torch.randn(n, generator=gen) * 3.0)
    r.step_ctl()
    first_partials, first = r.partials.clone(), r.rep()["norm"]
    want = host_norm(r.g)
    print(f"n={n}: norm {first!r} host {want!r}")
    assert within_ulp(first, want)
    assert float(r.partials[:, 1].sum().item()) == 0.0
    r.partials.fill_(float("nan"))
    r.step_ctl()
    assert torch.equal(bits(r.partials), bits(first_partials))
    assert np.float32(r.rep()["norm"]).tobytes() == np.float32(first).tobytes()
    # through FlatAdamW
    w = torch.nn.Parameter(torch.zeros(n, device=DEV))
    opt = FlatAdamW([w], lr=1e-3, device_control=True)
    opt.zero_grad(set_to_none=False)
    w.grad.copy_(r.g)
    opt.step()
    assert within_ulp(opt.stats()["grad_norm"], want)


# -- 3. clipping ------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_clipped_step_is_a_default_step_on_the_scaled_gradient(n):
    gen = torch.Generator().manual_seed(20 + n)
    grads = [torch.randn(n, generator=gen).to(DEV) for _ in range(3)]
    bound = 0.5 * min(host_norm(g) for g in grads)  # every step is clipped
    a, twin = Raw(n), Raw(n)
    a.set_ctl(2e-3, max_norm=bound)
    for g in grads:
        a.g.copy_(g)
        a.step_ctl()
        rep = a.rep()
        assert 0.0 < rep["coef"] < 1.0
        want = np.float32(bound) / (np.float32(host_norm(g)) + np.float32(1e-6))
        # the norm's 1 ulp (relative 2^-23 at worst) plus the divide's half ulp, on a quotient
        # whose own ulp can be 2^-24 relative: at most 3 ulps, 4 allowed
        assert within_ulp(rep["coef"], float(want), ulps=4)
        twin.g.copy_(g * torch.tensor(rep["coef"], dtype=torch.float32, device=DEV))
        twin.step_default(rep["lr"])
        assert a.same_state(twin)
    # a bound above the norm: the coefficient is exactly 1 and the bits are test 1's
    b, ref = Raw(n), Raw(n)
    b.set_ctl(2e-3, max_norm=4.0 * max(host_norm(g) for g in grads))
    for g in grads:
        b.g.copy_(g)
        ref.g.copy_(g)
        b.step_ctl()
        ref.step_default(2e-3)
        assert b.rep()["coef"] == 1.0
    assert b.same_state(ref) and b.tickets_zero() and a.tickets_zero()


@pytest.mark.parametrize("n", [13 * 1024 - 40, 600_000])
def test_clipping_matches_clip_grad_norm_and_torch_adamw(n):
    """The project's bar for FlatAdamW against torch (tests/test_gpu_training.py)."""
    torch.manual_seed(3)
    p = torch.nn.Parameter(torch.randn(n, device=DEV))
    q = torch.nn.Parameter(p.detach().clone())
    bound = 0.5 * math.sqrt(n)  # randn: norm ~ sqrt(n), so every step is clipped
    opt = FlatAdamW([p], lr=3e-3, weight_decay=0.01, max_grad_norm=bound)
    opt_ref = torch.optim.AdamW([q], lr=3e-3, weight_decay=0.01, foreach=False)
    for _ in range(6):
        g = torch.randn(n, device=DEV)
        opt.zero_grad(set_to_none=False)
        p.grad.copy_(g)
        q.grad = g.clone()
        opt.step()
        torch.nn.utils.clip_grad_norm_([q], bound)
        opt_ref.step()
        assert opt.stats()["clip_coef"] < 1.0
    err = rel_err(p.detach(), q.detach())
    print(f"n={n}: rel_err vs clip_grad_norm_ + torch AdamW {err:.3e}")
    assert err <= 2e-6
    assert opt.stats()["step"] == 6


# -- 4. the schedule --------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 13 * 1024 - 40])
@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_schedule_follows_lr_at_and_steps_like_the_default_mode(n, kind):
    torch.manual_seed(4)
    sch = Schedule(kind, warmup_steps=3, total_steps=8, min_lr_ratio=0.1)
    p = torch.nn.Parameter(torch.randn(n, device=DEV))
    q = torch.nn.Parameter(p.detach().clone())
    opt = FlatAdamW([p], lr=3e-3, weight_decay=0.01, schedule=sch)
    twin = FlatAdamW([q], lr=3e-3, weight_decay=0.01)
    for t in range(1, 11):
        g = torch.randn(n, device=DEV)
        opt.zero_grad(set_to_none=False)
        p.grad.copy_(g)
        opt.step()
        lr = opt.stats()["lr"]
        want = lr_at(sch, 3e-3, t)
        print(f"{kind} t={t}: lr {lr!r} lr_at {want!r}")
        assert within_ulp(lr, want)
        twin.lr = lr
        twin.zero_grad(set_to_none=False)
        q.grad.copy_(g)
        twin.step()
        assert same_bits(opt.flat_param, twin.flat_param)
        assert same_bits(opt.exp_avg_sq, twin.exp_avg_sq)
    assert opt.stats()["step"] == 10 and opt.lr == 3e-3


# -- 5. skipping ------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_nonfinite_gradient_is_skipped_and_counted(n, value):
    """One inf / NaN at element 0, at the last element (the n % 4 tail where there is one)
    and in a far workgroup (n = 600,000: float4 75,000, workgroup 292)."""
    r = Raw(n)
    r.set_ctl(1e-3, max_norm=1.0)
    gen = torch.Generator().manual_seed(30 + n)
    r.g.copy_(torch.randn(n, generator=gen))
    r.step_ctl()                                     # a finite step first: non-zero moments
    assert r.rep()["step"] == 1 and r.rep()["skipped"] == 0
    skipped = 0
    for pos in sorted({0, n - 1, n // 2}):
        before = [t.clone() for t in (r.p, r.m, r.v, r.state)]
        g = torch.randn(n, generator=gen)
        g[pos] = value
        r.g.copy_(g)
        r.step_ctl()
        skipped += 1
        for was, now in zip(before, (r.p, r.m, r.v, r.state)):
            assert same_bits(was, now), pos
        rep = r.rep()
        assert rep["skipped"] == skipped and rep["step"] == 1 and r.tickets_zero()
        assert float(r.partials[:, 1].sum().item()) == 1.0
    r.g.copy_(torch.randn(n, generator=gen))
    before_p = r.p.clone()
    r.step_ctl()
    assert r.rep()["step"] == 2 and r.rep()["skipped"] == skipped
    assert not same_bits(before_p, r.p) and bool(torch.isfinite(r.p).all())
    # skip_nonfinite off: the update goes through and the parameters are lost, as documented
    r.set_ctl(1e-3, max_norm=1.0, skip=0)
    g = torch.randn(n, generator=gen)
    g[n - 1] = value
    r.g.copy_(g)
    r.step_ctl()
    assert r.rep()["step"] == 3 and r.rep()["skipped"] == skipped
    assert not bool(torch.isfinite(r.p).all())


def test_flat_adamw_counts_skipped_steps_and_host_policies_reach_the_device():
    torch.manual_seed(5)
    n = 5000
    p = torch.nn.Parameter(torch.randn(n, device=DEV))
    opt = FlatAdamW([p], lr=1e-3, max_grad_norm=float("inf"))

    def step(g):
        opt.zero_grad(set_to_none=False)
        p.grad.copy_(g)
        opt.step()
        return opt.stats()

    g = torch.randn(n, device=DEV)
    assert step(g)["clip_coef"] == 1.0               # inf: no clipping
    opt.set_max_grad_norm(0.5 * host_norm(g))
    assert abs(step(g)["clip_coef"] - 0.5) < 1e-6
    bad = g.clone()
    bad[17] = float("nan")
    keep = opt.flat_param.clone()
    st = step(bad)
    assert st["skipped_steps"] == 1 and st["step"] == 2 and same_bits(keep, opt.flat_param)
    plateau = ReduceOnPlateau(opt, factor=0.5, patience=0, min_lr=4e-4)
    assert plateau.step(1.0) == 1e-3 and plateau.step(2.0) == 5e-4
    assert opt.lr == 5e-4 and step(g)["lr"] == float(np.float32(5e-4))
    assert plateau.step(3.0) == 4e-4                 # the floor
    assert step(g)["lr"] == float(np.float32(4e-4))
    with pytest.raises(RuntimeError):
        FlatAdamW([torch.nn.Parameter(torch.zeros(8, device=DEV))]).set_max_grad_norm(1.0)


# -- 6-8. the captured step ---------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """The model and batch of tests/test_gpu_parity.py::test_graph_capture_replay_matches_eager
    and that batch's gradient norm at the initial weights (read once from the device)."""
    from raincast_gnn.data import synthetic_batch
    from raincast_gnn.models import GNN
    torch.manual_seed(0)
    base = GNN(35, 128, 128, 4, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)
    batch = synthetic_batch(500, 4, k=10, seed=1).to(DEV)
    m = copy.deepcopy(base).to(DEV).train()
    opt = FlatAdamW(m.parameters(), lr=0.0, weight_decay=0.0, device_control=True)
    T.StepRunner(m, opt, graphed=False)(batch)
    norm = opt.stats()["grad_norm"]
    assert math.isfinite(norm) and norm > 0.0
    return base, batch, norm


def _control(base, norm, **kw):
    m = copy.deepcopy(base).to(DEV).train()
    kw.setdefault("weight_decay", 0.0)
    opt = FlatAdamW(m.parameters(), lr=1e-3, max_grad_norm=0.5 * norm,
                    schedule=Schedule("cosine", 2, 20, 0.1), **kw)
    return m, opt


def _poisoned(batch):
    """The same batch with one non-finite input row: every gradient of the step is NaN."""
    from raincast_gnn.data import GraphBatch
    x = batch.x.clone()
    x[0] = float("inf")
    return GraphBatch(x, batch.ensemble, batch.edge_index, batch.edge_attr, batch.y,
                      batch.batch, batch.ptr, batch.num_graphs)


def test_captured_replay_follows_the_control_block(small):
    base, batch, norm = small
    m_e, o_e = _control(base, norm)
    eager = T.StepRunner(m_e, o_e, graphed=False)
    want, coefs = [], []
    for _ in range(6):
        want.append(eager(batch).item())
        coefs.append(o_e.stats()["clip_coef"])
    assert coefs[0] < 1.0                                   # the bound is half the first norm
    m_g, o_g = _control(base, norm)
    runner = T.StepRunner(m_g, o_g, graphed=True)
    got = [runner(batch).item() for _ in range(6)]          # 2 eager steps, 4 replays
    assert len(runner._graphs) == 1
    assert got == want
    assert same_bits(o_g.flat_param, o_e.flat_param) and same_bits(o_g.exp_avg, o_e.exp_avg)
    st = o_g.stats()
    assert st["step"] == 6 and st["clip_coef"] == coefs[-1] and st["skipped_steps"] == 0
    assert within_ulp(st["lr"], lr_at(o_g.schedule, 1e-3, 6))
    graph = runner._graphs[batch.num_graphs][0]
    # lr 0 (weight decay 0): the replay changes no parameter but counts the step
    keep = o_g.flat_param.clone()
    o_g.set_lr(0.0)
    runner(batch)
    assert same_bits(keep, o_g.flat_param) and o_g.stats()["step"] == 7
    o_g.set_lr(1e-3)
    runner(batch)
    assert not same_bits(keep, o_g.flat_param) and o_g.stats()["step"] == 8
    assert within_ulp(o_g.stats()["lr"], lr_at(o_g.schedule, 1e-3, 8))
    # a non-finite gradient inside a replay: skipped and counted
    keep = o_g.flat_param.clone()
    runner(_poisoned(batch))
    st = o_g.stats()
    assert st["skipped_steps"] == 1 and st["step"] == 8 and same_bits(keep, o_g.flat_param)
    runner(batch)
    st = o_g.stats()
    assert st["skipped_steps"] == 1 and st["step"] == 9
    assert not same_bits(keep, o_g.flat_param) and bool(torch.isfinite(o_g.flat_param).all())
    assert runner._graphs[batch.num_graphs][0] is graph      # nothing was recaptured


def test_default_mode_recaptures_when_the_rate_changes(small):
    base, batch, _ = small

    def make():
        m = copy.deepcopy(base).to(DEV).train()
        return m, FlatAdamW(m.parameters(), lr=1e-3)

    m_e, o_e = make()
    eager = T.StepRunner(m_e, o_e, graphed=False)
    m_g, o_g = make()
    runner = T.StepRunner(m_g, o_g, graphed=True)
    for _ in range(4):
        eager(batch)
        runner(batch)
    first = runner._graphs[batch.num_graphs][0]
    assert same_bits(o_g.flat_param, o_e.flat_param)
    o_e.lr = o_g.lr = 2.5e-4
    for _ in range(4):                                       # warm-up again, then replays
        eager(batch)
        runner(batch)
    assert same_bits(o_g.flat_param, o_e.flat_param)
    assert runner._graphs[batch.num_graphs][0] is not first
    assert runner._graphs[batch.num_graphs][4] == o_g.hyper()


@pytest.mark.parametrize("control", [False, True])
def test_resume_continues_bit_for_bit(small, control):
    base, batch, norm = small

    def make(seed=None):
        if seed is None:
            src = base
        else:
            from raincast_gnn.models import GNN
            torch.manual_seed(seed)
            src = GNN(35, 128, 128, 4, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5)
        if control:
            return _control(src, norm, weight_decay=0.01)
        m = copy.deepcopy(src).to(DEV).train()
        return m, FlatAdamW(m.parameters(), lr=1e-3)

    m_a, o_a = make()
    run_a = T.StepRunner(m_a, o_a, graphed=False)
    saved = None
    for i in range(5):
        run_a(batch)
        if i == 2:
            saved = ({k: v.detach().cpu().clone() for k, v in m_a.state_dict().items()},
                     copy.deepcopy(o_a.state_dict()))
    # a fresh model and optimizer
    m_b, o_b = make(seed=77)
    m_b.load_state_dict(saved[0])
    o_b.load_state_dict(saved[1])
    run_b = T.StepRunner(m_b, o_b, graphed=False)
    for _ in range(2):
        run_b(batch)
    assert same_bits(o_b.flat_param, o_a.flat_param)
    assert same_bits(o_b.exp_avg, o_a.exp_avg) and same_bits(o_b.exp_avg_sq, o_a.exp_avg_sq)
    assert o_b.stats()["step"] == 5
    # an optimizer whose step is already captured: the storage pointers do not move
    m_c, o_c = make(seed=78)
    run_c = T.StepRunner(m_c, o_c, graphed=True)
    for _ in range(4):
        run_c(batch)
    ptrs = (o_c.flat_param.data_ptr(), o_c.exp_avg.data_ptr(), o_c._step_state.data_ptr())
    graph = run_c._graphs[batch.num_graphs][0]
    m_c.load_state_dict(saved[0])
    o_c.load_state_dict(saved[1])
    assert ptrs == (o_c.flat_param.data_ptr(), o_c.exp_avg.data_ptr(),
                    o_c._step_state.data_ptr())
    assert int(bits(o_c._step_state)[1:].abs().sum()) == 0
    for _ in range(2):
        run_c(batch)
    assert run_c._graphs[batch.num_graphs][0] is graph
    assert same_bits(o_c.flat_param, o_a.flat_param) and o_c.stats()["step"] == 5
    # another layout is refused
    other = FlatAdamW([torch.nn.Parameter(torch.zeros(100, device=DEV))], lr=1e-3)
    with pytest.raises(ValueError, match="layout"):
        other.load_state_dict(saved[1])


# -- 9. fit -----------------------------------------------------------------------------
def test_fit_takes_clipping_and_schedule_from_params(tmp_path):
    import os
    from raincast_gnn.batching import DeviceDataset, DeviceLoader
    from raincast_gnn.data import synthetic_samples
    from raincast_gnn.models import gnn_from_params
    from raincast_gnn.params import EXPERIMENTS
    params = dict(EXPERIMENTS["24h_mixed"], max_grad_norm=1.0,
                  lr_schedule={"kind": "cosine", "warmup_steps": 2, "min_lr_ratio": 0.1})
    full = DeviceDataset(synthetic_samples(122, 14, k=10, seed=5), DEV)
    tr, va = T.split_train_val(full, generator=torch.Generator().manual_seed(0))
    loader = DeviceLoader(tr, 4, seed=3)
    torch.manual_seed(42)
    model = gnn_from_params(params).to(DEV)
    steps = len(loader)
    opt = T.make_optimizer(model.parameters(), params, total_steps=2 * steps)
    assert opt.device_control and opt.max_grad_norm == 1.0
    assert opt.schedule == Schedule("cosine", 2, 2 * steps, 0.1)
    out = T.fit(model, opt, loader, DeviceLoader(va, 4, shuffle=False), DEV, 2,
                ckpt_dir=str(tmp_path), run_id="c", example=tr.batch(torch.tensor([0])))
    h = out["history"]
    assert all(math.isfinite(v) for v in h["train"] + h["val"] + h["grad_norm"])
    assert h["skipped"] == [0, 0]
    for e in range(2):
        assert within_ulp(h["lr"][e], lr_at(opt.schedule, params["lr"], (e + 1) * steps))
    assert opt.stats()["step"] == 2 * steps
    state = torch.load(T.opt_state_path(out["best_ckpt_path"]), weights_only=True)
    assert os.path.exists(out["best_ckpt_path"]) and state["numel"] == opt.numel
    assert state["control"]["max_norm"] == 1.0 and state["hyper"]["schedule"]["kind"] == "cosine"
    # the reference's params.json: the plain optimizer, nothing new in its step
    plain = T.make_optimizer(gnn_from_params(EXPERIMENTS["24h_mixed"]).to(DEV).parameters(),
                             EXPERIMENTS["24h_mixed"])
    assert not plain.device_control and plain._partials is None
