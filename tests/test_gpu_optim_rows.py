"""GPU: the kernels of csrc/gine_optim.hip held per element to tests/optim_oracle.py at the
cases of tests/optim_cases.py.

gine_adamw_step and gine_adamw_step_ctl: param, exp_avg and exp_avg_sq bit for bit against
oracle A (the fp32 restatement) at every size, element state, step count and hyper-parameter
set, the step count and the ticket words beside them; gine_grad_sumsq: every partial bit for
bit against the fp64 restatement of the documented order; the clip coefficient and the
scheduled rate bit for bit against their exact formulas; FlatAdamW end to end per parameter
slice; and the 20-step trajectory against torch.optim.AdamW on the CPU at the analytic bound.
A NaN on both sides is agreement.  The buffers hold exactly n elements (Raw)."""
import numpy as np
import pytest
import torch

import optim_cases as C
import optim_oracle as O
from helpers import rel_err
from raincast_gnn import _lib
from raincast_gnn.optim import FlatAdamW, Schedule
from test_gpu_optim_ctl import DEV, Raw, bits

pytestmark = pytest.mark.gpu
F32 = np.float32


class Dev(Raw):
    """Raw with the hyper-parameters of a combo, loaded from numpy arrays."""

    def __init__(self, n, combo, partials=False):
        super().__init__(n, partials=partials)
        self.combo = combo

    def load(self, d, preset=0):
        for dst, key in ((self.p, "p"), (self.g, "g"), (self.m, "m"), (self.v, "v")):
            dst.copy_(torch.from_numpy(np.array(d[key])))
        self.state.zero_()
        self.state[0] = float(preset)
        self.report.zero_()
        return self

    def step_default(self, lr=None):
        _, lr0, b1, b2, eps, wd = self.combo
        _lib.call("gine_adamw_step", *self.buffers(), float(lr0 if lr is None else lr), b1, b2,
                  eps, wd, _lib.stream_handle(DEV))

    def step_ctl(self):
        _, _, b1, b2, eps, wd = self.combo
        num = 0
        if self.partials is not None:
            num = self.partials.size(0)
            self.sumsq()
        _lib.call("gine_adamw_step_ctl", *self.buffers(), _lib.ptr(self.ctl),
                  _lib.ptr(self.partials), num, _lib.ptr(self.report), b1, b2, eps, wd,
                  _lib.stream_handle(DEV))

    def read(self):
        return tuple(t.cpu().numpy() for t in (self.p, self.m, self.v))

    def report_f32(self):
        r = self.report.cpu().numpy()
        return {"lr": r[0], "norm": r[1], "coef": r[2], "skipped": int(r.view(np.uint32)[3])}

    def check(self, want, count, d, where):
        got = self.read()
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
            C.assert_bits(f"{where} {name}", a, b, d)
        assert self.state[0].item() == count, where
        assert self.tickets_zero(), where


# -- 1. the update, every case -------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
def test_adamw_step_is_oracle_a_bit_for_bit(n):
    """Both kernels (gine_adamw_step; gine_adamw_step_ctl under a neutral control block), two
    steps from every preset step count: param, exp_avg, exp_avg_sq, the count (which stays at
    2^24 once it is there, the update still applied) and the re-armed tickets."""
    for k, (combo, preset) in enumerate(C.pairs(n)):
        # a seed per pair: the rotation walks even n = 1 through 40 states of the grid
        d = C.data(n, k if n < 512 * 1024 else k % 2)
        want, counts = C.run_a(d, combo, preset)
        for kernel in ("default", "ctl"):
            r = Dev(n, combo).load(d, preset)
            r.set_ctl(combo[1])
            for s in range(2):
                r.step_default() if kernel == "default" else r.step_ctl()
                r.check(want[s], counts[s], d, f"n={n} {combo[0]} step[0]={preset} {kernel} "
                                              f"step {s + 1}:")
            if kernel == "ctl":
                rep = r.report_f32()
                assert rep["lr"] == F32(combo[1]) and rep["coef"] == 1 and rep["skipped"] == 0


def test_the_step_count_stops_at_two_to_the_24():
    r = Dev(5, C.MAIN).load(C.data(5, 0), 2 ** 24)
    before = r.read()
    r.step_default()
    assert r.state[0].item() == 2 ** 24 and r.tickets_zero()
    assert C.mismatches(r.read()[0], before[0]).size > 0          # the update is applied


def test_eps_zero_gives_nan_where_torch_does_and_in_the_alignment_gaps():
    combo = ("eps0", 1e-3, 0.9, 0.999, 0.0, 0.01)
    n = 8 * 1024
    d = C.data(n, 0)
    want, counts = C.run_a(d, combo, 0, steps=1)
    zero = (d["v"] == 0) & (d["g"] == 0) & (d["m"] == 0)
    assert zero.sum() >= 10 and np.isnan(want[0][0][zero]).all()
    r = Dev(n, combo).load(d)
    r.step_default()
    r.check(want[0], counts[0], d, "eps = 0:")
    # FlatAdamW: the gap behind a 63-element parameter is 0 / 0 as well
    w = torch.nn.Parameter(torch.ones(63, device=DEV))
    opt = FlatAdamW([w], lr=1e-3, eps=0.0)
    opt.zero_grad(set_to_none=False)
    w.grad.fill_(1.0)
    opt.step()
    assert bool(torch.isnan(opt.flat_param[63:]).all())
    assert bool(torch.isfinite(opt.flat_param[:63]).all())


# -- 2. the trajectory and the tie to torch ------------------------------------------------
@pytest.fixture(scope="module")
def device_trajectory():
    tr = C.trajectory()
    r = Dev(C.TRAJ_N, C.MAIN)
    r.load({"p": tr["p0"], "g": tr["grads"][0], "m": np.zeros(C.TRAJ_N, np.float32),
            "v": np.zeros(C.TRAJ_N, np.float32)})
    out = []
    for k in range(C.TRAJ_STEPS):
        r.g.copy_(torch.from_numpy(tr["grads"][k].copy()))
        r.step_default()
        out.append(r.read())
    assert r.state[0].item() == C.TRAJ_STEPS and r.tickets_zero()
    return out


def test_trajectory_is_oracle_a_at_every_step(device_trajectory):
    want = C.trajectory_a()
    for k in range(C.TRAJ_STEPS):
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), device_trajectory[k], want[k]):
            C.assert_bits(f"trajectory step {k + 1} {name}", a, b)


def test_trajectory_is_tied_to_torch_adamw_at_the_analytic_bound(device_trajectory):
    """MI355X: v rel 1.3317e-05 (bound 1.7929e-05), m error / bound 0.278, p rel_err 6.5e-08."""
    p, m, v = device_trajectory[-1]
    pt, mt, vt = C.torch_trajectory()
    b = C.tie_bounds()
    rel_v = np.abs(v.astype(np.float64) - vt) / vt
    err_m = np.abs(m.astype(np.float64) - mt)
    err_p = rel_err(torch.from_numpy(p), torch.from_numpy(pt))
    print(f"tie to torch after {C.TRAJ_STEPS} steps: v rel {rel_v.max():.4e} (bound "
          f"{b['v_rel']:.4e}, analytic part {b['dep_v']:.4e}), m error / bound "
          f"{float((err_m / b['m_abs']).max()):.3f}, p rel_err {err_p:.3e}")
    assert (rel_v <= b["v_rel"]).all()
    assert (err_m <= b["m_abs"]).all()
    assert err_p <= 2e-6


# -- 3. the norm ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
def test_grad_sumsq_partials_are_the_documented_order_bit_for_bit(n):
    g = C.wide_grad(n)
    r = Dev(n, C.MAIN, partials=True)
    r.g.copy_(torch.from_numpy(g.copy()))
    r.set_ctl(1e-3)
    r.step_ctl()
    got = r.partials.cpu().numpy()
    want = O.sumsq_partials(g)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        np.nonzero(got.view(np.uint64) != want.view(np.uint64))
    rep = r.report_f32()
    norm = O.norm_f32(want)
    assert rep["norm"].tobytes() == norm.tobytes() and rep["coef"] == 1 and rep["skipped"] == 0
    exact = O.norm_exact(g)
    assert abs(O.mpf(float(rep["norm"])) - exact) <= float(np.spacing(norm))
    # non-finite values: counted in the workgroup that reads them, the sums NaN / inf alike
    bad = C.unit_grad(n).copy()
    spots = sorted({0, n - 1, min(C.last_workgroup_start(n), n - 1), n // 2})
    for k, i in enumerate(spots):
        bad[i] = (np.inf, np.nan, -np.inf)[k % 3]
    r.g.copy_(torch.from_numpy(bad))
    r.partials.fill_(-1.0)
    r.sumsq()
    got = r.partials.cpu().numpy()
    want = O.sumsq_partials(bad)
    assert np.array_equal(got[:, 1], want[:, 1]) and got[:, 1].sum() == len(spots)
    same = (got[:, 0].view(np.uint64) == want[:, 0].view(np.uint64)) | \
        (np.isnan(got[:, 0]) & np.isnan(want[:, 0]))
    assert same.all()


# -- 4. the clip coefficient ---------------------------------------------------------------
def _clipped(n, g, max_norm, skip, seed):
    d = dict(C.data(n, seed), g=g)
    r = Dev(n, C.MAIN, partials=True).load(d)
    r.set_ctl(C.MAIN[1], max_norm=max_norm, skip=skip)
    r.step_ctl()
    return r, d


@pytest.mark.parametrize("n", [5, 9 * 1024 + 1, 600_000])
def test_clip_coefficient_and_the_clipped_step(n):
    unit = C.unit_grad(n)
    norm = O.norm_f32(O.sumsq_partials(unit))
    cases = [("zero", np.zeros(n, np.float32), 1.0), ("norm == max_norm", unit, float(norm)),
             ("max_norm 1e-30", unit, 1e-30), ("above the norm", unit, 4.0)]
    for k, (name, g, max_norm) in enumerate(cases):
        r, d = _clipped(n, g, max_norm, 1, k % 2)
        want_norm = O.norm_f32(O.sumsq_partials(g))
        coef = O.clip_coef(max_norm, want_norm)
        rep = r.report_f32()
        print(f"n={n} {name}: norm {float(rep['norm'])!r} coef {float(rep['coef'])!r}")
        assert rep["norm"].tobytes() == want_norm.tobytes(), name
        assert rep["coef"].tobytes() == coef.tobytes(), name
        assert rep["skipped"] == 0 and rep["lr"] == F32(C.MAIN[1])
        if name in ("zero", "above the norm"):
            assert coef == 1
        elif name == "norm == max_norm":
            assert F32(max_norm) == want_norm and 0.99 < coef < 1
        else:
            assert 0 < coef < 2e-30
        want, counts = C.run_a(d, C.MAIN, 0, steps=1, coef=coef)
        r.check(want[0], counts[0], d, f"n={n} {name}:")
    # finite gradients whose norm overflows fp32
    big = unit.copy()
    big[sorted({0, n // 2, n - 1})] = 3e38
    r, d = _clipped(n, big, 1.0, 1, 0)
    rep = r.report_f32()
    assert np.isinf(rep["norm"]) and rep["skipped"] == 1 and r.state[0].item() == 0
    assert float(r.partials[:, 1].sum().item()) == 0.0           # no value is non-finite
    for name, a, key in zip(("param", "exp_avg", "exp_avg_sq"), r.read(), "pmv"):
        C.assert_bits(f"skipped step {name}", a, d[key])
    assert r.tickets_zero()
    r, d = _clipped(n, big, 1.0, 0, 0)
    rep = r.report_f32()
    assert np.isinf(rep["norm"]) and rep["coef"] == 0 and rep["skipped"] == 0
    assert not np.signbit(rep["coef"])
    want, counts = C.run_a(d, C.MAIN, 0, steps=1, coef=F32(0))    # a zero gradient, signs kept
    r.check(want[0], counts[0], d, f"n={n} overflowing norm, no skip:")


# -- 5. the schedule -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", [O.COSINE, O.LINEAR])
def test_scheduled_rate_is_the_exact_formula_rounded_once(kind):
    n = 1025
    d = C.data(n, 1)
    for kd, wtr, t in C.schedule_cases():
        if kd != kind:
            continue
        lr_t, _ = C.lr_t(kind, wtr, t)
        r = Dev(n, C.MAIN).load(d, t - 1)
        r.set_ctl(C.SCHED_LR, schedule=kind, warmup=float(wtr[0]), total=float(wtr[1]),
                  ratio=wtr[2])
        r.step_ctl()
        rep = r.report_f32()
        assert rep["lr"].tobytes() == lr_t.tobytes(), (wtr, t, float(rep["lr"]), float(lr_t))
        want, counts = C.run_a(d, C.MAIN, t - 1, steps=1, lr=lr_t)
        r.check(want[0], counts[0], d, f"schedule {kind} {wtr} t={t}:")
    for (W, T, ratio), t in C.S_HALF:                              # s = 0.5 exactly
        lr32, r32 = O.frac(F32(C.SCHED_LR)), O.frac(F32(ratio))
        assert C.lr_t(kind, (W, T, ratio), t)[0] == O.fl32(lr32 * (r32 + (1 - r32) / 2))[0]


# -- 6. FlatAdamW end to end ---------------------------------------------------------------
@pytest.mark.parametrize("control", [False, True])
def test_flat_adamw_slices_are_oracle_a_and_the_gaps_stay_zero(control):
    case = C.flat_case()
    offs, total = C.flat_layout()
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in case["p0"]]
    kw = {}
    if control:
        name, W, T, ratio = C.FLAT_SCHEDULE
        kw = {"max_grad_norm": C.FLAT_MAX_NORM, "schedule": Schedule(name, W, T, ratio)}
    _, lr, b1, b2, eps, wd = C.MAIN
    opt = FlatAdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, **kw)
    assert opt.numel == total and list(opt._offsets) == offs
    gap = np.ones(total, dtype=bool)
    for off, k in zip(offs, C.FLAT_SIZES):
        gap[off:off + k] = False
    want = C.flat_expected(control)
    clipped = 0
    for s in range(C.FLAT_STEPS):
        opt.zero_grad(set_to_none=False)
        for w, g in zip(params, case["grads"][s]):
            w.grad.copy_(torch.from_numpy(g.copy()))
        opt.step()
        row = want[s]
        got = {"p": opt.flat_param, "m": opt.exp_avg, "v": opt.exp_avg_sq}
        for key, t in got.items():
            a = t.cpu().numpy()
            for off, k in zip(offs, C.FLAT_SIZES):
                C.assert_bits(f"step {s + 1} {key} slice at {off}", a[off:off + k],
                              row[key][off:off + k])
            assert not a.view(np.uint32)[gap].any(), (s, key)
            assert not row[key].view(np.uint32)[gap].any()
        if control:
            st = opt.stats()
            assert F32(st["lr"]).tobytes() == row["lr"].tobytes()
            assert F32(st["grad_norm"]).tobytes() == row["norm"].tobytes()
            assert F32(st["clip_coef"]).tobytes() == row["coef"].tobytes()
            clipped += row["coef"] < 1
    assert opt.views_intact() and opt.stats()["step"] == C.FLAT_STEPS
    assert int(bits(opt._step_state)[1:].abs().sum()) == 0
    if control:
        assert clipped == C.FLAT_STEPS // 2                        # both branches were taken
