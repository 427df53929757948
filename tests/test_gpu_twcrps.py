"""GPU: the threshold-weighted CRPS kernels -- gine_forecast_twcrps, gine_ensemble_twcrps
(csrc/gine_forecast.hip) and gine_crps_tw_fwd / _fwd_grad / _bwd (csrc/gine_loss.hip) -- against
the independent oracle (tests/twcrps_oracle.py; cases and bounds in tests/twcrps_cases.py) and,
for the fused loss, against the package's fp64 torch formulation with autograd.

Shapes: score kernel n in {1, 65, 257, 1031} (one row; a 64-row tile and a row; several
workgroups; more than 16 of them, not a multiple of 64); ensemble N in {1, 64, 257} x
M in {1, 2, 11, 51, 64}; loss N in {1, 63, 257} (a partial wave; more than one 256-thread
workgroup).

Measured on an MI355X (printed with -s): rows against the oracle's closed forms 2.9e-13 of scale
(bound 1e-12), against quadrature 1.2e-12 with quad's own estimate at 1.2e-9 (xi = 0.2); ensemble
2.7e-15 absolute; fused loss value 1.0e-7, gradient 4.9e-7, and 8.8e-6 for the single row of N = 1
at t = 1 (a row with 1e-10 of its mass above t: a gradient of 1e-11 from O(1) terms on both sides).
"""
import copy

import numpy as np
import pytest
import torch

import ensemble_cases as EC
import forecast_cases as FC
import twcrps_cases as TC
from helpers import rel_err
from raincast_gnn import RawEnsemble, _lib, evaluate
from raincast_gnn.ensemble import skill
from raincast_gnn.forecast import Forecast
from raincast_gnn.models import GNN, make_loss
from raincast_gnn.postprocess import PostProcess

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------ the score kernel
@pytest.mark.parametrize("kind,xi", FC.KIND_XI)
@pytest.mark.parametrize("n", [1, 65, 257, 1031])
def test_score_kernel_matches_the_oracle(n, kind, xi):
    b, a, e = TC.check_rows(kind, xi, n, DEV, with_quad=(n == 65))
    msg = f", quadrature {a:.1e} (quad's estimate {e:.1e})" if n == 65 else ""
    print(f"n={n} {kind} xi={xi}: closed {b:.1e}{msg} of scale")


@pytest.mark.parametrize("kind,xi", [("normal", None), ("mixed", 0.5), ("mixed_u", 0.2)])
def test_score_kernel_edges(kind, xi):
    P, y, x, _ = TC.case(kind, xi, 257)
    fc, _ = FC.build(kind, xi, np.array(P), DEV)
    yt = torch.from_numpy(np.array(y)).to(DEV)
    full = fc.twcrps(yt, np.array(x), rows=True)
    lean = fc.twcrps(yt, np.array(x))                       # rows = NULL
    assert lean.rows is None
    assert torch.equal(bits(lean.mean), bits(full.mean)) and torch.equal(lean.valid, full.valid)
    again = fc.twcrps(yt, np.array(x), rows=True)          # the same bits every run
    assert torch.equal(bits(again.rows), bits(full.rows))
    assert torch.equal(bits(again.mean), bits(full.mean))
    none = fc.twcrps(yt, [], rows=True)                     # T = 0: the count alone
    assert none.mean.shape == (0,) and none.rows.shape == (257, 0)
    assert none.valid.item() == float((~np.isnan(y)).sum())
    gone = fc.twcrps(torch.full((257,), float("nan"), device=DEV), [1.0, 2.5], rows=True)
    assert gone.valid.item() == 0 and torch.isnan(gone.mean).all() and torch.isnan(gone.rows).all()
    empty = Forecast(torch.zeros(0, P.shape[1], device=DEV), kind,
                     u=FC.U_FIXED if kind == "mixed" else None, xi=xi)
    e = empty.twcrps(torch.zeros(0, device=DEV), [1.0], rows=True)   # N = 0: nothing launched
    assert e.valid.item() == 0 and torch.isnan(e.mean).all() and e.rows.shape == (0, 1)
    inf = fc.twcrps(yt, [float("inf")], rows=True)
    assert torch.all(inf.rows[~torch.isnan(yt)] == 0.0) and inf.mean.item() == 0.0


def test_score_kernel_captured_with_device_thresholds():
    """One capture; the thresholds are a device tensor refilled in place between replays."""
    kind, xi = "mixed", 0.5
    P, y, x, _ = TC.case(kind, xi, 257)
    fc, _ = FC.build(kind, xi, np.array(P), DEV)
    yt = torch.from_numpy(np.array(y)).to(DEV)
    first = torch.tensor([-1.0, 1.0, 2.5], dtype=torch.float64, device=DEV)
    second = torch.tensor([FC.C, FC.U_FIXED, 4.0], dtype=torch.float64, device=DEV)
    want = [fc.twcrps(yt, t.clone(), rows=True) for t in (first, second)]
    static = first.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fc.twcrps(yt, static, rows=True)  # warm-up: ticket and allocations
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = fc.twcrps(yt, static, rows=True)
    for t, w in zip((first, second), want):
        static.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(got.rows), bits(w.rows))
        assert torch.equal(bits(got.mean), bits(w.mean)) and torch.equal(got.valid, w.valid)


# ------------------------------------------------------------------------- the ensemble kernel
@pytest.mark.parametrize("M", [1, 2, 11, 51, 64])
@pytest.mark.parametrize("n", [1, 64, 257])
def test_ensemble_kernel_matches_the_double_sum(n, M):
    mem, y, ref = TC.ensemble_case(n, M)
    raw = EC.raw_on(mem, DEV)
    assert raw.on_kernel
    worst = TC.check_ensemble(raw, y, ref)
    print(f"N={n} M={M}: {worst:.1e} abs")


def test_ensemble_strided_view_and_the_torch_path():
    n, col, scale, shift = 257, 7, 1.75, -1.25
    r = np.random.default_rng(11)
    ens = r.normal(0, 1, (n, 11, 35)).astype(np.float32)
    mem = EC.make_members(n, 11, seed=4)
    ens[:, :, col] = (mem - shift) / scale
    y = EC.make_targets(mem, seed=4)
    dev_ens = torch.from_numpy(ens).to(DEV)
    raw = RawEnsemble.from_batch(dev_ens, col, mean=shift, std=scale)
    assert raw.members.data_ptr() == dev_ens[:, :, col].data_ptr() and raw.on_kernel
    import ensemble_oracle as EO
    ref = TC.ensemble_reference(EO.values(ens[:, :, col], scale, shift), y)
    TC.check_ensemble(raw, y, ref)
    copy_ = RawEnsemble(dev_ens[:, :, col].contiguous(), scale=scale, shift=shift)
    yt = torch.from_numpy(y).to(DEV)
    a, b = raw.twcrps(yt, TC.ENS_THRESHOLDS), copy_.twcrps(yt, TC.ENS_THRESHOLDS)
    assert torch.equal(bits(a.rows), bits(b.rows)) and torch.equal(bits(a.fair_rows), bits(b.fair_rows))
    # 65 members: the torch formulation, on the device
    mem65, y65, ref65 = TC.ensemble_case(9, 65)
    big = EC.raw_on(mem65, DEV)
    assert not big.on_kernel
    TC.check_ensemble(big, y65, ref65)


# ------------------------------------------------------------------------------ the fused loss
LOSSES = [("normal", "NormalCRPS", "False"), ("mixed_normal", "MixedNormalCRPS", "False"),
          ("mixed", "MixedLoss", "False"), ("mixed_u", "MixedLoss", "True")]


def _raw_and_targets(kind, n):
    g = torch.Generator().manual_seed(100 + n)
    raw = torch.randn(n, FC.WIDTH[kind], generator=g)
    y = torch.from_numpy(FC.make_targets(n, seed=1))
    if n > 1:
        y[0] = 0.5  # at least one target
    else:
        y[0] = 2.0
    return raw, y


@pytest.mark.parametrize("weight", [0.3, 1.0])
@pytest.mark.parametrize("t", [-1.0, 1.0, 2.5])
@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("kind,name,grad_u", LOSSES)
def test_fused_tw_loss_matches_torch_formulation(kind, name, grad_u, n, t, weight):
    """The bounds of test_fused_crps_matches_torch_formulation: value 1e-6 relative, gradient
    rel_err 1e-5, against the package's torch formulation (CPU, autograd)."""
    raw, y = _raw_and_targets(kind, n)
    fn, _ = make_loss(name, grad_u, 1.71, 0.5, tw_threshold=t, tw_weight=weight)
    pp = PostProcess(name, grad_u)
    xg = raw.to(DEV).requires_grad_(True)
    v = fn.crps(pp(xg), y.to(DEV))
    v.backward()                                   # a fresh seed tensor: gine_crps_tw_bwd
    xc = raw.clone().requires_grad_(True)
    vc = fn.crps(pp(xc), y)
    vc.backward()
    assert v.dtype == vc.dtype
    ev = abs(v.item() - vc.item())
    eg = rel_err(xg.grad.cpu(), xc.grad)
    print(f"{kind} n={n} t={t} w={weight}: value {ev / max(abs(vc.item()), 1e-300):.1e}, "
          f"gradient {eg:.1e}")
    assert ev <= 1e-6 * abs(vc.item()), ev  # (NormalCRPS is fp32: a value of 1e-47 is 0 on both)
    assert eg <= 1e-5, eg


@pytest.mark.parametrize("kind,name,grad_u", LOSSES)
def test_fused_tw_loss_seeds_and_off_switch(kind, name, grad_u):
    from raincast_gnn import gradbuf
    raw, y = _raw_and_targets(kind, 257)
    pp = PostProcess(name, grad_u)
    yd = y.to(DEV)

    def run(seed, **tw):
        fn, _ = make_loss(name, grad_u, 1.71, 0.5, **tw)
        x = raw.to(DEV).requires_grad_(True)
        v = fn.crps(pp(x), yd)
        if seed is None:
            gradbuf.loss_backward(v)           # the cached unit seed: grad_unit as it is
        else:
            v.backward(torch.full_like(v, seed))  # gine_crps(_tw)_bwd
        return v.detach(), x.grad

    tw = dict(tw_threshold=1.0, tw_weight=0.3)
    v1, g1 = run(None, **tw)
    v2, g2 = run(1.0, **tw)
    v3, g3 = run(2.5, **tw)
    assert torch.equal(v1, v2) and torch.equal(v1, v3)
    assert torch.equal(g1, g2)                     # the unit gradient as _bwd rounds it
    assert rel_err(g3.cpu(), 2.5 * g1.cpu()) <= 1e-6
    plain = run(None)
    for off in (dict(tw_threshold=1.0, tw_weight=0.0), dict(tw_threshold=None, tw_weight=0.5)):
        v, g = run(None, **off)
        assert torch.equal(v, plain[0]) and torch.equal(g, plain[1])
    # all targets NaN: as the plain loss (NaN value, zero gradient)
    fn_tw, _ = make_loss(name, grad_u, 1.71, 0.5, **tw)
    fn, _ = make_loss(name, grad_u, 1.71, 0.5)
    nan_y = torch.full((257,), float("nan"), device=DEV)
    outs = []
    for f in (fn_tw, fn):
        x = raw.to(DEV).requires_grad_(True)
        v = f.crps(pp(x), nan_y)
        v.backward()
        outs.append((v.detach(), x.grad))
    assert torch.isnan(outs[0][0]) and torch.isnan(outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


def test_native_entry_rejects_bad_scalars():
    z = torch.zeros(4, 2, device=DEV)
    d = torch.zeros(8, dtype=torch.float64, device=DEV)
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    for t, w in ((1.0, -0.1), (1.0, 1.5), (float("inf"), 0.5), (float("nan"), 0.5)):
        rc = lib.gine_crps_tw_fwd(z.data_ptr(), z.data_ptr(), 4, _lib.LOSS_NORMAL, 0.0, 0.5, -4.6,
                                  5.0, t, w, d.data_ptr(), d.data_ptr(), d.data_ptr(),
                                  d.data_ptr(), tk.data_ptr(), None)
        assert rc == _lib.GINE_ERR_INVALID


# ------------------------------------------------------------------------------------ the model
def _tw_model():
    torch.manual_seed(0)
    return GNN(35, 128, 128, 2, loss="MixedLoss", grad_u="False", u=1.71, xi=0.5,
               tw_threshold=1.0, tw_weight=0.5)


def test_model_training_step_eager_and_captured():
    from raincast_gnn.data import synthetic_batch
    batch = synthetic_batch(500, 2, k=10).to(DEV)
    base = _tw_model()

    def step(m):
        for p in m.parameters():
            if p.grad is not None:
                p.grad.zero_()
        loss = m.loss_fn.crps(m(batch), batch.y)
        loss.backward()
        return loss

    m_e = copy.deepcopy(base).to(DEV).train()
    for _ in range(3):
        loss_e = step(m_e)
    for name, p in m_e.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        assert bool(torch.isfinite(p.grad).all()), name
    assert bool(m_e.aggr.weight.grad.abs().max() > 0) and bool(m_e.aggr.bias.grad.abs().max() > 0)

    m_g = copy.deepcopy(base).to(DEV).train()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(m_g)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_g = step(m_g)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e)
    for (name, pe), (_, pg) in zip(m_e.named_parameters(), m_g.named_parameters()):
        assert torch.equal(pe.grad, pg.grad), name
    for (name, be), (_, bg) in zip(m_e.named_buffers(), m_g.named_buffers()):
        assert torch.equal(be, bg), name

    # verify_tw on this model's predictions beside the batch's raw ensemble
    m_e.eval()
    with torch.no_grad():
        preds = m_e(batch)
    raw = RawEnsemble.from_batch(batch.ensemble, 0)
    out = evaluate.verify_tw(m_e, preds, batch.y, raw, [0.0, 1.0, 10.0])
    assert out.model.shape == out.ensemble.shape == out.skill.shape == out.valid.shape == (3,)
    ft = Forecast.from_model(m_e, preds).twcrps(batch.y, out.thresholds, rows=True)
    et = raw.twcrps(batch.y, out.thresholds)
    both = ~torch.isnan(ft.rows) & ~torch.isnan(et.rows)
    zero = torch.zeros_like(ft.rows)
    m = torch.where(both, ft.rows, zero).sum(0) / both.sum(0)
    e = torch.where(both, et.rows, zero).sum(0) / both.sum(0)
    assert torch.equal(out.skill, skill(m, e)) and torch.equal(out.skill, 1.0 - m / e)
