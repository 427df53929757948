"""GPU: the fused CRPS losses (csrc/gine_loss.hip: k_crps, k_crps_tw and the head backward run
inside the pass) row by row against the 50-digit oracle (tests/loss_oracle.py), at every xi, u, c
and t of tests/loss_cases.py, whose docstring has the table, the bounds and what was measured.

The C entry points are called with the test's own buffers, so the fp64 ``dpred``, ``loss`` and
``count`` and the fp32 ``grad_unit`` are all read.  Shapes: N in {1, 63, 64, 65, 255, 256, 257,
1031} (a partial wave, one wave, a workgroup and one row either side of it, five workgroups);
256 * 257 + 3 rows (plain, tw) and 64 * 257 + 1 (head form): the smallest that give the
last-workgroup finish a second round of its stride loop; head backward in the pass at D in {4, 36,
128, 132, 256} (one float4 lane; a ragged first chunk; one full chunk; one lane into the second
chunk; two full chunks).
"""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import loss_cases as LC
from helpers import rel_err
from raincast_gnn import _lib, gradbuf, head
from raincast_gnn import loss as L
from raincast_gnn.postprocess import PostProcess
from test_gpu_head import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CODE = {"normal": _lib.LOSS_NORMAL, "mixed_normal": _lib.LOSS_MIXED_NORMAL,
        "mixed": _lib.LOSS_MIXED, "mixed_u": _lib.LOSS_MIXED_U}
NAMES = {"normal": ("NormalCRPS", "False"), "mixed_normal": ("MixedNormalCRPS", "False"),
         "mixed": ("MixedLoss", "False"), "mixed_u": ("MixedLoss", "True")}
SIZES = (1, 63, 64, 65, 255, 256, 257, 1031)


def scalars(kind, cb):
    """(u, xi, c, t) as the loss classes pass them to the launch."""
    return (cb["u"] if kind == "mixed" else 0.0, cb["xi"] if cb["xi"] is not None else 0.5,
            float(cb["c"]), float(cb["t"]))


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class Buffers:
    """Device buffers of one launch of N rows (the sizes the package allocates)."""

    def __init__(self, n, K):
        n_part = ctypes.c_int32(0)
        _lib.call("gine_crps_num_partials", n, ctypes.byref(n_part))
        self.dpred = torch.full((n, K), float("nan"), dtype=torch.float64, device=DEV)
        self.unit = torch.full((n, K), float("nan"), dtype=torch.float32, device=DEV)
        self.partials = torch.zeros(n_part.value, 2, dtype=torch.float64, device=DEV)
        self.loss = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        self.count = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.parts = torch.zeros(_lib.COUNT_PARTS, dtype=torch.int32, device=DEV)


def launch(kind, cb, pred, y, tw=None, grad=True, buf=None):
    """gine_crps(_tw)_fwd(_grad) on device tensors pred [N, K] fp32, y [N] fp32 -> Buffers."""
    n, K = pred.shape
    b = buf or Buffers(n, K)
    st = _lib.stream_handle(DEV)
    args = [_lib.ptr(pred), _lib.ptr(y), n, CODE[kind], *scalars(kind, cb)]
    if tw is not None:
        args += [float(tw[0]), float(tw[1])]
    args += [_lib.ptr(b.dpred), _lib.ptr(b.partials), _lib.ptr(b.loss), _lib.ptr(b.count),
             _lib.ptr(b.ticket)]
    name = "gine_crps_tw_fwd" if tw is not None else "gine_crps_fwd"
    if grad:
        _lib.call("gine_count_valid", _lib.ptr(y), n, _lib.ptr(b.parts), st)
        args += [_lib.ptr(b.parts), _lib.ptr(b.unit)]
        name += "_grad"
    _lib.call(name, *args, st)
    return b


def backward(kind, b, n, seed, tw=None):
    g = torch.tensor([seed], dtype=torch.float64, device=DEV)
    out = torch.full(b.dpred.shape, float("nan"), dtype=torch.float32, device=DEV)
    st = _lib.stream_handle(DEV)
    if tw is None:
        _lib.call("gine_crps_bwd", _lib.ptr(b.dpred), _lib.ptr(b.count), _lib.ptr(g), n, CODE[kind],
                  _lib.ptr(out), st)
    else:
        _lib.call("gine_crps_tw_bwd", _lib.ptr(b.dpred), _lib.ptr(b.count), _lib.ptr(g), n,
                  CODE[kind], float(tw[0]), float(tw[1]), _lib.ptr(out), st)
    return out


def rows_for(kind, cb, n, first=0):
    """The table tiled or truncated to n rows from row ``first`` on, about 5 % of the targets NaN
    (none for n = 1) -> (idx [n], P [n, K], y [n] with the NaN, valid [n])."""
    P, y, _ = LC.table(kind, cb)
    idx = (first + np.arange(n)) % len(y)
    yy = y[idx].copy()
    if n > 1:
        gone = np.random.default_rng(n).random(n) < 0.05
        gone[0] = False
        yy[gone] = np.nan
    return idx, np.ascontiguousarray(P[idx]), yy, ~np.isnan(yy)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the table's arrays are read-only)


# ------------------------------------------------------------------------------ per-row value
@pytest.mark.parametrize("kind,cb", LC.ALL, ids=LC.ALL_IDS)
def test_row_values(kind, cb):
    """gine_crps_fwd and gine_crps_tw_fwd with N = 1, once per row of the table and form: the
    launch's loss is the row's value, held to the row's value bound; count is 1."""
    P, y, _ = LC.table(kind, cb)
    R, K = P.shape
    Pd, yd = dev(P), dev(y)
    worst = {}
    for tw_t, tw_w in LC.forms(kind, cb):
        tw = None if tw_t is None else (tw_t, tw_w)
        b = Buffers(1, K)
        loss = torch.full((R,), float("nan"), dtype=torch.float64, device=DEV)
        count = torch.zeros(R, dtype=torch.float64, device=DEV)
        dpred = torch.full((R, K), float("nan"), dtype=torch.float64, device=DEV)
        st = _lib.stream_handle(DEV)
        for i in range(R):
            args = [Pd.data_ptr() + 4 * K * i, yd.data_ptr() + 4 * i, 1, CODE[kind],
                    *scalars(kind, cb)]
            if tw is not None:
                args += [float(tw_t), float(tw_w)]
            args += [dpred.data_ptr() + 8 * K * i, _lib.ptr(b.partials), loss.data_ptr() + 8 * i,
                     count.data_ptr() + 8 * i, _lib.ptr(b.ticket), st]
            _lib.call("gine_crps_fwd" if tw is None else "gine_crps_tw_fwd", *args)
        assert torch.all(count == 1.0) and b.ticket.item() == 0
        LC.merge(worst, LC.check_rows(kind, cb, np.arange(R), loss.cpu().numpy(),
                                      dpred.cpu().numpy(), tw_t, tw_w))
    print(f"{LC.combo_id(kind, cb)}: " + ", ".join(
        f"{k} value {v[0]:.1e} gradient {v[1]:.1e}" for k, v in worst.items()))


# --------------------------------------------------------------------------- per-row gradient
@pytest.mark.parametrize("kind,cb", LC.ALL, ids=LC.ALL_IDS)
def test_row_gradients_means_and_roundings(kind, cb):
    """One launch over the table per form and N: ``dpred`` row by row within the gradient bound
    and exactly 0 on NaN targets, ``loss`` the oracle's mean, ``count`` exact; bitwise,
    ``grad_unit`` = float32(dpred / count) and gine_crps(_tw)_bwd = float32(seed * dpred / count)."""
    worst = {}
    for n in SIZES:
        idx, P, y, ok = rows_for(kind, cb, n, first=7 * n)
        Pd, yd = dev(P), dev(y)
        forms = LC.forms(kind, cb)
        if n not in (1, 257):  # every threshold at two sizes, two of them at the others
            forms = forms[:1] + forms[1 + 2 * (n % 5):3 + 2 * (n % 5)]
        for tw_t, tw_w in forms:
            tw = None if tw_t is None else (tw_t, tw_w)
            b = launch(kind, cb, Pd, yd, tw)
            dpred = b.dpred.cpu().numpy()
            cnt = b.count.item()
            assert cnt == ok.sum() and b.ticket.item() == 0
            assert np.all(dpred[~ok] == 0.0) and torch.all(b.unit[dev(~ok)] == 0.0)
            LC.merge(worst, LC.check_rows(kind, cb, idx[ok], None, dpred[ok], tw_t, tw_w))
            mean, bound = LC.mean_bound(kind, cb, idx[ok], tw_t, tw_w)
            assert abs(b.loss.item() - mean) <= bound, (n, tw, b.loss.item(), mean, bound)
            unit = (dpred / cnt).astype(np.float32)
            assert np.array_equal(b.unit.cpu().numpy().view(np.int32), unit.view(np.int32))
            if n in (1, 65, 1031):
                for seed in (1.0, 2.5):
                    got = backward(kind, b, n, seed, tw).cpu().numpy()
                    want = (seed * dpred / cnt).astype(np.float32)
                    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, seed)
                    if seed == 1.0:
                        assert np.array_equal(got.view(np.int32), b.unit.cpu().numpy().view(np.int32))
            plain = launch(kind, cb, Pd, yd, tw, grad=False)   # the form without grad_unit
            assert torch.equal(bits(plain.dpred), bits(b.dpred))
            assert torch.equal(bits(plain.loss), bits(b.loss)) and plain.count.item() == cnt
    print(f"{LC.combo_id(kind, cb)}: " + ", ".join(
        f"{k} gradient {v[1]:.1e}" for k, v in worst.items()))


# ----------------------------------------------------------------------- more than 256 partials
def _pick(kind, **want):
    return next((kind, cb) for cb in LC.combos(kind) if all(cb[k] == v for k, v in want.items()))


# one combination per kind, away from the defaults
BIG = [_pick("normal"), _pick("mixed_normal", c=-2.0),
       _pick("mixed", xi=LC.f32(0.8), u=LC.f32(0.3), c=-2.0),
       _pick("mixed_u", xi=LC.f32(0.2), c=-2.0, t=1.0)]
BIG_IDS = [LC.combo_id(k, cb) for k, cb in BIG]


def regular_rows(kind, cb, n):
    """The table's regular rows tiled to n, about 5 % NaN targets."""
    P, y, _ = LC.table(kind, cb)
    idx = np.arange(n) % LC.N_REGULAR
    yy = y[idx].copy()
    yy[np.random.default_rng(n).random(n) < 0.05] = np.nan
    return idx, np.ascontiguousarray(P[idx]), yy, ~np.isnan(yy)


def check_against_torch(kind, cb, P, y, ok, dpred, loss, tw=None, min_finite=0.3):
    """The fp64 torch formulation on the CPU over the rows themselves: the gradient row by row
    where torch's is finite, the mean against math.fsum.  Bounds: the kernel's against the oracle
    plus the reference's own measured error, by each row's class -> worst gradient error."""
    tw_t, tw_w = tw if tw is not None else (None, 0.0)
    P, y = P[ok], y[ok]
    rval, rgrad = LC.reference(kind, P, y, cb, tw_t, tw_w)
    cls = LC.row_class(kind, P)
    bv = np.array([LC.BOUNDS[c][0] + LC.MEASURED[c][0] for c in cls])
    bg = np.array([LC.BOUNDS[c][1] + LC.MEASURED[c][1] for c in cls])
    fin = np.isfinite(rgrad).all(axis=1)
    assert np.isfinite(rval).all() and fin.mean() >= min_finite, fin.mean()
    eg = np.abs(dpred[ok] - rgrad).max(axis=1) / np.maximum(np.abs(rgrad).max(axis=1), 1.0)
    assert np.all(eg[fin] <= bg[fin]), float((eg[fin] / bg[fin]).max())
    n = len(y)
    bound = math.fsum(bv * LC.term_scale(kind, P, y, cb, tw_t)) / n \
        + (math.log2(n) + 2) * 2.0 ** -53 * math.fsum(np.abs(rval)) / n
    ref = LC.fsum_mean(rval)
    assert abs(loss - ref) <= bound, (loss, ref, bound)
    return float(eg[fin].max())


@pytest.mark.parametrize("tw", [None, (-1.0, 0.3)], ids=["plain", "tw"])
@pytest.mark.parametrize("kind,cb", BIG, ids=BIG_IDS)
def test_finish_past_256_partials(kind, cb, tw):
    """N = 256 * 257 + 3: 258 workgroups, so the last one's stride loop over the partials takes a
    second round.  Regular rows tiled; against the fp64 torch formulation where its gradient is
    finite (every row at xi = 0.5; the rows above u - sigma_u / xi otherwise) and against the
    oracle on every row; the mean against math.fsum; the same bits on a second call; the ticket
    back at 0 after each call and after an N = 0 call, which gives a NaN loss and count 0."""
    n = 256 * 257 + 3
    idx, P, y, ok = regular_rows(kind, cb, n)
    Pd, yd = dev(P), dev(y)
    b = launch(kind, cb, Pd, yd, tw)
    assert b.ticket.item() == 0 and b.count.item() == ok.sum()
    again = launch(kind, cb, Pd, yd, tw, buf=None)
    assert again.ticket.item() == 0
    for a_, b_ in ((again.dpred, b.dpred), (again.loss, b.loss), (again.count, b.count)):
        assert torch.equal(bits(a_), bits(b_))
    assert torch.equal(bits(again.unit), bits(b.unit))
    reuse = launch(kind, cb, Pd, yd, tw, buf=b)               # the same buffers and ticket again
    assert reuse.ticket.item() == 0 and torch.equal(bits(reuse.loss), bits(again.loss))
    dpred, loss = b.dpred.cpu().numpy(), b.loss.item()
    tw_t, tw_w = tw if tw is not None else (None, 0.0)
    assert np.all(dpred[~ok] == 0.0)
    worst = LC.check_rows(kind, cb, idx[ok], None, dpred[ok], tw_t, tw_w)
    mean, bound = LC.mean_bound(kind, cb, idx[ok], tw_t, tw_w)
    assert abs(loss - mean) <= bound, (loss, mean, bound)
    check_against_torch(kind, cb, P, y, ok, dpred, loss, tw)
    unit = (dpred / b.count.item()).astype(np.float32)
    assert np.array_equal(b.unit.cpu().numpy().view(np.int32), unit.view(np.int32))
    empty = launch(kind, cb, Pd[:0], yd[:0], tw, grad=False, buf=b)
    assert math.isnan(empty.loss.item()) and empty.count.item() == 0.0 and empty.ticket.item() == 0
    print(f"{LC.combo_id(kind, cb)} {'tw' if tw else 'plain'}: value "
          f"{abs(loss - mean):.1e} (bound {bound:.1e}), gradient {worst['regular'][1]:.1e}")


# ------------------------------------------------------------- the head backward inside the pass
def head_case(kind, N, D, seed=0):
    K = LC.WIDTH[kind]
    g = torch.Generator().manual_seed(1000 * D + 10 * N + K + seed)
    h = torch.randn(N, D, generator=g)
    lin = torch.nn.Linear(D, K)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(K, D, generator=g) / math.sqrt(D))
        lin.bias.copy_(torch.tensor([-0.5, 0.3, -0.2, 0.1, 0.4][:K]))
    y = torch.from_numpy(LC.FC.make_targets(N, seed=2))
    y[0] = 0.5 if N > 1 else 2.0
    return h, lin, y


def run_head(kind, cb, h, lin, y, unit):
    """head.head -> the fused loss -> backward: the cached unit seed (the pass's own head
    backward) or a fresh seed tensor (gine_crps_bwd, then gine_head_bwd)."""
    u, xi, c, t = scalars(kind, cb)
    hd = h.to(DEV).requires_grad_(True)
    ld = copy.deepcopy(lin).to(DEV)
    yd = y.to(DEV)
    pred = head.head(hd, ld, CODE[kind], yd)
    val = L._fused(pred, yd, CODE[kind], u=u, xi=xi, c=c, t=t)
    rec = head.record_of(pred)
    assert rec is not None and rec.pre is not None       # the pass ran the head backward
    out = dict(val=val.detach().clone(), pred=pred.detach().clone(),
               dpred=val.grad_fn.saved_tensors[0].clone(), unit=rec.pre[0].clone(),
               dh_pass=rec.pre[1].clone())
    if unit:
        gradbuf.loss_backward(val)
    else:
        val.backward()
    torch.cuda.synchronize()
    out.update(dh=hd.grad.clone(), dw=ld.weight.grad.clone(), db=ld.bias.grad.clone())
    return out


def regroup(n, loss):
    """Two fixed-order fp64 sums of the same n non-negative rows in different groupings (64 or 256
    rows per workgroup): each within (log2 n + 2) half-ulps of the exact mean."""
    return 2 * (math.log2(n) + 2) * 2.0 ** -53 * abs(loss)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.abs().max().item()
    return (a - b).abs().max().item() / (den if den > 0 else 1.0)


HEAD_CB = {"normal": LC.combos("normal")[0], "mixed_normal": LC.combos("mixed_normal")[0],
           "mixed": dict(xi=0.5, u=LC.f32(1.71), c=LC.C, t=5.0),
           "mixed_u": dict(xi=0.5, u=None, c=LC.C, t=5.0)}


@pytest.mark.parametrize("D", [4, 36, 128, 132, 256])
@pytest.mark.parametrize("kind", LC.KINDS)
def test_head_backward_in_the_pass(kind, D):
    """k_crps<KIND, 1> (D <= 128) and <KIND, 2> at N in {1, 63, 64, 65, 200}: dh of the unit-seeded
    path bit-identical to the separate gine_head_bwd launch, dW / db within 1e-6 normwise of it
    (test_head_backward_in_crps_pass_matches_separate_launch's claim, at the model's D = 128
    there); dpred, grad_unit and dh within test_gpu_head's TOL of PostProcess(linear) and the
    loss in fp64 torch; the head form's dpred and grad_unit bit-equal to the plain form's (the
    loss to the regrouping of its sum: 64 rows per workgroup there, 256 here)."""
    cb = HEAD_CB[kind]
    name, grad_u = NAMES[kind]
    worst = 0.0
    for N in (1, 63, 64, 65, 200):
        h, lin, y = head_case(kind, N, D)
        fus = run_head(kind, cb, h, lin, y, unit=True)
        sep = run_head(kind, cb, h, lin, y, unit=False)
        assert torch.equal(bits(fus["val"]), bits(sep["val"]))
        assert torch.equal(bits(fus["dh"]), bits(fus["dh_pass"]))          # the pass's own dh was used
        assert torch.equal(bits(fus["dh"]), bits(sep["dh"])), (N, _rel(fus["dh"], sep["dh"]))
        assert rel_err(fus["dw"], sep["dw"]) <= 1e-6 and rel_err(fus["db"], sep["db"]) <= 1e-6
        # the plain form on the same prediction and targets
        b = launch(kind, cb, fus["pred"], y.to(DEV))
        assert torch.equal(bits(b.dpred), bits(fus["dpred"]))
        assert torch.equal(bits(b.unit), bits(fus["unit"]))
        assert abs(b.loss.item() - fus["val"].item()) <= regroup(N, b.loss.item())
        assert L._ticket(DEV).item() == 0
        # fp64 restatement
        ok = ~torch.isnan(y)
        h64 = h.double().requires_grad_(True)
        w64 = lin.weight.detach().double().requires_grad_(True)
        b64 = lin.bias.detach().double().requires_grad_(True)
        pred64 = PostProcess(name, grad_u)(torch.nn.functional.linear(h64, w64, b64))
        pred64.retain_grad()
        rows = LC.torch_rows(kind, pred64[ok], y[ok].double(), cb)
        ref = rows.mean()
        ref.backward()
        cnt = int(ok.sum())
        errs = [_rel(fus["pred"], pred64), _rel(fus["dpred"], pred64.grad * cnt),
                _rel(fus["unit"], pred64.grad), _rel(fus["dh"], h64.grad),
                _rel(fus["dw"], w64.grad), _rel(fus["db"], b64.grad),
                abs(fus["val"].item() - ref.item()) / abs(ref.item())]
        worst = max(worst, max(errs))
        assert max(errs) <= TOL, (N, errs)
    print(f"{kind} D={D}: {worst:.1e} of the fp64 restatement")


@pytest.mark.parametrize("kind", LC.KINDS)
def test_head_form_finish_past_256_partials(kind):
    """N = 64 * 257 + 1 at D = 4 through head.head -> the fused loss -> gradbuf.loss_backward: 258
    workgroups of 64 nodes.  The plain form on the same prediction gives the same dpred and
    grad_unit bits (its 65 workgroups sum in another grouping: the loss to that regrouping); dh as the
    separate launch's; the same bits on a second run; the package's ticket back at 0."""
    cb = HEAD_CB[kind]
    N, D = 64 * 257 + 1, 4
    assert N <= L.HEAD_BWD_MAX_NODES
    h, lin, y = head_case(kind, N, D)
    fus = run_head(kind, cb, h, lin, y, unit=True)
    assert L._ticket(DEV).item() == 0
    again = run_head(kind, cb, h, lin, y, unit=True)
    assert L._ticket(DEV).item() == 0
    for k in ("val", "dpred", "unit", "dh", "dw", "db"):
        assert torch.equal(bits(again[k]), bits(fus[k])), k
    sep = run_head(kind, cb, h, lin, y, unit=False)
    assert torch.equal(bits(fus["dh"]), bits(sep["dh"]))
    assert rel_err(fus["dw"], sep["dw"]) <= 1e-6 and rel_err(fus["db"], sep["db"]) <= 1e-6
    b = launch(kind, cb, fus["pred"], y.to(DEV))
    assert torch.equal(bits(b.dpred), bits(fus["dpred"])) and torch.equal(bits(b.unit), bits(fus["unit"]))
    ok = ~torch.isnan(y)
    assert b.count.item() == int(ok.sum())
    assert abs(b.loss.item() - fus["val"].item()) <= regroup(N, b.loss.item())
    # the fp64 torch formulation on the pass's own fp32 prediction, row by row
    dpred = fus["dpred"].cpu().numpy()
    assert np.all(dpred[~ok.numpy()] == 0.0)
    err = check_against_torch(kind, cb, fus["pred"].cpu().numpy(), y.numpy(), ok.numpy(), dpred,
                              fus["val"].item(), min_finite=1.0)
    print(f"{kind}: per-row gradient {err:.1e} of the fp64 torch formulation")


# ----------------------------------------------------------------------- through the loss classes
CLASS_CASES = [
    ("mixed", dict(xi=0.2, u=0.3, c=-2.0, t=5.0), None),
    ("mixed", dict(xi=0.8, u=0.3, c=LC.C, t=5.0), (-1.0, 0.3)),
    ("mixed_u", dict(xi=0.8, u=None, c=-2.0, t=1.0), None),
    ("mixed_u", dict(xi=0.2, u=None, c=-2.0, t=1.0), (-3.0, 1.0)),
    ("mixed_normal", dict(xi=None, u=None, c=-2.0, t=5.0), None),
    ("mixed_normal", dict(xi=None, u=None, c=-2.0, t=5.0), (-3.0, 0.3)),
]


@pytest.mark.parametrize("kind,raw_cb,tw", CLASS_CASES)
def test_loss_classes_pass_their_scalars(kind, raw_cb, tw):
    """MixedLoss(grad_u, xi, u, t=, c=) and MixedNormalCRPS(c=) with non-default scalars given as
    plain Python numbers, N = 257 on the device, against the oracle at the fp32-rounded xi and u:
    the value at the value bound (an xi or u that arrived unrounded, or a default in its place,
    is 1e-9 or more away), the fp32 gradient to its rounding."""
    cb = next(c for c in LC.combos(kind)
              if all(c[k] == (LC.f32(v) if k in ("xi", "u") and v is not None else v)
                     for k, v in raw_cb.items()))
    kw = {} if tw is None else dict(tw_threshold=tw[0], tw_weight=tw[1])
    if kind == "mixed_normal":
        fn = L.MixedNormalCRPS(c=raw_cb["c"], **kw)
    else:
        fn = L.MixedLoss(kind == "mixed_u", raw_cb["xi"], raw_cb["u"], t=raw_cb["t"], c=raw_cb["c"], **kw)
    if tw is not None:
        assert tw[0] in LC.thresholds(kind, cb)
    idx, P, y, ok = rows_for(kind, cb, 257)
    pred = dev(P).requires_grad_(True)
    val = fn.crps(pred, dev(y))
    val.backward()
    tw_t, tw_w = tw if tw is not None else (None, 0.0)
    mean, bound = LC.mean_bound(kind, cb, idx[ok], tw_t, tw_w)
    assert val.dtype == torch.float64
    assert abs(val.item() - mean) <= bound, (val.item(), mean, bound)
    _, og = LC.oracle(kind, cb, tw_t, tw_w)
    want = np.where(ok[:, None], og[idx], 0.0) / ok.sum()
    got = pred.grad.cpu().numpy().astype(np.float64)
    tol = 2.0 ** -23 * np.maximum(np.abs(og[idx]).max(axis=1, keepdims=True), 1.0) / ok.sum()
    assert np.all(np.abs(got - want) <= tol)
    assert np.all(got[~ok] == 0.0)
