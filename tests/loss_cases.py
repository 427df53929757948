"""The row table and the checks of the fused CRPS losses (csrc/gine_loss.hip: k_crps, k_crps_tw)
against tests/loss_oracle.py, shared by the CPU tests (tests/test_loss_rows.py: the oracle's
anchoring and the measurement of the fp64 reference) and the GPU tests
(tests/test_gpu_loss_rows.py: the kernels): the same rows at the same bounds on either device.

Scalars: xi in {0.2, 0.5, 0.8} and a fixed u in {1.71, 0.3}, both as their fp32 roundings (what
the loss classes pass), c in {log 0.01, -2}, t in {5, 1}; every combination of the scalars a kind
reads (1 + 2 + 12 + 12 launches' worth).  Forms: the plain loss, and (1 - w) L + w twCRPS at
w in {0.3, 1} and five thresholds: c - 1, c, -1 (between c and every u), exactly u (fixed u; for
"mixed_u" 1.0, with rows whose u is one fp32 ulp either side of it and regular rows on both
sides), 2.5 (above every u): tw_censored, crps_mixed with c := t', and tw_tail.

Rows (fp32): 40 seeded rows in PostProcess's ranges (forecast_cases.make_params / make_targets),
then edge rows as explicit numbers around mu 0.4, sigma 0.9, p 0.3, sigma_u 0.7 (u 1.3 for
"mixed_u"): y == fp32(c), y < c, y = -9; y == u, one fp32 ulp below and above, u + 1e-3, u + 0.2,
u + 50 sigma_u; sigma and sigma_u at 1e-3 and at the 1e-6 floor; p = 0, 1, 1e-7; mu = -30 at
sigma 0.5 (all mass on the atom: gradient exactly 0); mu = 12; sigma = sigma_u = 30; for "mixed_u"
u = 2.12e-4 and 2.1199, each also with y == u.

Errors are per row, never over the batch:
  value     |v - oracle| / (sigma (1 + |z_y| + |z_c| + |z_u|) + sigma_u (1 + |y - u| / sigma_u)),
            the terms the kind has; with a tw term, whose closed form has t' in the place of c and
            whose tail form measures from t', + sigma |z_t'| + |t' - u|
  gradient  max_k |g_k - oracle_k| / max(|oracle|_inf, 1)   (1: the natural size of d / d mu)
and the rows fall into classes by their smallest scale min(sigma, sigma_u), since z and the
derivatives in the scales grow as 1 / scale and the rounding errors of any fp64 evaluation with
them: "regular" >= 1e-2, "milli" (the 1e-3 rows), "floor" (the 1e-6 rows).

Measured: the package's torch formulation on float64 inputs (CPU) against the oracle, over every
row, combination and form (test_loss_rows.py::test_reference_measurement reproduces it), and the
kernels' bounds, 16 times that and never below 64 fp64 ulp = 1.4e-14 (the margin: last-place
differences between device and host erf / exp / pow under the same conditioning):

             reference, value   gradient    bound, value   gradient    MI355X, value   gradient
  regular        2.5e-16         1.5e-14       1.4e-14      2.4e-13       2.6e-16       1.3e-14
  milli          2.7e-16         1.1e-12       1.4e-14      1.8e-11       2.6e-16       1.1e-12
  floor          1.5e-16         4.9e-10       1.4e-14      7.8e-9        1.4e-16       8.3e-10

(MI355X: the worst over tests/test_gpu_loss_rows.py, printed with -s.)  The reference is measured
where its gradient is finite: every row at xi = 0.5.  At xi != 0.5 torch.where hands a NaN to the
branch not taken in two places, and those rows are measured at xi = 0.5 only; the kernels
differentiate the chosen branch alone and are held to the oracle there at every xi:
  - the plain term for y <= u - sigma_u / xi (pow of a negative base behind `x_re <= 0`);
  - the tw term in its tail form (t' >= u) once (t' - u) / sigma_u >= (2^(53 xi) - 1) / xi
    (7.8e3 at xi = 0.2: the sigma_u-floor rows at t' = 2.5), where the unused body form's 1 - cdf
    has rounded to 0 and pow's slope there is infinite.

What stays out of the table, because the fp64 reference itself is not finite there and the kernel
evaluates the same expression: the plain loss at (y - u) / sigma_u >= (2^(53 xi) - 1) / xi (7.8e3,
1.9e8, 7.3e12 for xi = 0.2, 0.5, 0.8).  1 - (1 + xi r)^(-1/xi) rounds to 1, 1 - cdf to 0, and the
derivative of (1 - cdf)^(1 - xi) is infinite: an inf or NaN gradient in the reference and in
k_crps alike.  The largest r in the table is 50.  For "mixed_u", a tw threshold exactly equal to a
row's learned u is out as well: torch.maximum splits the gradient in u evenly at the tie, the
kernel takes the tail form with t' a constant; the rows one ulp either side are in.
"""
import functools
import itertools
import math

import numpy as np
import torch

import forecast_cases as FC
import loss_oracle as LO

C = LO.C
KINDS = ("normal", "mixed_normal", "mixed", "mixed_u")
WIDTH = LO.WIDTH
XIS = (0.2, 0.5, 0.8)
US = (1.71, 0.3)
CS = (C, -2.0)
TS = (5.0, 1.0)
TW_WEIGHTS = (0.3, 1.0)
N_REGULAR = 40
U_ROW = 1.3          # the u column of the mixed_u edge rows
U_TW = 1.0           # mixed_u: the tw threshold with rows' u one fp32 ulp either side of it
FLOOR = 1e-6         # PostProcess: softplus(.) + 1e-6


def f32(x):
    return float(np.float32(x))


def combos(kind):
    """Every launch-scalar set of a kind as dicts (xi, u, c, t): only the scalars it reads vary."""
    if kind == "normal":
        return [dict(xi=None, u=None, c=C, t=5.0)]
    if kind == "mixed_normal":
        return [dict(xi=None, u=None, c=c, t=5.0) for c in CS]
    if kind == "mixed":
        return [dict(xi=f32(xi), u=f32(u), c=c, t=5.0) for xi, u, c in itertools.product(XIS, US, CS)]
    return [dict(xi=f32(xi), u=None, c=c, t=t) for xi, c, t in itertools.product(XIS, CS, TS)]


def combo_id(kind, cb):
    bits = [kind]
    if cb["xi"] is not None:
        bits.append(f"xi{cb['xi']:.1f}")
    if cb["u"] is not None:
        bits.append(f"u{cb['u']:.2f}")
    if kind != "normal":
        bits.append(f"c{cb['c']:.1f}")
    if kind == "mixed_u":
        bits.append(f"t{cb['t']:.0f}")
    return "-".join(bits)


ALL = [(k, cb) for k in KINDS for cb in combos(k)]
ALL_IDS = [combo_id(k, cb) for k, cb in ALL]


def _key(cb):
    return (cb["xi"], cb["u"], cb["c"], cb["t"])


def thresholds(kind, cb):
    """Below c, at c, between c and u, exactly u (for "mixed_u": U_TW, which rows' u surround),
    above every u."""
    c = cb["c"]
    at_u = cb["u"] if kind == "mixed" else (U_TW if kind == "mixed_u" else f32(1.71))
    return (c - 1.0, c, -1.0, at_u, 2.5)


@functools.lru_cache(maxsize=None)
def _table(kind, u, c):
    K = WIDTH[kind]
    tail = kind in ("mixed", "mixed_u")
    P = FC.make_params(kind, N_REGULAR).astype(np.float64)
    y = FC.make_targets(N_REGULAR).astype(np.float64)
    y[np.isnan(y)] = 0.5
    rows = [list(p) + [yy] for p, yy in zip(P, y)]
    tags = ["regular"] * N_REGULAR
    U = u if kind == "mixed" else (U_ROW if kind == "mixed_u" else 1.71)
    U = f32(U)
    cf = f32(c)
    up = float(np.nextafter(np.float32(U), np.float32(np.inf)))
    dn = float(np.nextafter(np.float32(U), np.float32(-np.inf)))

    def add(tag, y, mu=0.4, sigma=0.9, p=0.3, su=0.7, uc=U, only_tail=False):
        if only_tail and not tail:
            return
        rows.append([mu, sigma, p, su, uc][:K] + [y])
        tags.append(tag)

    add("y == c", cf)
    add("y < c", cf - 1.5)
    add("y == c, mu below", cf, mu=-6.0)
    add("y == u", U)
    add("y == u - ulp", dn)
    add("y == u + ulp", up)
    add("y = u + 50 sigma_u", U + 50 * 0.7)
    add("y = u + 1e-3", U + 1e-3)
    add("y = u + 0.2", U + 0.2)
    add("sigma 1e-3, y == c", cf, sigma=1e-3)
    add("sigma 1e-3, y near mu", 0.4005, sigma=1e-3)
    add("sigma floor, y near mu", 0.4 + 2e-6, sigma=FLOOR)
    add("sigma floor, y == c", cf, sigma=FLOOR)
    add("sigma floor, mu at u", U + 1e-6, mu=U, sigma=FLOOR, only_tail=True)
    add("sigma_u 1e-3", U + 2e-3, su=1e-3, only_tail=True)
    add("sigma_u 1e-3, y below", 0.2, su=1e-3, only_tail=True)
    add("sigma_u floor", U + 3e-6, su=FLOOR, only_tail=True)
    add("sigma_u floor, y below", 0.2, su=FLOOR, only_tail=True)
    add("p = 0", 0.9, p=0.0)
    add("p = 0, y == c", cf, p=0.0)
    add("p = 1", 0.9, p=1.0)
    add("p = 1, y == c", cf, p=1.0)
    add("p = 1e-7", 0.9, p=1e-7)
    add("p = 1e-7, y above u", U + 1.0, p=1e-7)
    add("all mass on the atom, y == c", cf, mu=-30.0, sigma=0.5)
    add("all mass on the atom, y above", 0.9, mu=-30.0, sigma=0.5)
    add("mu far above u", 11.0, mu=12.0)
    add("mu far above u, y == c", cf, mu=12.0)
    add("large scales", 3.0, sigma=30.0, su=30.0)
    add("large scales, y == c", cf, sigma=30.0, su=30.0)
    add("y = -9", -9.0)
    if kind == "mixed_u":
        for uc in (2.12e-4, 2.1199):
            add("u at its range's end", 0.5, uc=uc)
            add("u at its range's end, y == c", cf, uc=uc)
            add("u at its range's end, y == u", f32(uc), uc=uc)
        for uc in (float(np.nextafter(np.float32(U_TW), np.float32(s))) for s in (0.0, 2.0)):
            add("u one ulp off the tw threshold", 0.5, uc=uc)
            add("u one ulp off the tw threshold, y above", 2.0, uc=uc)
            add("u one ulp off the tw threshold == y", uc, uc=uc)
    A = np.array(rows, dtype=np.float32)
    P32, y32 = np.ascontiguousarray(A[:, :K]), np.ascontiguousarray(A[:, K])
    for a in (P32, y32):
        a.setflags(write=False)
    return P32, y32, tuple(tags)


def table(kind, cb):
    """-> (P [R, K] float32, y [R] float32, tags): the regular rows, then the edge rows."""
    return _table(kind, cb["u"], cb["c"])


CLASSES = ("regular", "milli", "floor")


def row_class(kind, P):
    """The class of each row by its smallest scale, min(sigma, sigma_u): "regular" from 1e-2 up
    (what softplus of an O(1) raw gives), "milli" around 1e-3, "floor" below 5e-4 (the rows at
    PostProcess's 1e-6).  z = (x - mu) / sigma and the derivatives in sigma grow as the scale
    shrinks, and the reference's rounding errors with them."""
    P = np.asarray(P, dtype=np.float64)
    small = P[:, 1] if P.shape[1] <= 3 else np.minimum(P[:, 1], P[:, 3])
    return np.where(small < 5e-4, "floor", np.where(small < 1e-2, "milli", "regular"))


def term_scale(kind, P, y, cb, tw_t=None):
    """sigma (1 + |z_y| + |z_c| + |z_u|) + sigma_u (1 + |y - u| / sigma_u) per row, with the terms
    the kind has.  With a tw term, whose closed form has t' in the place of c: + sigma |z_t'|, and
    + |t' - u| for the kinds with a tail."""
    P, y = np.asarray(P, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mu, s = P[:, 0], P[:, 1]
    z = 1 + np.abs(y - mu) / s
    if tw_t is not None:
        tp = tw_t if kind == "normal" else max(tw_t, cb["c"])
        z = z + np.abs(tp - mu) / s
    if kind != "normal":
        z = z + np.abs(cb["c"] - mu) / s
    out = s * z
    if kind in ("mixed", "mixed_u"):
        u = P[:, 4] if kind == "mixed_u" else cb["u"]
        out = s * (z + np.abs(u - mu) / s) + P[:, 3] * (1 + np.abs(y - u) / P[:, 3])
        if tw_t is not None:
            out = out + np.abs(tp - u)
    return out


# ------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def _oracle_plain(kind, key):
    xi, u, c, t = key
    P, y, _ = _table(kind, u, c)
    out = []
    for i in range(len(y)):
        r = LO.plain(kind, [float(x) for x in P[i]], float(y[i]), xi, u, c, t)
        out.append((r.v, r.d))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_tw(kind, key, tw_t):
    xi, u, c, _ = key
    P, y, _ = _table(kind, u, c)
    out = []
    for i in range(len(y)):
        r = LO.tw(kind, [float(x) for x in P[i]], float(y[i]), tw_t, xi, u, c)
        out.append((r.v, r.d))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(kind, key, tw_t, tw_w):
    K = WIDTH[kind]
    pl = _oracle_plain(kind, key)
    if tw_t is None:
        mix = pl
    else:
        w = LO.mp.mpf(tw_w)
        # the tw term does not read t: one evaluation serves both t of "mixed_u"
        tws = _oracle_tw(kind, key[:3] + (5.0,), tw_t)
        mix = [(w * b[0] + (1 - w) * a[0], [w * db + (1 - w) * da for da, db in zip(a[1], b[1])])
               for a, b in zip(pl, tws)]
    val = np.array([float(v) for v, _ in mix])
    grad = np.array([[float(e) for e in d] for _, d in mix]).reshape(len(mix), K)
    val.setflags(write=False)
    grad.setflags(write=False)
    return val, grad


def oracle(kind, cb, tw_t=None, tw_w=0.0):
    """Values [R] and gradients [R, K] of the table's rows (float64, rounded once), read-only."""
    return _oracle(kind, _key(cb), tw_t, tw_w if tw_t is not None else 0.0)


# ------------------------------------------------------ the fp64 reference: the torch formulation
def torch_rows(kind, pred, y, cb, tw_t=None, tw_w=0.0):
    """The package's torch formulation on float64 tensors ``pred [N, K]`` and ``y [N]`` (no NaN)
    -> rows [N, 1], differentiable.  xi and u go in as float64 tensors holding the fp32-rounded
    numbers (a plain Python float would make them fp32 tensors, and -1 / xi an fp32 quotient).
    "normal": twcrps._normal, the formula of NormalCRPS with 1/sqrt(pi) in fp64 (the class keeps
    the reference's fp32 constant, 1.1e-8 sigma away; the kernel does not)."""
    from raincast_gnn import _lib, twcrps
    from raincast_gnn.loss import MixedLoss, MixedNormalCRPS
    assert pred.dtype == torch.float64 and y.dtype == torch.float64
    c = np.float64(cb["c"])
    if kind == "normal":
        rows = twcrps._normal(pred[:, 0:1], pred[:, 1:2], y[:, None])
        code = _lib.LOSS_NORMAL
    elif kind == "mixed_normal":
        rows = MixedNormalCRPS(reduce=False, c=c).crps(pred, y)
        code = _lib.LOSS_MIXED_NORMAL
    else:
        grad_u = kind == "mixed_u"
        fn = MixedLoss(grad_u, np.float64(cb["xi"]), None if grad_u else np.float64(cb["u"]),
                       reduce=False, t=cb["t"], c=c)
        rows = fn.crps(pred, y)
        code = _lib.LOSS_MIXED_U if grad_u else _lib.LOSS_MIXED
    assert rows.shape == (len(y), 1) and rows.dtype == torch.float64
    if tw_t is not None:
        t = torch.full((1, 1), float(tw_t), dtype=torch.float64)
        tw = twcrps.tw_rows_of(code, pred, y[:, None], t, cb["u"], float(c), cb["xi"])
        rows = tw if tw_w == 1.0 else (1.0 - tw_w) * rows + tw_w * tw
    return rows


def reference(kind, P, y, cb, tw_t=None, tw_w=0.0):
    """:func:`torch_rows` on the CPU -> (values [N], gradients [N, K] by autograd of the rows'
    sum)."""
    pred = torch.from_numpy(np.asarray(P, dtype=np.float64)).clone().requires_grad_(True)
    rows = torch_rows(kind, pred, torch.from_numpy(np.asarray(y, dtype=np.float64)), cb, tw_t, tw_w)
    rows.sum().backward()
    return rows.detach().numpy()[:, 0], pred.grad.numpy()


def row_errors(kind, P, y, cb, val, grad, oval, ograd, tw_t=None):
    """-> (value error / term scale [N], gradient error / max(|g_oracle|_inf, 1) [N]); a
    non-finite entry gives inf."""
    ev = np.abs(np.asarray(val) - oval) / term_scale(kind, P, y, cb, tw_t)
    eg = np.abs(np.asarray(grad) - ograd).max(axis=1) / np.maximum(np.abs(ograd).max(axis=1), 1.0)
    ev[~np.isfinite(ev)] = np.inf
    eg[~np.isfinite(eg)] = np.inf
    return ev, eg


def forms(kind, cb):
    """The loss forms of a combination: the plain loss, then every threshold and weight."""
    return [(None, 0.0)] + [(t, w) for t in thresholds(kind, cb) for w in TW_WEIGHTS]


# The fp64 reference's worst per-row errors against the oracle over the whole table, every
# combination and form (test_loss_rows.py::test_reference_measurement reproduces them), and the
# kernels' bounds: 16 times that, never below 64 fp64 ulp.
MEASURED = {"regular": (2.5e-16, 1.5e-14), "milli": (2.7e-16, 1.1e-12), "floor": (1.5e-16, 4.9e-10)}   # class -> (value, gradient)
ULP64 = 64 * 2.0 ** -52
BOUNDS = {k: tuple(max(16.0 * e, ULP64) for e in v) for k, v in MEASURED.items()}


def check_rows(kind, cb, idx, val, grad, tw_t=None, tw_w=0.0):
    """Rows ``idx`` of the table as some device computed them (``val`` may be None): every row
    within its class's bounds -> worst errors {class: [value, gradient]}."""
    P, y, tags = table(kind, cb)
    oval, ograd = oracle(kind, cb, tw_t, tw_w)
    idx = np.asarray(idx)
    Pi, yi = P[idx], y[idx]
    ev, eg = row_errors(kind, Pi, yi, cb, oval[idx] if val is None else val, grad, oval[idx],
                        ograd[idx], tw_t)
    cls = row_class(kind, Pi)
    worst = {}
    for name in CLASSES:
        sel = cls == name
        if not sel.any():
            continue
        bv, bg = BOUNDS[name]
        worst[name] = [float(ev[sel].max()), float(eg[sel].max())]
        bad = sel & ((ev > bv) | (eg > bg))
        if bad.any():
            j = int(np.flatnonzero(bad)[0])
            raise AssertionError(
                f"{combo_id(kind, cb)} tw=({tw_t}, {tw_w}) row {int(idx[j])} [{tags[int(idx[j])]}] "
                f"pred={Pi[j].tolist()} y={float(yi[j])!r}: value error {ev[j]:.2e} (bound {bv:.1e}), "
                f"gradient error {eg[j]:.2e} (bound {bg:.1e}); {int(bad.sum())} rows out")
    return worst


def mean_bound(kind, cb, idx, tw_t=None, tw_w=0.0):
    """The oracle's mean over rows ``idx`` (math.fsum) and the bound of a device's mean: every
    row's value bound, averaged, plus a fixed-order fp64 summation of n terms (a tree of depth
    log2 n, then one division)."""
    P, y, _ = table(kind, cb)
    oval, _ = oracle(kind, cb, tw_t, tw_w)
    idx = np.asarray(idx)
    scale = term_scale(kind, P[idx], y[idx], cb, tw_t)
    per_row = np.array([BOUNDS[c][0] for c in row_class(kind, P[idx])]) * scale
    n = len(idx)
    summing = (math.log2(n) + 2) * 2.0 ** -53 * math.fsum(np.abs(oval[idx])) / n
    return fsum_mean(oval[idx]), math.fsum(per_row) / n + summing


def merge(worst, more):
    for k, v in more.items():
        w = worst.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], v[0]), max(w[1], v[1])
    return worst


def fsum_mean(values):
    return math.fsum(float(v) for v in values) / len(values)
