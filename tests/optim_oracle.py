"""Two oracles of the AdamW step, its learning-rate schedule, its clip coefficient and the
gradient norm of csrc/gine_optim.hip, independent of raincast_gnn (numpy, fractions, mpmath).

The definition they restate is the kernel's own: the `AdamW` functor and the
scalar formation in `k_adamw` / `k_adamw_ctl`, from the fp32 lr, beta1, beta2, eps and
weight_decay that the C ABI receives.

Oracle A, the bit target (scalars, step_a).  numpy float32, one rounding per operation:

    decay = f32(1 - f64(lr) f64(wd))          w1 = 1f - beta1
    nss   = f32(-(f64(lr) / (1 - f64(beta1)^t)))   w2 = 1f - beta2
    bc2   = f32(sqrt(1 - f64(beta2)^t))
    p = p decay;  m = m + w1 (g - m);  v = v beta2;  v = v + (w2 g) g
    den = sqrt(v) / bc2 + eps;  p = p + nss (m / den)

In control mode g is f32(g coef) and lr is the scheduled lr_t.  The three double-precision
scalars are evaluated with mpmath at 60 digits and rounded ONCE to fp32 (fl32, round to
nearest even, subnormals included).  The device forms them with pow, sqrt and cospi in double,
none of them guaranteed correctly rounded: a handful of fp64 operations, each within a few
2^-53, with the worst amplification in 1 - beta2^t at t = 1 (1,000 x), stay below 2^-42
relative.  So the oracle is the device's value whenever the exact scalar lies at least 2^-40
relative away from an fp32 rounding boundary; fl32 returns that margin and the tests assert
MARGIN on every (lr, beta, t) they use.  An exact zero (lr_t at the end of a schedule with
ratio 0) has no boundary near it and reports an infinite margin.

Oracle B, exact real arithmetic (step_b).  One step on the same fp32 inputs and the same
five fp32 scalars with NO rounding: m' and v' as fractions.Fraction, p' through mpmath at 60
digits (sqrt and two quotients, 1e-60 relative).  It bounds oracle A, and through it the
kernel, componentwise.  Model of one fp32 operation: fl(x) = x (1 + d) + h with |d| <= U =
2^-24 and |h| <= TAU = 2^-150 (h only where a product or quotient can underflow; sums, differences
and square roots have h = 0).  G(k) = k U / (1 - k U).

  m' = fl(m + fl(w1 fl(g - m))): three roundings on the terms, one possible underflow:
      E_m = G(3) (|m| + w1 |g - m|) + 2 TAU
  v' = fl(fl(v beta2) + fl(fl(w2 g) g)): four roundings, all terms non-negative, three possible
  underflows (the one inside w2 g is multiplied by |g|):
      E_v = G(4) (v beta2 + w2 g^2) + 3 TAU (1 + |g|)
  p' by intervals along the chain, each line one operation (x: exact value, E: bound so far):
      sqrt:   E_sq = max(sqrt(v' + E_v) - sqrt(v'), sqrt(v') - sqrt(max(v' - E_v, 0)))
              E_s  = E_sq + U (sqrt(v') + E_sq)
      / bc2:  E_q  = E_s / bc2 + U (q + E_s / bc2) + TAU,     q = sqrt(v') / bc2
      + eps:  E_den = E_q + U (den + E_q),                    den = q + eps
      m / den: E_r = E_0 + U (|r| + E_0) + TAU,  E_0 = (E_m + |r| E_den) / (den - E_den),
              r = m' / den   (no bound where den <= E_den: eps = 0 at v' = 0, pinned apart)
      nss r:  E_t  = |nss| E_r + U |nss| (|r| + E_r) + TAU
      p decay: E_1 = U |p decay| + TAU
      sum:    E_p  = E_1 + E_t + U (|p decay| + |nss r| + E_1 + E_t)
The model has no overflow: elements whose inputs or oracle A outputs are not finite are outside
oracle B (step_b returns None for them) and are pinned by explicit expectations instead.

The norm (sumsq_partials, norm_exact) and the schedule (lr_exact) are described at the
functions.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 60

F32 = np.float32
U = Fraction(1, 1 << 24)
TAU = Fraction(1, 1 << 150)
MARGIN = 2.0 ** -40
ONE = F32(1)

CONSTANT, COSINE, LINEAR = 0, 1, 2      # GINE_LR_* (include/gine_hip.h)


def G(k):
    return k * U / (1 - k * U)


def frac(x):
    """Exact Fraction of a binary floating-point scalar or of an mpf."""
    if isinstance(x, Fraction):
        return x
    if isinstance(x, MP.mpf):
        sign, man, exp, _ = x._mpf_
        q = Fraction(int(man)) * Fraction(2) ** int(exp)
        return -q if sign else q
    return Fraction(float(x))


def mpf(q):
    if isinstance(q, Fraction):
        return MP.mpf(q.numerator) / MP.mpf(q.denominator)
    return MP.mpf(float(q)) if not isinstance(q, MP.mpf) else q


def fl32(x):
    """(round-to-nearest-even fp32 of x, relative distance of x from the nearest fp32 rounding
    boundary).  x: Fraction, mpf or float; gradual underflow; overflow gives inf."""
    q = frac(x)
    if q == 0:
        return F32(0), math.inf
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    e = max(e, -126)
    quantum = Fraction(2) ** (e - 23)
    x = a / quantum
    n = x.numerator // x.denominator
    rest = x - n
    near = abs(rest - Fraction(1, 2))
    if n == 1 << 23 and e > -126:      # just above a power of two: the ulp below is half
        near = min(near, rest + Fraction(1, 4))
    margin = float(near * quantum / a)
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    val = math.ldexp(n, e - 23) if e - 23 + n.bit_length() <= 128 else math.inf
    with np.errstate(over="ignore"):
        val = F32(val)
    return (-val if q < 0 else val), margin


def scalars(lr, beta1, beta2, eps, wd, t):
    """The seven fp32 values of the AdamW functor at step t (1-based) and the smallest boundary
    margin of the three that pass through double precision."""
    lr, beta1, beta2, eps, wd = (F32(x) for x in (lr, beta1, beta2, eps, wd))
    t = int(t)
    L, B1, B2, WD = (MP.mpf(float(x)) for x in (lr, beta1, beta2, wd))
    decay, m0 = fl32(1 - L * WD)
    nss, m1 = fl32(-(L / (1 - MP.power(B1, t))))
    if lr == 0:
        nss = F32(-0.0)                    # -(0 / x): the sign decides p = -0 + nss * r
    bc2, m2 = fl32(MP.sqrt(1 - MP.power(B2, t)))
    return {"decay": decay, "nss": nss, "bc2": bc2, "w1": ONE - beta1, "w2": ONE - beta2,
            "beta2": beta2, "eps": eps, "margin": min(m0, m1, m2)}


def torch_scalars(lr, beta1, beta2, eps, wd, t):
    """The same seven values the way torch.optim.AdamW forms them from Python doubles: 1 - beta
    in double, then rounded (the kernel subtracts the already rounded fp32 betas)."""
    t = int(t)
    L, B1, B2, WD = (MP.mpf(float(x)) for x in (lr, beta1, beta2, wd))
    return {"decay": fl32(1 - L * WD)[0], "nss": fl32(-(L / (1 - MP.power(B1, t))))[0],
            "bc2": fl32(MP.sqrt(1 - MP.power(B2, t)))[0], "w1": F32(1.0 - float(beta1)),
            "w2": F32(1.0 - float(beta2)), "beta2": F32(beta2), "eps": F32(eps)}


def step_a(p, g, m, v, sc, coef=None):
    """Oracle A: one step on fp32 arrays; returns new (p, m, v).  coef: the clip coefficient of
    control mode (g becomes f32(g coef))."""
    p, g, m, v = (np.asarray(x) for x in (p, g, m, v))
    assert all(x.dtype == np.float32 for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        if coef is not None:
            g = g * F32(coef)
        p = p * sc["decay"]
        m = m + sc["w1"] * (g - m)
        v = v * sc["beta2"]
        v = v + (sc["w2"] * g) * g
        den = np.sqrt(v) / sc["bc2"] + sc["eps"]
        p = p + sc["nss"] * (m / den)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def step_b(p, g, m, v, sc):
    """Oracle B on one element (fp32 scalars): None outside the model, else a dict with the
    exact m, v (Fraction), p (mpf) and the bounds E_m, E_v (Fraction), E_p (mpf or inf)."""
    if not all(np.isfinite(x) for x in (p, g, m, v)):
        return None
    pa, ma, va = step_a(*(np.array([x], dtype=np.float32) for x in (p, g, m, v)), sc)
    if not (np.isfinite(pa[0]) and np.isfinite(ma[0]) and np.isfinite(va[0])):
        return None
    P, Gr, M, V = frac(p), frac(g), frac(m), frac(v)
    w1, w2, b2 = frac(sc["w1"]), frac(sc["w2"]), frac(sc["beta2"])
    mx = M + w1 * (Gr - M)
    vx = V * b2 + w2 * Gr * Gr
    e_m = G(3) * (abs(M) + w1 * abs(Gr - M)) + 2 * TAU
    e_v = G(4) * (V * b2 + w2 * Gr * Gr) + 3 * TAU * (1 + abs(Gr))
    u, tau = mpf(U), mpf(TAU)
    bc2, eps, nss = (mpf(frac(sc[k])) for k in ("bc2", "eps", "nss"))
    vm, evm, em = mpf(vx), mpf(e_v), mpf(e_m)
    root = MP.sqrt(vm)
    lo = vm - evm if vm > evm else MP.mpf(0)
    e_sq = max(MP.sqrt(vm + evm) - root, root - MP.sqrt(lo))
    e_s = e_sq + u * (root + e_sq)
    q = root / bc2
    e_q = e_s / bc2 + u * (q + e_s / bc2) + tau
    den = q + eps
    e_den = e_q + u * (den + e_q)
    p1 = mpf(P * frac(sc["decay"]))
    if den <= e_den:
        return {"m": mx, "v": vx, "p": None, "E_m": e_m, "E_v": e_v, "E_p": MP.inf}
    r = mpf(mx) / den
    e_0 = (em + abs(r) * e_den) / (den - e_den)
    e_r = e_0 + u * (abs(r) + e_0) + tau
    e_t = abs(nss) * e_r + u * abs(nss) * (abs(r) + e_r) + tau
    e_1 = u * abs(p1) + tau
    e_p = e_1 + e_t + u * (abs(p1) + abs(nss * r) + e_1 + e_t)
    return {"m": mx, "v": vx, "p": p1 + nss * r, "E_m": e_m, "E_v": e_v, "E_p": e_p}


# -- the schedule -------------------------------------------------------------------------
def lr_exact(lr, kind, W, T, r, t):
    """lr_t of step t (1-based) in exact arithmetic on the control block's fp32 fields (mpf;
    cospi is exact at s = 0, 0.5, 1):  constant lr;  t <= W: lr t / W;  else with
    s = min(1, (t - W) / max(1, T - W))  cosine lr (r + (1 - r) (1 + cos(pi s)) / 2),
    linear lr (r + (1 - r) (1 - s))."""
    lr, W, T, r = (MP.mpf(float(F32(x))) for x in (lr, W, T, r))
    if kind not in (COSINE, LINEAR):
        return lr
    t = MP.mpf(int(t))
    if t <= W:
        return lr * t / W
    s = min(MP.mpf(1), (t - W) / max(MP.mpf(1), T - W))
    if kind == COSINE:
        return lr * (r + (1 - r) * (1 + MP.cospi(s)) / 2)
    return lr * (r + (1 - r) * (1 - s))


def lr_f32(lr, kind, W, T, r, t):
    """(fp32 lr_t, boundary margin)."""
    return fl32(lr_exact(lr, kind, W, T, r, t))


# -- the norm and the clip coefficient ----------------------------------------------------
def num_blocks(n):
    """The grid of gine_grad_sumsq and of both steps: min(512, ceil(ceil(n / 4) / 256))."""
    return min(512, -(-max(-(-n // 4), 1) // 256)) if n > 0 else 0


def sumsq_partials(g):
    """fp64 restatement of k_grad_sumsq in its documented order; [blocks, 2] float64 {sum of
    squares, number of non-finite values}.  Thread tid of the grid takes float4 tid, tid +
    stride, ... in x, y, z, w order, then (the grid's first n % 4 threads) one tail element;
    the 64 lanes of a wave combine by butterfly over xor 32, 16, ..., 1; the four waves of a
    workgroup add in order.  The square of an fp32 value is exact in fp64; adding the +0.0 of
    an element that does not exist changes no bit, so missing float4s are zero-padded."""
    g = np.asarray(g)
    assert g.dtype == np.float32 and g.ndim == 1
    n = g.size
    blocks = num_blocks(n)
    threads = blocks * 256
    n4 = n // 4
    trips = max(-(-n4 // threads), 1)
    with np.errstate(all="ignore"):
        sq = g.astype(np.float64) ** 2
        bad_e = (~np.isfinite(g)).astype(np.int64)
        body = np.zeros(trips * threads * 4)
        body[:4 * n4] = sq[:4 * n4]
        body = body.reshape(trips, threads, 4)
        bad_b = np.zeros(trips * threads * 4, dtype=np.int64)
        bad_b[:4 * n4] = bad_e[:4 * n4]
        acc = np.zeros(threads)
        for k in range(trips):
            for c in range(4):
                acc = acc + body[k, :, c]
        bad = bad_b.reshape(trips, threads, 4).sum(axis=(0, 2))
        tail = n - 4 * n4
        acc[:tail] = acc[:tail] + sq[4 * n4:]
        bad[:tail] += bad_e[4 * n4:]
        acc = acc.reshape(-1, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ off]
        waves = acc[:, 0].reshape(blocks, 4)
        total = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    return np.stack([total, bad.reshape(blocks, 256).sum(1).astype(np.float64)], axis=1)


def norm_f32(partials):
    """total_norm as k_adamw_ctl forms it: the partial sums added in index order in fp64, the
    fp64 square root, one conversion to fp32."""
    s = np.float64(0)
    with np.errstate(all="ignore"):
        for x in partials[:, 0]:
            s = s + x
        return F32(np.sqrt(s))


def sumsq_exact(g):
    """Exact sum of squares of a finite fp32 array (Fraction)."""
    g = np.asarray(g)
    assert g.dtype == np.float32 and np.isfinite(g).all()
    f, e = np.frexp(g.astype(np.float64))
    man = np.ldexp(f, 24).astype(np.int64)          # |man| <= 2^24, g = man 2^(e - 24)
    e = e.astype(np.int64) - 24
    tot = {}
    for ex in np.unique(e):
        sel = man[e == ex]
        tot[int(ex)] = sum(int(x) * int(x) for x in sel.tolist())
    if not tot:
        return Fraction(0)
    lo = 2 * min(tot)
    return Fraction(sum(s << (2 * ex - lo) for ex, s in tot.items())) * Fraction(2) ** lo


def norm_exact(g):
    """sqrt of the exact sum of squares (mpf)."""
    return MP.sqrt(mpf(sumsq_exact(g)))


def clip_coef(max_norm, norm):
    """min(1, f32(max_norm / f32(norm + 1e-6f))) in fp32, as clip_grad_norm_ forms it; exactly 1
    without a bound (max_norm <= 0 or inf).  A NaN quotient stays a NaN."""
    max_norm, norm = F32(max_norm), F32(norm)
    if not (max_norm > 0 and np.isfinite(max_norm)):
        return ONE
    with np.errstate(all="ignore"):
        q = max_norm / (norm + F32(1e-6))
    return ONE if q > ONE else q
