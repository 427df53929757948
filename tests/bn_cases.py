"""The case table, the derived bounds and the checkers of the BatchNorm statistics tests, shared
by the CPU tests (tests/test_bn_stats.py: an fp64 model of the documented algorithm and its
mutants) and the GPU tests (tests/test_gpu_bn_stats.py: the kernels), against tests/bn_oracle.py.

Cases.  case(N, D, step) is seeded by (N, D, step, SALT).  Every channel of a1 belongs to one
class
of A1_CLASSES and every channel of the intended dbn to one class of DBN_CLASSES:

  a1:  randn 0.5 + 2 randn | const 1.5 (var exactly 0) | mean100 100 + 0.01 randn |
       grid4096 4096 + (n mod 7) 2^-11 (var << eps, cond ~ 3e12) | small 1e-3 randn (var < eps) |
       big 3e5 randn | zero | onehot (row N // 2 is 1e4, the rest 0) | alt +1 / -1 |
       tiny30 1e-30 randn, |randn| >= 1/16 (below the accumulator's 2^-64) |
       neg1000 -1000 + randn |
       tiny12 1e-12 randn
  dbn: randn | e10 1e-10 randn | e18 1e-18 randn (at 2^-64) | const 0.75 | alt +1 / -1 (sd is
       exactly 0 for even N where the ReLU mask is all on) | xhat (proportional to xhat) |
       zero | onerow (row N // 3 only) | e4 1e4 randn

At D = 128 every (a1 class, dbn class) pair owns a column (108 of 128, the rest randn /
randn); at D = 32, 64 and 256 the columns cycle through PAIRS, 36 pairs that hold every class
of both kinds within their first 12.  gamma in [0.5, 1.5] with two negative entries, beta in
[-0.2, 0.2], running mean in [1, 3] and running var in [2, 3], eps = 1e-5.

The launches are reduced to the bare operation by W1 = I, so a1 = fl32(z + b1), and b1 is NOT
zero: a tile row past N that reached the sums would show (the padded rows of a tile are b1).
b1 is a multiple of 2^-10 in [0.25, 0.75], which makes z = class - b1 and z + b1 exact for the
const, grid4096, zero, onehot and alt classes.  The one exception: tiny30 and tiny12 cannot
exist in fp32 behind a bias of that size (fl32(z + b1) is a multiple of 2^-25 there), so b1
is 0 in the columns of those two classes and nowhere else.  tiny30 keeps |a1| >= 2^-104
(|randn| is lifted to 1/16): the split-bf16 product behind W1 = I returns x * 1 exactly only
while the lowest of x's three bf16 planes is a normal number, |x| >= 2^-110 (measured on the
MI355X: below 1e-33 the plane is lost and a1 is off in its last bits, the matrix product's
property and not BatchNorm's), and the tests assert a1 == fl32(z + b1).  All values are finite.

Bounds.  Derived, not measured; u = 2^-53, v = 2^-24, G the launch's workgroup count
(gine_mlp_num_partials), q = G 2^-65 on the accumulator path (each workgroup sum is rounded
once to 2^-64; the integer totals are exact and their conversion back to fp64 is within the
summation term below) and q = 0 on the partials path.  An fp64 sum of N terms in any order is
within (N - 1) u sum|x| of exact (tests/compare_cases.py uses the same bound); the N-th u pays
for the division by N, since |mean| <= A / N.  The squares a^2 and the products dbn * xhat of
fp32 numbers are exact in fp64.  Each stored fp32 is one rounding: a stored x whose fp64 value
is within E of exact is within v |x| + E + 2^-150 (the last term: half the spacing of fp32
subnormals).  With A = sum|a|, Q = sum a^2, per channel:

  d_mean = (N u A + q) / N                     stored mean: v |mean| + d_mean + 2^-150
  d_var  = (N u Q + q) / N + 4 u (Q / N + mean^2) + 2 |mean| d_mean
           (the sum; the division, the square, the subtraction and one spare; the mean)
  invstd: E_is = max |is(w) - is(var)| over w in {var + d_var, max(var - d_var, 0)} + 4 u is
           with is(w) = 1 / sqrt(w + eps32): the interval, not its linearisation, valid where
           d_var > var + eps; the kernels clamp var at 0, which only moves it towards var >= 0;
           4 u: the sum, the root and the quotient, one spare
  alpha:  E_al = |gamma| E_is + u |alpha|
  shift:  E_sh = |mean| E_al + |alpha| d_mean + d_mean E_al + u |mean alpha|
                 + u (|beta| + |mean alpha|)   -- the terms' magnitudes, not the result's
  running mean: E = f d_mean + 4 u (|f mean| + |(1 - f) rm|)
  running var:  E_unb = d_var N / (N - 1) + 2 u unbiased  (d_var at N = 1)
                E = f E_unb + 4 u (|f unbiased| + |(1 - f) rv|)
  (eval mode: mean = running_mean and var = running_var are exact, d_mean = d_var = 0)

Backward, with SD = sum|dbn|, SX = sum|dbn xhat| and xhat exact in the saved fp32 statistics.
The documented algorithm forms xhat = fl32(fl32(a1 - mean32) * invstd32) -- two fp32 roundings,
(1 + v)^2 - 1 = 2 v + v^2 relative per term, and an underflowing product loses at most 2^-149
-- before the exact fp64 product with dbn:

  d_sd = N u SD + q                            dbeta:  v |sd| + d_sd + 2^-150
  d_sx = (2 v + v^2) SX + N u (1 + 3 v) SX + 2^-149 SD + q
                                               dgamma: v |sx| + d_sx + 2^-150
  c1 = gamma * invstd32 is a 24 x 24 bit product, exact in fp64: the stored c1 must be its
       correctly rounded fp32, bit for bit
  c2: E = |c1| d_sx / N + 2 u |c2|   c3: E = |c1| d_sd / N + 2 u |c3|   (product, quotient)
  without batch statistics (training = 0) c2 and c3 are +0.0f exactly

Checkers return a Report: per quantity the worst |got - exact| / bound, the worst plain
relative error and the channel classes where they occurred; ok() is ratio <= 1 everywhere.
"""
import functools

import numpy as np

import bn_oracle as O

EPS = np.float32(1e-5)
MOMENTUM = np.float32(0.1)
A1_CLASSES = ("randn", "const", "mean100", "grid4096", "small", "big", "zero", "onehot", "alt",
              "tiny30", "neg1000", "tiny12")
DBN_CLASSES = ("randn", "e10", "e18", "const", "alt", "xhat", "zero", "onerow", "e4")
NO_BIAS = ("tiny30", "tiny12")
PAIRS = tuple((A1_CLASSES[k % 12], DBN_CLASSES[k % 9]) for k in range(36))
WELL = ("randn", "small", "big", "alt", "neg1000")   # well-conditioned a1 classes (the anchor)
SIZES = (1, 2, 33, 1031)
# part of every case's seed: with it the ReLU mask leaves at least 30 % of dbn non-zero at every
# tested (N, D, step), N = 1 at D = 32 included (the GPU tests assert a quarter)
SALT = 5
DIMS = (32, 64, 128, 256)

U = O.MP.mpf(2) ** -53
V = O.MP.mpf(2) ** -24
TINY = O.MP.mpf(2) ** -150


def columns(D):
    """[(a1 class, dbn class)] of the D columns."""
    if D == 128:
        full = [(a, d) for a in A1_CLASSES for d in DBN_CLASSES]
        return full + [("randn", "randn")] * (128 - len(full))
    return [PAIRS[c % len(PAIRS)] for c in range(D)]


def _a1_column(name, N, rng):
    n = np.arange(N)
    r = rng.standard_normal(N)
    return {"randn": 0.5 + 2 * r, "const": np.full(N, 1.5), "mean100": 100 + 0.01 * r,
            "grid4096": 4096 + (n % 7) * 2.0 ** -11, "small": 1e-3 * r, "big": 3e5 * r,
            "zero": np.zeros(N), "onehot": np.where(n == N // 2, 1e4, 0.0),
            "alt": np.where(n % 2 == 0, 1.0, -1.0),
            "tiny30": 1e-30 * np.copysign(np.maximum(np.abs(r), 1 / 16), r),
            "neg1000": -1000 + r, "tiny12": 1e-12 * r}[name]


def _dbn_column(name, N, rng, xhat):
    n = np.arange(N)
    r = rng.standard_normal(N)
    return {"randn": r, "e10": 1e-10 * r, "e18": 1e-18 * r, "const": np.full(N, 0.75),
            "alt": np.where(n % 2 == 0, 1.0, -1.0), "xhat": xhat, "zero": np.zeros(N),
            "onerow": np.where(n == N // 3, 1.5, 0.0), "e4": 1e4 * r}[name]


def _ro(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(N, D, step=0):
    """Read-only arrays of one case: z, b1, a1 = fl32(z + b1) (what a launch with W1 = I must
    store), dy (the intended dbn), gamma, beta, rm, rv and the per-column class names."""
    rng = np.random.default_rng([N, D, step, SALT])
    cols = columns(D)
    b1 = (np.rint(rng.uniform(0.25, 0.75, D) * 1024) / 1024).astype(np.float32)
    b1[[a in NO_BIAS for a, _ in cols]] = 0
    want = np.stack([_a1_column(a, N, rng) for a, _ in cols], axis=1).astype(np.float32)
    z = want - b1                                   # fp32
    a1 = z + b1                                     # fp32: fl32(z + b1)
    for c, (a, _) in enumerate(cols):
        if a in ("const", "grid4096", "zero", "onehot", "alt", "tiny30", "tiny12"):
            assert np.array_equal(a1[:, c], want[:, c]), a
    a64 = a1.astype(np.float64)
    xhat = (a64 - a64.mean(0)) / np.sqrt(a64.var(0) + float(EPS))
    dy = np.stack([_dbn_column(d, N, rng, xhat[:, c]) for c, (_, d) in enumerate(cols)],
                  axis=1).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, D).astype(np.float32)
    gamma[[1, D - 2]] *= -1
    return _ro({"N": N, "D": D, "z": z, "b1": b1, "a1": a1, "dy": dy, "gamma": gamma,
                "beta": rng.uniform(-0.2, 0.2, D).astype(np.float32),
                "rm": rng.uniform(1, 3, D).astype(np.float32),
                "rv": rng.uniform(2, 3, D).astype(np.float32), "cols": cols})


@functools.lru_cache(maxsize=None)
def forward_sums(N, D, step=0):
    """The oracle's exact sums of case(N, D, step)['a1'], computed once."""
    return O.forward_sums(case(N, D, step)["a1"])


class Report:
    """Worst |got - exact| / bound and worst relative error per quantity, with the classes."""

    def __init__(self):
        self.worst = {}      # quantity -> [ratio, class, rel, class]
        self.fails = []      # (quantity, channel, class, ratio)

    def add(self, what, c, cls, got, exact, bound):
        err = abs(O.mpf(float(got)) - exact)
        ratio = float(err / bound)
        rel = float(err / abs(exact)) if exact != 0 else (0.0 if err == 0 else float("inf"))
        w = self.worst.setdefault(what, [0.0, "-", 0.0, "-"])
        if ratio > w[0]:
            w[0], w[1] = ratio, cls
        if rel > w[2]:
            w[2], w[3] = rel, cls
        if not ratio <= 1.0:
            self.fails.append((what, c, cls, ratio))

    def exact_bits(self, what, c, cls, got, want):
        """A quantity held bit for bit: ratio 0 or inf."""
        same = np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)
        w = self.worst.setdefault(what, [0.0, "-", 0.0, "-"])
        if not same:
            w[0], w[1] = float("inf"), cls
            self.fails.append((what, c, cls, float("inf")))

    def ok(self):
        return not self.fails

    def line(self, site, N, D, **extra):
        parts = [f"BNSTAT site={site} N={N} D={D}"] + [f"{k}={v}" for k, v in extra.items()]
        for what, (ratio, rc, rel, lc) in self.worst.items():
            parts.append(f"{what}: ratio={ratio:.3g}@{'/'.join(rc)} rel={rel:.3g}@{'/'.join(lc)}")
        return " ".join(parts)

    def assert_ok(self):
        assert self.ok(), "outside the derived bound: " + "; ".join(
            f"{w} channel {c} ({'/'.join(k)}) ratio {r:.3g}" for w, c, k, r in self.fails[:8])


def save_bounds(mean, var, d_mean, d_var, gamma, beta, eps32=EPS):
    """Exact bn_save entries of one channel and their bounds: {row: (exact mpf, bound mpf)}."""
    m, w = O.mpf(mean), O.mpf(var)
    eps = O.mpf(O.frac(eps32))
    inv = 1 / O.MP.sqrt(w + eps)
    lo = w - d_var
    lo = lo if lo > 0 else O.MP.mpf(0)
    e_is = max(abs(1 / O.MP.sqrt(w + d_var + eps) - inv),
               abs(1 / O.MP.sqrt(lo + eps) - inv)) + 4 * U * inv
    g, b = O.mpf(O.frac(gamma)), O.mpf(O.frac(beta))
    alpha = g * inv
    e_al = abs(g) * e_is + U * abs(alpha)
    ma = abs(m * alpha)
    e_sh = abs(m) * e_al + abs(alpha) * d_mean + d_mean * e_al + U * ma + U * (abs(b) + ma)
    stored = lambda x, e: V * abs(x) + e + TINY
    return {"mean": (m, stored(m, d_mean)), "invstd": (inv, stored(inv, e_is)),
            "alpha": (alpha, stored(alpha, e_al)),
            "shift": (b - m * alpha, stored(b - m * alpha, e_sh))}


def stat_errors(ch, N, G, acc):
    """d_mean, d_var (mpf) of one channel (forward_channel's dict)."""
    q = O.MP.mpf(G) * O.MP.mpf(2) ** -65 if acc else O.MP.mpf(0)
    A, Q, m = O.mpf(ch["A"]), O.mpf(ch["Q"]), abs(O.mpf(ch["mean"]))
    d_mean = (N * U * A + q) / N
    d_var = (N * U * Q + q) / N + 4 * U * (Q / N + m * m) + 2 * m * d_mean
    return d_mean, d_var


def check_forward(sums, cols, save, gamma, beta, G, acc, running=None, eps32=EPS):
    """bn_save [4, D] (fp32, as a launch stored it) of a training-mode step against the oracle.
    gamma / beta: the fp32 arrays the launch read (None: no affine).  running = (f, rm_old,
    rv_old, rm_new, rv_new) also holds the updated running statistics."""
    N, D = sums["N"], save.shape[1]
    rep = Report()
    for c in range(D):
        g = gamma[c] if gamma is not None else np.float32(1)
        b = beta[c] if beta is not None else np.float32(0)
        ch = O.forward_channel(sums, c, g, b, eps32)
        d_mean, d_var = stat_errors(ch, N, G, acc)
        sb = save_bounds(ch["mean"], ch["var"], d_mean, d_var, g, b, eps32)
        for row, what in enumerate(("mean", "invstd", "alpha", "shift")):
            rep.add(what, c, cols[c], save[row, c], *sb[what])
        if running is not None:
            f, rm_old, rv_old, rm_new, rv_new = running
            rm, rv, unb = O.running(ch["mean"], ch["var"], N, f, rm_old[c], rv_old[c])
            fm = O.mpf(O.frac(f))
            keep_m = abs((1 - fm) * O.mpf(O.frac(rm_old[c])))
            keep_v = abs((1 - fm) * O.mpf(O.frac(rv_old[c])))
            e_rm = fm * d_mean + 4 * U * (abs(fm * O.mpf(ch["mean"])) + keep_m)
            unb = O.mpf(unb)
            e_unb = (d_var * N / (N - 1) if N > 1 else d_var) + 2 * U * unb
            e_rv = fm * e_unb + 4 * U * (abs(fm * unb) + keep_v)
            rm, rv = O.mpf(rm), O.mpf(rv)
            rep.add("rmean", c, cols[c], rm_new[c], rm, V * abs(rm) + e_rm + TINY)
            rep.add("rvar", c, cols[c], rv_new[c], rv, V * abs(rv) + e_rv + TINY)
    return rep


def check_eval(cols, save, gamma, beta, rm, rv, eps32=EPS):
    """bn_save of an eval-mode finish: mean = running_mean bit for bit, the rest from the
    exact running statistics (d_mean = d_var = 0)."""
    rep = Report()
    zero = O.MP.mpf(0)
    for c in range(save.shape[1]):
        g = gamma[c] if gamma is not None else np.float32(1)
        b = beta[c] if beta is not None else np.float32(0)
        sb = save_bounds(O.frac(rm[c]), O.frac(rv[c]), zero, zero, g, b, eps32)
        rep.exact_bits("mean", c, cols[c], save[0, c], rm[c])
        for row, what in ((1, "invstd"), (2, "alpha"), (3, "shift")):
            rep.add(what, c, cols[c], save[row, c], *sb[what])
    return rep


def check_backward(cols, dbn, a1, save, gamma, dgamma, dbeta, coef, G, acc, training=True):
    """dgamma, dbeta [D] and coef [3, D] as a launch stored them, against the oracle on the dbn
    the launch stored, the a1 and the bn_save it read (gamma None: no affine)."""
    N, D = dbn.shape
    sums = O.backward_sums(dbn, a1, save[0], save[1])
    q = O.MP.mpf(G) * O.MP.mpf(2) ** -65 if acc else O.MP.mpf(0)
    rep = Report()
    for c in range(D):
        g = gamma[c] if gamma is not None else np.float32(1)
        sd, sx = O.mpf(sums["sd"][c]), O.mpf(sums["sx"][c])
        SD, SX = O.mpf(sums["SD"][c]), O.mpf(sums["SX"][c])
        d_sd = N * U * SD + q
        d_sx = (2 * V + V * V) * SX + N * U * (1 + 3 * V) * SX + 2 * TINY * SD + q
        if dbeta is not None:
            rep.add("dbeta", c, cols[c], dbeta[c], sd, V * abs(sd) + d_sd + TINY)
        if dgamma is not None:
            rep.add("dgamma", c, cols[c], dgamma[c], sx, V * abs(sx) + d_sx + TINY)
        c1, c2, c3 = O.coef(sums, c, g, save[1, c], N, training)
        rep.exact_bits("c1", c, cols[c], coef[0, c], O.fl32(c1))
        if training:
            a1c, c2, c3 = abs(O.mpf(c1)), O.mpf(c2), O.mpf(c3)
            rep.add("c2", c, cols[c], coef[1, c], c2,
                    V * abs(c2) + a1c * d_sx / N + 2 * U * abs(c2) + TINY)
            rep.add("c3", c, cols[c], coef[2, c], c3,
                    V * abs(c3) + a1c * d_sd / N + 2 * U * abs(c3) + TINY)
        else:
            rep.exact_bits("c2", c, cols[c], coef[1, c], np.float32(0))
            rep.exact_bits("c3", c, cols[c], coef[2, c], np.float32(0))
    return rep


def bits(a):
    """uint32 patterns of an fp32 array, -0 folded into +0."""
    return (np.ascontiguousarray(a, dtype=np.float32) + np.float32(0)).view(np.uint32)


def y_reference(a1, save):
    """relu(fl32(fl32(a1 * alpha32) + shift32)): bn_apply's mul then add, no contraction."""
    t = a1 * save[2][None, :]
    t = t + save[3][None, :]
    return np.where(t > 0, t, np.float32(0)).astype(np.float32)


def da1_reference(dbn, a1, save, coef):
    """The fp32 sequence of transform<PRO_DA1>: c1 dbn + c2 ((a1 - mean) invstd) + c3."""
    xh = (a1 - save[0][None, :]) * save[1][None, :]
    return (coef[0][None, :] * dbn + coef[1][None, :] * xh) + coef[2][None, :]
