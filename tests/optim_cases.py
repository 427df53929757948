"""Seeded inputs, the edge grid and the shared checks of the optimizer tests, used by the CPU
tests (tests/test_optim_oracle.py: the oracles against each other and against torch) and the
GPU tests (tests/test_gpu_optim_rows.py: the kernels of csrc/gine_optim.hip) with
tests/optim_oracle.py.

Sizes (SIZES): the smallest n at which each branch of the grid min(512, ceil(ceil(n/4)/256)) x
256 threads x one float4 first appears: 1, 2, 3 (tail only), 4, 5 (one float4, then a tail),
1023, 1024, 1025 (one workgroup full, then spilling), 8 x 1024 (exactly 8 workgroups: one per
sub-ticket), 9 x 1024 + 1 (the first ragged ticket group), 512 x 1024 (the capped grid, one
trip), + 1 (a tail only), + 4 (one float4 on the second trip), 600,000.

Element states (edge_grid): planted and fully crossed, 11 x 5 x 5 x 5 = 1,375 elements:
  g  +0, -0, 2^-149, 1e-30 (g^2 underflows), +-1e-8 (sqrt(v) about eps), +-1, 1e15, 1e21
     ((w2 g) g overflows to inf), and "anti": -m moved one ulp away from 0 (g - m cancels to
     about -2 m; for m = 0 the smallest subnormal)
  v  0, 1e-40 (subnormal), 1e-16, 1, inf          p  +0, -0, 1e-40 (subnormal), 1, 1e30
  m  0, +-1e-20, +-1
data(n, seed): up to FULL_GRID_MAX = 9 x 1024 + 1 the permuted grid from index 0 (rotated by
the seed) and again ending at n - 1 once n >= 2 x 1,375, seeded random values between (g of
scale s = 2^-20 to 2^20, m about 0.3 s, v = s^2 2^-24..2^1, p of scale 2^-14 to 2^2, so that
w2 g^2 runs from far below v beta2 to far above it, the update from far below p to above it,
and every rounding reaches the result's bits); above, random values with PLANT = 40 grid
elements at index 0, ending at n - 1, and at the start of the last workgroup's first-trip range.

Step counts: PRESETS are values of step[0] ahead of the launch; t = f32(step[0] + 1f) is 1, 2,
10, 1000, 1e5, 2^24 - 1, 2^24 and, from step[0] = 2^24, 2^24 again: the fp32 counter no longer
advances there (2^24 + 1f == 2^24), the update is applied with t = 2^24 and the count stays.

Hyper-parameters (COMBOS): the defaults (0.9, 0.999, 1e-8, 0.01) at lr 1e-4, 1e-3 and 3e-3, a
non-default set (0.8, 0.99, 1e-6, 0.1) and the defaults with weight_decay = 0.  Small sizes take
every (combo, preset) pair; the four sizes from 512 x 1024 take every combo at step[0] = 0 and
every preset at the default combo (pairs()).

Trajectory: TRAJ_STEPS = 20 consecutive steps at TRAJ_N = 9 x 1024 + 1 from m = v = 0; three
quarters of the elements keep a magnitude 2^e, e uniform in [-40, 40], the rest redraw it every
step, |g| in [2^-40, 2^40] throughout.

The tie to torch (tie_bounds): after the trajectory, the kernel's p, m, v against
torch.optim.AdamW(foreach=False) on the CPU on the same gradients.  Both start at m = v = 0,
so in exact arithmetic
  v_T = sum_k w2 beta2^(T-k) g_k^2:  v_kernel / v_torch = w2_kernel / w2_torch, the analytic
        departure |w2_k / w2_t - 1| (1.29e-5 at the defaults); every term is non-negative, so
        rounding adds at most (1 + U)^(2 (T - k) + 4) - 1 <= G(2 T + 2) relative per evaluation
        (two roundings per later step on an older term), twice for the two evaluations:
        |v_k - v_t| <= (|w2_k / w2_t - 1| + 2 G(2 T + 2)) v_t
  m_T = sum_k w (1 - w)^(T-k) g_k with w = w1: d log(term_k) / d log w = 1 - w (T - k) / (1 - w),
        in magnitude at most 1 + w T / (1 - w); with M = sum_k w (1 - w)^(T-k) |g_k| the
        scalar part is |w1_k / w1_t - 1| (1 + w T / (1 - w)) M (1 + 1e-3) (the last factor:
        second order).  Rounding: a step adds at most e_k = G(3) (|m_{k-1}| + w |g_k - m_{k-1}|)
        (oracle B's E_m; values from oracle A's trajectory in fp64) and the recurrence carries
        an earlier error on with the factor 1 - w: E_T = sum_k (1 - w)^(T-k) e_k, once per
        evaluation: |m_k - m_t| <= scalar part + 2.02 E_T   (1 %: second order).
  p stays at the project's bar, rel_err <= 2e-6 (tests/test_gpu_training.py).
None of it is fitted: the figures come from the scalars and the operation count, and they are
measured against torch's CPU result.

The fused-multiply-add bound (fma_bounds): torch's CPU kernels may contract a multiply into
the following add.  Two evaluations of the same real expression with at most k roundings each
differ by at most 2 G(k) times the operand terms: 2 G(3) (|m| + w1 |g - m|) for m and
2 G(4) (v beta2 + w2 g^2) for v, one step from a common state.
"""
import functools

import numpy as np

import optim_oracle as O

F32 = np.float32
SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 8 * 1024, 9 * 1024 + 1, 512 * 1024, 512 * 1024 + 1,
         512 * 1024 + 4, 600_000)
FULL_GRID_MAX = 9 * 1024 + 1
PLANT = 40
PRESETS = (0, 1, 9, 999, 99_999, 2 ** 24 - 2, 2 ** 24 - 1, 2 ** 24)
DEFAULT = (0.9, 0.999, 1e-8, 0.01)
# (name, lr, beta1, beta2, eps, weight_decay)
COMBOS = (("default-1e-4", 1e-4) + DEFAULT, ("default-1e-3", 1e-3) + DEFAULT,
          ("default-3e-3", 3e-3) + DEFAULT, ("alt", 1e-3, 0.8, 0.99, 1e-6, 0.1),
          ("nowd", 1e-3, 0.9, 0.999, 1e-8, 0.0))
MAIN = COMBOS[1]
TRAJ_N, TRAJ_STEPS = 9 * 1024 + 1, 20

SUB = F32(2.0 ** -149)
G_STATES = ("+0", "-0", "sub", "1e-30", "1e-8", "-1e-8", "1", "-1", "1e15", "1e21", "anti")
V_STATES = (0.0, 1e-40, 1e-16, 1.0, np.inf)
P_STATES = (0.0, -0.0, 1e-40, 1.0, 1e30)
M_STATES = (0.0, 1e-20, -1e-20, 1.0, -1.0)
_G_VALUES = {"+0": 0.0, "-0": -0.0, "sub": float(SUB), "1e-30": 1e-30, "1e-8": 1e-8,
             "-1e-8": -1e-8, "1": 1.0, "-1": -1.0, "1e15": 1e15, "1e21": 1e21}

# schedules: (W, T, r) and the steps around every breakpoint, plus s = 0.5 exactly
SCHEDULES = ((3, 8, 0.1), (0, 8, 0.0), (8, 8, 0.5), (10, 4, 1.0), (0, 0, 0.0),
             (1000, 100_000, 0.01))
S_HALF = (((0, 8, 0.0), 4), ((1000, 100_000, 0.01), 50_500))
SCHED_LR = 3e-3


def t_of(preset):
    """The step number the kernel uses from step[0] = preset: f32(preset + 1f)."""
    return int(F32(preset) + F32(1))


def pairs(n):
    """The (combo, preset) pairs run at size n."""
    if n < 512 * 1024:
        return [(c, s) for c in COMBOS for s in PRESETS]
    return [(c, 0) for c in COMBOS] + [(MAIN, s) for s in PRESETS[1:]]


def scalars(combo, t, lr=None):
    _, lr0, b1, b2, eps, wd = combo
    return _scalars(lr0 if lr is None else float(lr), b1, b2, eps, wd, t)


@functools.lru_cache(maxsize=None)
def _scalars(lr, b1, b2, eps, wd, t):
    return O.scalars(lr, b1, b2, eps, wd, t)


def _ro(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def edge_grid():
    """The 1,375 crossed element states in a seeded order: p, g, m, v (fp32) and the index of
    each element's g state."""
    p, g, m, v, gs = [], [], [], [], []
    for gi, name in enumerate(G_STATES):
        for vv in V_STATES:
            for pp in P_STATES:
                for mm in M_STATES:
                    mm32 = F32(mm)
                    if name == "anti":
                        gg = -SUB if mm32 == 0 else np.nextafter(-mm32, F32(-np.inf if mm32 > 0
                                                                             else np.inf))
                    else:
                        gg = F32(_G_VALUES[name])
                    p.append(pp), g.append(gg), m.append(mm), v.append(vv), gs.append(gi)
    order = np.random.default_rng(1375).permutation(len(p))
    with np.errstate(over="ignore"):
        out = {k: np.array(x, dtype=np.float32)[order] for k, x in
               (("p", p), ("g", g), ("m", m), ("v", v))}
    out["state"] = np.array(gs)[order]
    return _ro(out)


def _random(n, rng):
    scale = np.exp2(rng.uniform(-20, 20, n))
    return {"p": (np.exp2(rng.uniform(-14, 2, n)) * rng.standard_normal(n)).astype(np.float32),
            "g": (scale * rng.standard_normal(n)).astype(np.float32),
            "m": (0.3 * scale * rng.standard_normal(n)).astype(np.float32),
            "v": (scale * scale * np.exp2(rng.uniform(-24, 1, n))).astype(np.float32)}


def last_workgroup_start(n):
    """First element of the last workgroup's first-trip range."""
    return (O.num_blocks(n) - 1) * 1024


@functools.lru_cache(maxsize=None)
def data(n, seed=0):
    """Read-only p, g, m, v (fp32 [n]) of one case."""
    rng = np.random.default_rng([n, seed, 77])
    grid = edge_grid()
    size = grid["g"].size
    out = _random(n, rng)

    def plant(at, count, rot):
        idx = (np.arange(count) + rot) % size
        for k in "pgmv":
            out[k][at:at + count] = grid[k][idx]

    rot = (97 * seed) % size
    if n <= FULL_GRID_MAX:
        plant(0, min(n, size), rot)
        if n >= 2 * size:
            plant(n - size, size, rot + 11)
    else:
        plant(0, PLANT, rot)
        plant(last_workgroup_start(n), PLANT, rot + PLANT)
        plant(n - PLANT, PLANT, rot + 2 * PLANT)
    return _ro(out)


def run_a(d, combo, preset, steps=2, coef=None, lr=None):
    """Oracle A from step[0] = preset on the case d with its gradient held: [(p, m, v)] after
    each step, and the step counts the device must show."""
    p, m, v = d["p"], d["m"], d["v"]
    out, counts, count = [], [], F32(preset)
    for _ in range(steps):
        count = count + F32(1)
        p, m, v = O.step_a(p, d["g"], m, v, scalars(combo, int(count), lr), coef)
        out.append((p, m, v))
        counts.append(float(count))
    return out, counts


def mismatches(got, want):
    """Indices where two fp32 arrays differ in bits; a NaN on both sides is agreement."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return np.nonzero(~same)[0]


def describe(what, got, want, idx, d=None):
    i = int(idx[0])
    text = (f"{what}: {idx.size} of {got.size} elements differ, first at {i}: got "
            f"{float(got[i])!r} ({got.view(np.uint32)[i]:#010x}) want {float(want[i])!r} "
            f"({want.view(np.uint32)[i]:#010x})")
    if d is not None:
        text += " inputs " + " ".join(f"{k}={float(d[k][i])!r}" for k in "pgmv")
    return text


def assert_bits(what, got, want, d=None):
    idx = mismatches(got, want)
    assert idx.size == 0, describe(what, np.asarray(got), np.asarray(want), idx, d)


# -- the trajectory and the tie to torch --------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory():
    """{"p0": [n], "grads": [TRAJ_STEPS, n]} fp32, read-only."""
    rng = np.random.default_rng([TRAJ_N, TRAJ_STEPS, 5])
    n = TRAJ_N
    e = rng.uniform(-40, 40, n)
    redraw = rng.random(n) < 0.25
    grads = np.empty((TRAJ_STEPS, n), dtype=np.float32)
    for k in range(TRAJ_STEPS):
        ek = np.where(redraw, rng.uniform(-40, 40, n), e)
        mag = np.clip(np.exp2(ek) * rng.uniform(0.5, 1.0, n), 2.0 ** -40, 2.0 ** 40)
        grads[k] = (mag * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    return _ro({"p0": rng.standard_normal(n).astype(np.float32), "grads": grads})


@functools.lru_cache(maxsize=None)
def trajectory_a(combo=MAIN):
    """Oracle A along the trajectory: [(p, m, v)] after each step (read-only arrays)."""
    tr = trajectory()
    p, m, v = tr["p0"], np.zeros(TRAJ_N, np.float32), np.zeros(TRAJ_N, np.float32)
    out = []
    for k in range(TRAJ_STEPS):
        p, m, v = O.step_a(p, tr["grads"][k], m, v, scalars(combo, k + 1))
        for a in (p, m, v):
            a.setflags(write=False)
        out.append((p, m, v))
    return out


def torch_trajectory(combo=MAIN, steps=TRAJ_STEPS):
    """torch.optim.AdamW(foreach=False) on the CPU over the same gradients: (p, m, v) fp32."""
    import torch
    _, lr, b1, b2, eps, wd = combo
    tr = trajectory()
    q = torch.nn.Parameter(torch.from_numpy(tr["p0"].copy()))
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for k in range(steps):
        q.grad = torch.from_numpy(tr["grads"][k].copy())
        opt.step()
    st = opt.state[q]
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def tie_bounds(combo=MAIN):
    """(relative bound on v against torch's v, absolute bound on m [n]) after the trajectory;
    the derivation is in the module docstring."""
    _, lr, b1, b2, eps, wd = combo
    T = TRAJ_STEPS
    k_sc, t_sc = O.scalars(lr, b1, b2, eps, wd, 1), O.torch_scalars(lr, b1, b2, eps, wd, 1)
    dep_v = abs(float(O.frac(k_sc["w2"]) / O.frac(t_sc["w2"]) - 1))
    dep_m = abs(float(O.frac(k_sc["w1"]) / O.frac(t_sc["w1"]) - 1))
    v_rel = dep_v + 2 * float(O.G(2 * T + 2))
    w = float(k_sc["w1"])
    g = trajectory()["grads"].astype(np.float64)
    traj = trajectory_a(combo)
    M = np.zeros(TRAJ_N)
    E = np.zeros(TRAJ_N)
    m_prev = np.zeros(TRAJ_N)
    g3 = float(O.G(3))
    for k in range(T):
        M = (1 - w) * M + w * np.abs(g[k])
        E = (1 - w) * E + g3 * (np.abs(m_prev) + w * np.abs(g[k] - m_prev))
        m_prev = traj[k][1].astype(np.float64)
    m_abs = dep_m * (1 + w * T / (1 - w)) * M * (1 + 1e-3) + 2.02 * E
    return {"v_rel": v_rel, "m_abs": m_abs, "dep_v": dep_v, "dep_m": dep_m}


def fma_bounds(p, g, m, v, sc):
    """Absolute bounds (fp64 arrays) on the m and v of two evaluations of one step that differ
    only in contracted multiply-adds."""
    g, m, v = (np.asarray(x, dtype=np.float64) for x in (g, m, v))
    w1, w2, b2 = float(sc["w1"]), float(sc["w2"]), float(sc["beta2"])
    return (2 * float(O.G(3)) * (np.abs(m) + w1 * np.abs(g - m)),
            2 * float(O.G(4)) * (v * b2 + w2 * g * g))


# -- schedules ----------------------------------------------------------------------------
def schedule_steps(W, T):
    return sorted({t for t in (1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T) if t >= 1})


def schedule_cases():
    """[(kind, (W, T, r), t)] for cosine and linear."""
    out = []
    for kind in (O.COSINE, O.LINEAR):
        for wtr in SCHEDULES:
            out += [(kind, wtr, t) for t in schedule_steps(wtr[0], wtr[1])]
        out += [(kind, wtr, t) for wtr, t in S_HALF]
    return out


@functools.lru_cache(maxsize=None)
def lr_t(kind, wtr, t, lr=SCHED_LR):
    """(fp32 lr_t, boundary margin) of one schedule case."""
    return O.lr_f32(lr, kind, wtr[0], wtr[1], wtr[2], t)


# -- gradients for the norm ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_grad(n):
    """Finite gradient spread over 2^-60 to 2^60, so that the order of the sum shows in the
    bits of every partial."""
    rng = np.random.default_rng([n, 60])
    g = np.exp2(rng.uniform(-60, 60, n)) * rng.uniform(1.0, 2.0, n)
    g = (g * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def unit_grad(n, scale=1.0):
    """Finite gradient of norm about `scale`: randn / sqrt(n)."""
    rng = np.random.default_rng([n, 61])
    g = (scale * rng.standard_normal(n) / np.sqrt(n)).astype(np.float32)
    g.setflags(write=False)
    return g


# -- FlatAdamW end to end -----------------------------------------------------------------
FLAT_SIZES = (1, 63, 64, 65, 4097)
FLAT_STEPS = 10
FLAT_ALIGN = 64                       # FlatAdamW.ALIGN
FLAT_SCHEDULE = ("cosine", 3, 10, 0.1)
FLAT_MAX_NORM = 30.0                  # between the norms of the odd and the even steps


def flat_layout():
    """(offsets, total) of FLAT_SIZES in the flat buffers."""
    offs, off = [], 0
    for k in FLAT_SIZES:
        offs.append(off)
        off = -(-(off + k) // FLAT_ALIGN) * FLAT_ALIGN
    return offs, off


@functools.lru_cache(maxsize=None)
def flat_case():
    """{"p0": [param arrays], "grads": [FLAT_STEPS][param arrays]}: randn gradients, the even
    steps scaled by 1/4 (norm about 16 against about 65: clipped and unclipped steps)."""
    rng = np.random.default_rng([4290, 9])
    p0 = [rng.standard_normal(k).astype(np.float32) for k in FLAT_SIZES]
    grads = [[((1.0 if s % 2 == 0 else 0.25) * rng.standard_normal(k)).astype(np.float32)
              for k in FLAT_SIZES] for s in range(FLAT_STEPS)]
    return {"p0": p0, "grads": grads}


@functools.lru_cache(maxsize=None)
def flat_expected(control):
    """Oracle A over the flat buffers: per step {"p", "m", "v" (flat fp32), "lr", "coef",
    "norm", "margin"}.  control: the cosine FLAT_SCHEDULE and clipping at FLAT_MAX_NORM."""
    offs, total = flat_layout()
    case = flat_case()
    p, m, v = (np.zeros(total, np.float32) for _ in range(3))
    for off, x in zip(offs, case["p0"]):
        p[off:off + x.size] = x
    kind = {"cosine": O.COSINE, "linear": O.LINEAR}[FLAT_SCHEDULE[0]]
    out = []
    for s in range(FLAT_STEPS):
        g = np.zeros(total, np.float32)
        for off, x in zip(offs, case["grads"][s]):
            g[off:off + x.size] = x
        lr, margin, coef, norm = F32(MAIN[1]), np.inf, None, None
        if control:
            lr, margin = O.lr_f32(MAIN[1], kind, *FLAT_SCHEDULE[1:], s + 1)
            norm = O.norm_f32(O.sumsq_partials(g))
            coef = O.clip_coef(FLAT_MAX_NORM, norm)
        sc = scalars(MAIN, s + 1, lr)
        p, m, v = O.step_a(p, g, m, v, sc, coef)
        out.append({"p": p, "m": m, "v": v, "lr": lr, "coef": coef, "norm": norm,
                    "margin": min(margin, sc["margin"])})
    return out
