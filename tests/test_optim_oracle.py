"""CPU: the optimizer oracles (tests/optim_oracle.py) and the conditions of the cases
(tests/optim_cases.py) that tests/test_gpu_optim_rows.py holds csrc/gine_optim.hip to.

Oracle A (the fp32 restatement) against oracle B (exact arithmetic) at B's derived bounds; the
boundary margin of every double-precision scalar of every case; the fp64 restatement of the
norm against exact sums; oracle A against torch.optim.AdamW on the CPU, with torch's scalars
(equal up to contracted multiply-adds) and with the kernel's (the documented departure);
optim.lr_at against the exact schedule."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import optim_cases as C
import optim_oracle as O

F32 = np.float32


def ulp32(x):
    return float(np.spacing(F32(abs(float(x)))))


# -- the oracle's own arithmetic ----------------------------------------------------------
def test_numpy_fp32_keeps_subnormals_and_fl32_rounds_like_ieee():
    tiny = F32(2.0 ** -149)
    assert tiny * F32(1) == tiny and tiny + tiny == F32(2.0 ** -148) and tiny > 0
    assert F32(1e-30) * F32(1e-30) == 0 and F32(3e-23) * F32(3e-23) > 0     # gradual underflow
    assert np.sqrt(F32(1e-40)) * np.sqrt(F32(1e-40)) > 0
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.standard_normal(200) * np.exp2(rng.uniform(-160, 130, 200)),
                         [0.1, 1.0, 2.0 ** -126, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149,
                          3.4028235e38, 3.4028236e38, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24,
                          1.0 + 2.0 ** -24 + 2.0 ** -50, -(1.0 - 2.0 ** -25)]])
    for x in xs:
        with np.errstate(over="ignore", under="ignore"):
            want = F32(x)                  # a double rounds to fp32 correctly, ties to even
        got, margin = O.fl32(float(x))
        assert got.tobytes() == want.tobytes(), x
        assert margin >= 0
    assert O.fl32(1.0 + 2.0 ** -24)[1] == 0.0                     # a tie: on the boundary
    assert O.fl32(Fraction(1, 3))[0] == F32(1 / 3)
    assert O.fl32(O.MP.mpf(1) / 3)[0] == F32(1 / 3)
    assert 0.24 < O.fl32(1.0)[1] * 2 ** 24 <= 0.5                  # half an ulp from both


def test_scalars_are_the_kernel_text():
    sc = O.scalars(1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    lr, b1, b2, wd = (float(F32(x)) for x in (1e-3, 0.9, 0.999, 0.01))
    # t = 1: every double expression of the kernel is a handful of exact-enough operations
    assert sc["decay"] == F32(1.0 - lr * wd)
    assert sc["nss"] == F32(-(lr / (1.0 - b1)))
    assert sc["bc2"] == F32(math.sqrt(1.0 - b2))
    assert sc["w1"] == F32(1) - F32(0.9) and sc["w2"] == F32(1) - F32(0.999)
    assert sc["beta2"] == F32(0.999) and sc["eps"] == F32(1e-8)
    # past the point where beta^t underflows in double: the corrections are exactly 1
    late = O.scalars(1e-3, 0.9, 0.999, 1e-8, 0.01, 2 ** 24)
    assert late["bc2"] == 1 and late["nss"] == -F32(1e-3)


def test_the_documented_departure_from_torch():
    """DESIGN.md 6d states these figures; they are facts of the two scalar formations."""
    k = O.scalars(1e-3, *C.DEFAULT, 1)
    t = O.torch_scalars(1e-3, *C.DEFAULT, 1)
    assert float(k["w1"]) == pytest.approx(0.100000024, rel=1e-8) and t["w1"] == F32(0.1)
    assert float(k["w2"]) == pytest.approx(0.00099998713, rel=1e-8) and t["w2"] == F32(0.001)
    d1 = float(O.frac(k["w1"]) / O.frac(t["w1"]) - 1)
    d2 = float(O.frac(k["w2"]) / O.frac(t["w2"]) - 1)
    print(f"w1 departure {d1:.4e}  w2 departure {d2:.4e}")
    assert d1 == pytest.approx(2.2e-7, rel=0.03) and d2 == pytest.approx(-1.29e-5, rel=0.005)
    # the bias corrections come from the fp32 betas too: the step size and sqrt(1 - beta2^t)
    # depart as well (t = 1), the latter by half the departure of w2, so that v / bc2^2 keeps it
    dn = float(O.frac(k["nss"]) / O.frac(t["nss"]) - 1)
    db = float(O.frac(k["bc2"]) / O.frac(t["bc2"]) - 1)
    print(f"step size departure {dn:.4e}  sqrt(bias_correction2) departure {db:.4e}")
    assert dn == pytest.approx(-1.9e-7, rel=0.03) and db == pytest.approx(-6.4e-6, rel=0.01)
    for key in ("decay", "beta2", "eps"):                          # the other three agree
        assert k[key] == t[key], key
    # the kernel's choice is the self-consistent one: a constant gradient keeps
    # v / (1 - beta2^t) at g^2 (w2 = 1 - beta2 exactly), torch's misses it by the departure
    b2 = O.frac(k["beta2"])
    assert O.frac(k["w2"]) == 1 - b2 and O.frac(t["w2"]) != 1 - b2


# -- the boundary margins -----------------------------------------------------------------
def test_every_scalar_of_every_case_is_clear_of_a_rounding_boundary():
    worst = (math.inf, None)
    seen = set()
    for combo in C.COMBOS:
        for preset in C.PRESETS:
            count = F32(preset)
            for _ in range(2):                                     # run_a takes two steps
                count = count + F32(1)
                seen.add((combo, int(count)))
    seen |= {(C.MAIN, t) for t in range(1, C.TRAJ_STEPS + 1)}
    for combo, t in sorted(seen, key=lambda x: (x[0][0], x[1])):
        margin = C.scalars(combo, t)["margin"]
        worst = min(worst, (margin, (combo[0], t)))
        assert margin >= O.MARGIN, (combo[0], t, margin)
    print(f"AdamW scalars: {len(seen)} (combo, t), smallest margin 2^{math.log2(worst[0]):.1f} "
          f"at {worst[1]}")
    assert {t for _, t in seen} >= {1, 2, 10, 1000, 100_000, 2 ** 24 - 1, 2 ** 24}


def test_every_scheduled_rate_is_clear_of_a_rounding_boundary():
    worst = (math.inf, None)
    cases = C.schedule_cases()
    for kind, wtr, t in cases:
        lr, margin = C.lr_t(kind, wtr, t)
        assert margin >= O.MARGIN, (kind, wtr, t, margin)
        step = C.scalars(C.MAIN, t, lr)["margin"]                  # the step taken at lr_t
        assert step >= O.MARGIN, (kind, wtr, t, step)
        worst = min(worst, (min(margin, step), (kind, wtr, t)))
    print(f"schedule: {len(cases)} cases, smallest margin 2^{math.log2(worst[0]):.1f} at "
          f"{worst[1]}")
    for control in (False, True):
        for s, row in enumerate(C.flat_expected(control)):
            assert row["margin"] >= O.MARGIN, (control, s, row["margin"])
    # every breakpoint is present, and s = 0.5 gives exactly lr (r + (1 - r) / 2)
    for (W, T, r), t in C.S_HALF:
        lr32, r32 = O.frac(F32(C.SCHED_LR)), O.frac(F32(r))
        for kind in (O.COSINE, O.LINEAR):
            assert O.frac(O.lr_exact(C.SCHED_LR, kind, W, T, r, t)) == lr32 * (r32 + (1 - r32) / 2)
    assert C.lr_t(O.COSINE, (0, 0, 0.0), 1)[0] == 0 and C.lr_t(O.LINEAR, (10, 4, 1.0), 11)[0] \
        == F32(C.SCHED_LR)


def test_lr_at_is_within_one_ulp_of_the_exact_schedule():
    from raincast_gnn.optim import Schedule, lr_at
    worst = 0.0
    for kind, (W, T, r), t in C.schedule_cases():
        name = "cosine" if kind == O.COSINE else "linear"
        got = lr_at(Schedule(name, W, T, r), C.SCHED_LR, t)
        want = float(C.lr_t(kind, (W, T, r), t)[0])
        err = abs(got - want) / (ulp32(want) if want else 2.0 ** -149)
        worst = max(worst, err)
        assert err <= 1.0, (name, W, T, r, t, got, want)
    print(f"lr_at: worst {worst:.2f} ulp")
    assert lr_at(None, C.SCHED_LR, 7) == float(F32(C.SCHED_LR))


# -- oracle A against oracle B ------------------------------------------------------------
def _a_against_b(d, sc, idx):
    pa, ma, va = O.step_a(d["p"], d["g"], d["m"], d["v"], sc)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    inside = 0
    for i in idx:
        b = O.step_b(d["p"][i], d["g"][i], d["m"][i], d["v"][i], sc)
        if b is None:
            continue
        inside += 1
        em = abs(O.frac(ma[i]) - b["m"])
        ev = abs(O.frac(va[i]) - b["v"])
        rm, rv = float(em / b["E_m"]), float(ev / b["E_v"])
        rp = 0.0 if b["p"] is None else float(abs(O.mpf(float(pa[i])) - b["p"]) / b["E_p"])
        state = {k: float(d[k][i]) for k in "pgmv"}
        assert rm <= 1 and rv <= 1 and rp <= 1, (state, rm, rv, rp)
        worst = {"m": max(worst["m"], rm), "v": max(worst["v"], rv), "p": max(worst["p"], rp)}
    return worst, inside


def test_oracle_a_is_within_oracle_b_over_the_edge_grid():
    grid = C.edge_grid()
    size = grid["g"].size
    worst, inside = _a_against_b(grid, C.scalars(C.MAIN, 1), range(size))
    print(f"A against B, edge grid at {C.MAIN[0]} t=1: {inside} of {size} elements inside the "
          f"model, worst |A - B| / bound m {worst['m']:.3f} v {worst['v']:.3f} p {worst['p']:.3f}")
    assert inside == size - 275 - 100              # out: v = inf, and g = 1e21 at a finite v
    k = 0
    for combo in C.COMBOS:
        for preset in C.PRESETS:
            if (combo, preset) == (C.MAIN, 0):
                continue
            k += 1
            idx = range(k % 29, size, 29)                          # 47 elements of each pair
            w, _ = _a_against_b(grid, C.scalars(combo, C.t_of(preset)), idx)
            worst = {q: max(worst[q], w[q]) for q in worst}
    print(f"A against B, every (combo, preset): worst ratio m {worst['m']:.3f} "
          f"v {worst['v']:.3f} p {worst['p']:.3f}")


def test_oracle_a_is_within_oracle_b_on_random_states_and_along_the_trajectory():
    d = C.data(C.SIZES[9], 3)
    idx = range(2 * 1375, 2 * 1375 + 300)                          # the random stretch
    worst, inside = _a_against_b(d, C.scalars(C.COMBOS[3], 10), idx)
    assert inside == 300
    tr, traj = C.trajectory(), C.trajectory_a()
    for k in (1, 7, 19):
        p, m, v = traj[k - 1]
        state = {"p": p, "g": tr["grads"][k], "m": m, "v": v}
        w, n_in = _a_against_b(state, C.scalars(C.MAIN, k + 1), range(k, C.TRAJ_N, 97))
        assert n_in == len(range(k, C.TRAJ_N, 97))
        worst = {q: max(worst[q], w[q]) for q in worst}
    print(f"A against B, random and trajectory states: worst ratio m {worst['m']:.3f} "
          f"v {worst['v']:.3f} p {worst['p']:.3f}")


# -- the pinned states --------------------------------------------------------------------
def _one(p, g, m, v, sc):
    out = O.step_a(*(np.array([x], dtype=np.float32) for x in (p, g, m, v)), sc)
    return tuple(x[0] for x in out)


def test_pinned_states_of_oracle_a():
    sc = C.scalars(C.MAIN, 1)
    # v = 0, g = 0: den = eps, m / eps is finite, and with m = 0 the update is exactly 0
    for g in (0.0, -0.0):
        p, m, v = _one(1.0, g, 0.0, 0.0, sc)
        assert p == sc["decay"] and m == 0 and v == 0
        p, m, v = _one(1.0, g, 1.0, 0.0, sc)                       # den = eps exactly
        assert m == F32(1) + sc["w1"] * (F32(g) - F32(1)) and v == 0
        assert p == sc["decay"] + sc["nss"] * (m / sc["eps"])
    # v = inf: den = inf, the update is 0 and v stays inf, whatever m and g are
    for g, m0 in ((0.0, 1.0), (1.0, -1.0), (1e15, 1e-20), (1e21, 0.0)):
        p, m, v = _one(1.0, g, m0, np.inf, sc)
        assert p == sc["decay"] and np.isinf(v) and v > 0 and np.isfinite(m)
    # (w2 g) g overflows: v becomes inf from a finite state, the update is 0
    p, m, v = _one(1.0, 1e21, 0.0, 1.0, sc)
    assert np.isinf(v) and p == sc["decay"]
    # g^2 underflows: v keeps beta2 v, nothing is lost but the square
    p, m, v = _one(1.0, 1e-30, 0.0, 1.0, sc)
    assert v == sc["beta2"]
    # eps = 0 at v = 0, g = 0, m = 0: 0 / 0, NaN as in torch
    zero = O.scalars(1e-3, 0.9, 0.999, 0.0, 0.01, 1)
    p, m, v = _one(0.0, 0.0, 0.0, 0.0, zero)
    assert np.isnan(p) and m == 0 and v == 0
    q = torch.nn.Parameter(torch.zeros(4))
    opt = torch.optim.AdamW([q], lr=1e-3, eps=0.0, foreach=False)
    q.grad = torch.zeros(4)
    opt.step()
    assert bool(torch.isnan(q).all())
    # step[0] = 2^24: t = 2^24 again, the count cannot advance
    assert C.t_of(2 ** 24) == 2 ** 24 == C.t_of(2 ** 24 - 1)
    assert F32(2 ** 24) + F32(1) == F32(2 ** 24)


def test_the_edge_grid_holds_every_state_and_reaches_every_size():
    grid = C.edge_grid()
    assert grid["g"].size == 1375 and len(set(grid["state"])) == len(C.G_STATES)
    assert np.isinf(grid["v"]).sum() == 275 and (grid["v"] == 0).sum() == 275
    sub = (np.abs(grid["p"]) > 0) & (np.abs(grid["p"]) < 2.0 ** -126)
    assert sub.sum() == 275 and np.signbit(grid["p"][grid["p"] == 0]).sum() == 275
    anti = grid["state"] == C.G_STATES.index("anti")
    big = anti & (grid["m"] != 0)
    assert (np.sign(grid["g"][big]) == -np.sign(grid["m"][big])).all()
    assert (np.abs(grid["g"][big]) > np.abs(grid["m"][big])).all()
    for n in C.SIZES:
        d = C.data(n, 1)
        assert all(d[k].size == n and d[k].dtype == np.float32 for k in "pgmv")
        if n >= 2 * 1375 and n <= C.FULL_GRID_MAX:
            assert np.isinf(d["v"][:1375]).sum() == 275 and np.isinf(d["v"][-1375:]).sum() == 275
        if n > C.FULL_GRID_MAX:
            at = C.last_workgroup_start(n)
            assert at + C.PLANT <= n and at == (O.num_blocks(n) - 1) * 1024
    assert C.last_workgroup_start(600_000) == 511 * 1024
    tr = C.trajectory()
    a = np.abs(tr["grads"])
    assert a.min() >= 2.0 ** -40 and a.max() <= 2.0 ** 40
    assert a.min() < 2.0 ** -39 and a.max() > 2.0 ** 39            # the span is used


def test_subtly_wrong_kernels_would_change_bits_of_the_cases():
    """What the bit comparison on the device can see: each mutant of the definition moves
    bits of oracle A on the cases themselves, in the quantity it touches."""
    d = C.data(C.SIZES[9], 0)
    p, g, m, v = d["p"], d["g"], d["m"], d["v"]

    def mutant(name, sc):
        sc = dict(sc)
        with np.errstate(all="ignore"):
            if name == "torch w2":
                sc["w2"] = F32(0.001)
            elif name == "torch w1":
                sc["w1"] = F32(0.1)
            elif name == "bias_correction2 of step t - 1":
                sc["bc2"] = C.scalars(C.MAIN, 9)["bc2"]
            if name in ("torch w2", "torch w1", "bias_correction2 of step t - 1"):
                return O.step_a(p, g, m, v, sc)
            p1 = p * sc["decay"]
            m1 = m + sc["w1"] * (g - m)
            vb = v * sc["beta2"]
            if name == "contracted v":        # fma((w2 g), g, v beta2): one rounding fewer
                v1 = (vb.astype(np.float64) + (sc["w2"] * g).astype(np.float64) * g) \
                    .astype(np.float32)
            elif name == "w2 (g g)":
                v1 = vb + sc["w2"] * (g * g)
            elif name == "v without beta2":
                v1 = v + (sc["w2"] * g) * g
            else:
                v1 = vb + (sc["w2"] * g) * g
            if name == "eps inside the quotient":
                den = (np.sqrt(v1) + sc["eps"]) / sc["bc2"]
            elif name == "eps under the root":
                den = np.sqrt(v1 + sc["eps"]) / sc["bc2"]
            else:
                den = np.sqrt(v1) / sc["bc2"] + sc["eps"]
            if name == "contracted p":        # fma(nss, m / den, p decay)
                p1 = (p1.astype(np.float64) + float(sc["nss"]) * (m1 / den).astype(np.float64)) \
                    .astype(np.float32)
            elif name == "nss m / den":
                p1 = p1 + (sc["nss"] * m1) / den
            else:
                p1 = p1 + sc["nss"] * (m1 / den)
        return p1, m1, v1

    sc = C.scalars(C.MAIN, 10)
    want = O.step_a(p, g, m, v, sc)
    touched = {"torch w2": 2, "torch w1": 1, "bias_correction2 of step t - 1": 0,
               "contracted v": 2, "w2 (g g)": 2, "v without beta2": 2,
               "eps inside the quotient": 0, "eps under the root": 0, "contracted p": 0,
               "nss m / den": 0}
    for name, which in touched.items():
        got = mutant(name, sc)
        moved = C.mismatches(got[which], want[which]).size
        print(f"mutant {name}: {moved} of {p.size} {('param', 'exp_avg', 'exp_avg_sq')[which]} "
              "values move")
        assert moved >= 10, name
    same = mutant("none", sc)
    assert all(C.mismatches(a, b).size == 0 for a, b in zip(same, want))


# -- the norm -----------------------------------------------------------------------------
def _block_of(n):
    """The workgroup that takes each element (the documented order)."""
    threads = O.num_blocks(n) * 256
    e = np.arange(n)
    block = ((e // 4) % threads) // 256
    block[4 * (n // 4):] = 0                                       # the tail: the first threads
    return block


@pytest.mark.parametrize("n", [1, 5, 1025, 9 * 1024 + 1, 512 * 1024 + 4])
def test_partial_restatement_agrees_with_exact_sums_to_fp64_rounding(n):
    """A partial is a sum of non-negative exact squares through a chain of at most
    4 trips + 1 (the thread) + 6 (the butterfly) + 3 (the waves) fp64 additions."""
    g = C.wide_grad(n)
    part = O.sumsq_partials(g)
    blocks = O.num_blocks(n)
    assert part.shape == (blocks, 2) and (part[:, 1] == 0).all()
    threads = blocks * 256
    depth = 4 * max(-(-(n // 4) // threads), 1) + 1 + 6 + 3
    u64 = Fraction(1, 2 ** 53)
    bound = depth * u64 / (1 - depth * u64)
    block = _block_of(n)
    which = range(blocks) if blocks <= 10 else (0, 1, 73, 74, 510, 511)
    worst = 0.0
    for b in which:
        exact = O.sumsq_exact(g[block == b])
        err = abs(Fraction(float(part[b, 0])) - exact)
        assert err <= bound * exact, (n, b)
        worst = max(worst, float(err / (bound * exact)) if exact else 0.0)
    # the order shows in the bits: the index-order fp64 sum of the same squares differs
    if n >= 1025:
        sq = g.astype(np.float64) ** 2
        plain = np.array([sq[block == b].sum() for b in which])
        assert (plain != part[list(which), 0]).any()
    # the norm: fp32 of the fp64 root of the index-order sum, within 1 fp32 ulp of exact
    norm = O.norm_f32(part)
    exact = O.norm_exact(g)
    assert abs(O.mpf(float(norm)) - exact) <= ulp32(norm)
    print(f"n={n}: worst partial error / bound {worst:.3f}, norm {float(norm)!r}")


def test_nonfinite_counts_and_the_clip_coefficient():
    n = 9 * 1024 + 1
    g = C.unit_grad(n).copy()
    g[[0, 4100, n - 1]] = [np.inf, np.nan, -np.inf]
    part = O.sumsq_partials(g)
    block = _block_of(n)
    want = np.zeros(O.num_blocks(n))
    for i in (0, 4100, n - 1):
        want[block[i]] += 1
    assert (part[:, 1] == want).all() and part[:, 1].sum() == 3
    assert not np.isfinite(O.norm_f32(part))
    # the coefficient
    assert O.clip_coef(0.0, 5.0) == 1 and O.clip_coef(np.inf, 5.0) == 1
    assert O.clip_coef(1.0, 0.0) == 1                              # all-zero gradient: 1 / 1e-6
    norm = O.norm_f32(O.sumsq_partials(C.unit_grad(n)))
    assert 0.9 < norm < 1.1
    coef = O.clip_coef(norm, norm)                                 # norm == max_norm
    assert coef < 1 and coef == norm / (norm + F32(1e-6)) and 1 - float(coef) < 2e-6
    assert 0 < O.clip_coef(1e-30, norm) < 2e-30
    big = C.unit_grad(n).copy()
    big[[3, 5000, n - 2]] = 3e38                                   # finite, the norm is not
    pb = O.sumsq_partials(big)
    assert pb[:, 1].sum() == 0 and np.isfinite(pb[:, 0]).all() and np.isinf(O.norm_f32(pb))
    assert O.clip_coef(1.0, O.norm_f32(pb)) == 0


# -- torch on the CPU ---------------------------------------------------------------------
def test_oracle_a_with_torch_scalars_is_torch_up_to_contracted_multiply_adds():
    """One step at a time from torch's own state, so nothing compounds; torch's CPU kernels
    fuse multiply-adds and are no bit target (optim_cases.fma_bounds)."""
    _, lr, b1, b2, eps, wd = C.MAIN
    tr = C.trajectory()
    q = torch.nn.Parameter(torch.from_numpy(tr["p0"].copy()))
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    worst = {"m": 0.0, "v": 0.0}
    differ = 0
    m0 = v0 = np.zeros(C.TRAJ_N, np.float32)
    for k in range(7):
        p0 = q.detach().numpy().copy()
        g = tr["grads"][k]
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[q]
        assert float(st["step"]) == k + 1
        sc = O.torch_scalars(lr, b1, b2, eps, wd, k + 1)
        _, ma, va = O.step_a(p0, g, m0, v0, sc)
        mt, vt = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        bm, bv = C.fma_bounds(p0, g, m0, v0, sc)
        em = np.abs(ma.astype(np.float64) - mt)
        ev = np.abs(va.astype(np.float64) - vt)
        assert (em <= bm).all() and (ev <= bv).all(), k
        worst["m"] = max(worst["m"], float((em / bm).max()))
        worst["v"] = max(worst["v"], float((ev / bv).max()))
        differ += int((va != vt).sum())
        m0, v0 = mt, vt
    print(f"A with torch's scalars against torch: worst error / bound m {worst['m']:.3f} "
          f"v {worst['v']:.3f}; {differ} of {7 * C.TRAJ_N} exp_avg_sq values differ in bits")


def test_oracle_a_with_the_kernel_scalars_departs_from_torch_as_documented():
    pt, mt, vt = C.torch_trajectory(steps=7)
    _, ma, va = C.trajectory_a()[6]
    rel = va.astype(np.float64) / vt.astype(np.float64) - 1
    k = O.scalars(1e-3, *C.DEFAULT, 1)
    t = O.torch_scalars(1e-3, *C.DEFAULT, 1)
    dep = float(O.frac(k["w2"]) / O.frac(t["w2"]) - 1)
    slack = 2 * float(O.G(2 * 7 + 2))
    print(f"exp_avg_sq after 7 steps, kernel scalars / torch - 1: {rel.min():.4e} .. "
          f"{rel.max():.4e} (analytic {dep:.4e}, rounding {slack:.2e})")
    assert (np.abs(rel - dep) <= slack).all()
    assert (np.abs(rel) > 1.0e-5).all()                            # at every element


def test_trajectory_tie_bounds_hold_for_oracle_a():
    """The bound the GPU test holds the kernel to, held here by oracle A."""
    pt, mt, vt = C.torch_trajectory()
    pa, ma, va = C.trajectory_a()[-1]
    b = C.tie_bounds()
    rel_v = np.abs(va.astype(np.float64) - vt) / vt
    err_m = np.abs(ma.astype(np.float64) - mt)
    err_p = np.abs(pa.astype(np.float64) - pt).max() / np.abs(pt).max()
    print(f"tie to torch after {C.TRAJ_STEPS} steps: v rel {rel_v.max():.4e} (bound "
          f"{b['v_rel']:.4e}), m err / bound {float((err_m / b['m_abs']).max()):.3f}, "
          f"p rel_err {err_p:.3e}")
    assert b["dep_v"] == pytest.approx(1.29e-5, rel=0.005)
    assert (rel_v <= b["v_rel"]).all() and (err_m <= b["m_abs"]).all() and err_p <= 2e-6
