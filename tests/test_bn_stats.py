"""CPU: the BatchNorm statistics oracle (tests/bn_oracle.py) is anchored to torch in fp64, an
fp64 model of the documented algorithm stays inside every derived bound of tests/bn_cases.py
on every case, and the checker rejects each of nine wrong kernels (mutants of that model).

The model restates csrc/gine_bnacc.hpp and the finish kernels of csrc/gine_mlp.hip in numpy:
32-row tiles dealt to G workgroups, fp64 workgroup sums, on the accumulator path each rounded
to 2^-64, var = s2 / N - mean^2 clamped at 0, fp32 stores; in the backward xhat in fp32 and
its product with dbn in fp64.  It is the proof that a correct implementation attains the
bounds; the GPU tests (tests/test_gpu_bn_stats.py) hold the kernels to the same checker.
"""
import numpy as np
import pytest
import torch

import bn_cases as BC
import bn_oracle as O

F32 = np.float32


def model_grid(N):
    return min(-(-N // 32), 256)


def _wg_sums(terms, G, acc, mut):
    """Column totals of fp64 (fp32 in one mutant) terms [N, D]: per workgroup, then summed."""
    N = terms.shape[0]
    wg = (np.arange(N) // 32) % G
    res = 32 if mut == "lo_dropped" else 64
    tot = np.zeros(terms.shape[1], dtype=terms.dtype)
    for g in range(G):
        s = terms[wg == g].sum(0, dtype=terms.dtype)
        if acc:
            s = np.ldexp(np.rint(np.ldexp(s.astype(np.float64), res)), -res).astype(terms.dtype)
        tot = tot + s
    return tot.astype(np.float64)


def model_forward(c, G, acc, f=float(BC.MOMENTUM), mut=None):
    """bn_save [4, D], new running mean and var (fp32) of one training step of case c."""
    a1, N = c["a1"], c["N"]
    t = a1 if mut == "fp32_sums" else a1.astype(np.float64)
    s1, s2 = _wg_sums(t, G, acc, mut), _wg_sums(t * t, G, acc, mut)
    if mut == "b1_leak":
        b = c["b1"].astype(np.float64)
        s1, s2 = s1 + b, s2 + b * b
    n = float(32 * -(-N // 32)) if mut == "n_rounded_up" else float(N)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + float(BC.EPS))
    alpha = c["gamma"].astype(np.float64) * invstd
    shift = c["beta"].astype(np.float64) - mean * alpha
    unb = var if (N == 1 or mut == "biased_running") else var * n / (n - 1.0)
    k = 1.0 - f if mut == "momentum_flipped" else f
    rm = k * mean + (1.0 - k) * c["rm"].astype(np.float64)
    rv = k * unb + (1.0 - k) * c["rv"].astype(np.float64)
    return np.stack([mean, invstd, alpha, shift]).astype(F32), rm.astype(F32), rv.astype(F32)


def model_backward(c, save, G, acc, mut=None, training=True):
    """The dbn a launch would store (dy behind the ReLU mask of bn_apply) and dgamma, dbeta,
    coef [3, D] (fp32)."""
    a1, N = c["a1"], c["N"]
    dbn = np.where(BC.y_reference(a1, save) > 0, c["dy"], F32(0)).astype(F32)
    xh = (a1 - save[0][None, :]) * save[1][None, :]                 # fp32, two roundings
    d64 = dbn.astype(np.float64)
    sd, sx = _wg_sums(d64, G, acc, mut), _wg_sums(d64 * xh.astype(np.float64), G, acc, mut)
    g = c["gamma"].astype(np.float64)
    c1 = g * save[1].astype(np.float64)
    if mut == "c1_from_alpha":
        c1 = save[2].astype(np.float64)
    a, b = (sd, sx) if mut == "sx_sd_swapped" else (sx, sd)
    c2 = (c1 if mut == "c2_sign" else -c1) * a / N
    c3 = -c1 * b / N
    if not training:
        c2, c3 = np.zeros_like(c2), np.zeros_like(c3)
    return dbn, sx.astype(F32), sd.astype(F32), np.stack([c1, c2, c3]).astype(F32)


def check_model(N, D, acc, mut=None):
    """Both reports of the model (or a mutant) on case (N, D)."""
    c, G = BC.case(N, D), model_grid(N)
    f = float(BC.MOMENTUM)
    save, rm, rv = model_forward(c, G, acc, f, mut)
    fwd = BC.check_forward(BC.forward_sums(N, D), c["cols"], save, c["gamma"], c["beta"], G, acc,
                           running=(f, c["rm"], c["rv"], rm, rv))
    dbn, dgamma, dbeta, coef = model_backward(c, save, G, acc, mut)
    bwd = BC.check_backward(c["cols"], dbn, c["a1"], save, c["gamma"], dgamma, dbeta, coef, G,
                            acc)
    return fwd, bwd


def test_case_table():
    for D in BC.DIMS:
        cols = BC.columns(D)
        assert {a for a, _ in cols} == set(BC.A1_CLASSES)
        assert {d for _, d in cols} == set(BC.DBN_CLASSES)
    assert len(set(BC.columns(128))) == 108 and len(set(BC.PAIRS)) >= 32
    c = BC.case(33, 128)
    assert int((c["gamma"] < 0).sum()) == 2
    nobias = np.array([a in BC.NO_BIAS for a, _ in c["cols"]])
    assert (c["b1"][~nobias] >= 0.25).all() and (c["b1"][~nobias] <= 0.75).all()
    assert (c["b1"][nobias] == 0).all() and nobias.sum() == 18
    assert all(np.isfinite(c[k]).all() for k in ("z", "a1", "dy"))


def test_column_dots_is_exact():
    """Against fractions.Fraction term by term, on a column that spans fp32's whole range."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((97, 3)) * 10.0 ** rng.uniform(-44, 38, (97, 3))).astype(F32)
    y = (rng.standard_normal((97, 3)) * 10.0 ** rng.uniform(-30, 0, (97, 3))).astype(F32)
    x[5, 0] = F32(1e-45)    # a subnormal
    for c in range(3):
        assert O.column_dots(x)[c] == sum(Fraction(float(t)) for t in x[:, c])
        assert O.column_dots(x, y)[c] == sum(Fraction(float(s)) * Fraction(float(t))
                                             for s, t in zip(x[:, c], y[:, c]))


@pytest.mark.parametrize("N", [33, 1031])
def test_oracle_anchored_to_torch_fp64(N):
    """A sanity anchor of the oracle (1e-12 relative), not a bound on a kernel: forward against
    torch.nn.functional.batch_norm in fp64, backward against fp64 autograd, on the
    well-conditioned classes."""
    D, tol = 128, 1e-12
    c = BC.case(N, D)
    well = [i for i, (a, _) in enumerate(c["cols"]) if a in BC.WELL]
    a64 = torch.from_numpy(c["a1"][:, well].astype(np.float64)).requires_grad_(True)
    g64 = torch.from_numpy(c["gamma"][well].astype(np.float64)).requires_grad_(True)
    b64 = torch.from_numpy(c["beta"][well].astype(np.float64)).requires_grad_(True)
    rm = torch.from_numpy(c["rm"][well].astype(np.float64))
    rv = torch.from_numpy(c["rv"][well].astype(np.float64))
    eps, f = float(BC.EPS), float(BC.MOMENTUM)
    y = torch.nn.functional.batch_norm(a64, rm, rv, g64, b64, True, f, eps)
    dbn = torch.from_numpy(c["dy"][:, well].astype(np.float64))
    y.backward(dbn)
    with torch.no_grad():
        mean = a64.mean(0)
        inv = 1 / torch.sqrt(a64.var(0, unbiased=False) + eps)
    sums = BC.forward_sums(N, D)
    bsum = O.backward_sums(c["dy"][:, well], c["a1"][:, well], mean.numpy(), inv.numpy())

    def close(got, want, scale=None):
        scale = abs(want) if scale is None else scale
        assert abs(float(got) - float(want)) <= tol * float(scale), (float(got), float(want))

    for j, col in enumerate(well):
        ch = O.forward_channel(sums, col, c["gamma"][col], c["beta"][col], BC.EPS)
        close(mean[j], ch["mean"], scale=O.mpf(ch["A"]) / N)
        close(inv[j], ch["invstd"])
        r_m, r_v, _ = O.running(ch["mean"], ch["var"], N, f, c["rm"][col], c["rv"][col])
        close(rm[j], r_m)
        close(rv[j], r_v)
        # y = a1 alpha + shift
        yo = c["a1"][:, col].astype(np.float64) * float(ch["alpha"]) + float(ch["shift"])
        assert np.abs(y[:, j].detach().numpy() - yo).max() <= tol * (
            np.abs(c["a1"][:, col]).max() * abs(float(ch["alpha"])) + 1)
        # backward: the input gradient is c1 dbn + c2 xhat + c3
        c1, c2, c3 = (float(t) for t in O.coef(bsum, j, c["gamma"][col], inv[j].item(), N))
        xh = (a64[:, j].detach().numpy() - mean[j].item()) * inv[j].item()
        d = dbn[:, j].numpy()
        want = c1 * d + c2 * xh + c3
        mag = abs(c1) * np.abs(d).max() + abs(c2) * np.abs(xh).max() + abs(c3)
        assert np.abs(a64.grad[:, j].numpy() - want).max() <= tol * mag
        close(g64.grad[j], bsum["sx"][j], scale=bsum["SX"][j])
        close(b64.grad[j], bsum["sd"][j], scale=bsum["SD"][j])


@pytest.mark.parametrize("D", BC.DIMS)
@pytest.mark.parametrize("N", BC.SIZES)
def test_fp64_model_is_inside_every_bound(N, D):
    for acc in (False, True):
        fwd, bwd = check_model(N, D, acc)
        path = "acc" if acc else "partials"
        print(fwd.line(f"model.fwd.{path}", N, D))
        print(bwd.line(f"model.bwd.{path}", N, D))
        fwd.assert_ok()
        bwd.assert_ok()
    # without batch statistics c2 and c3 are +0.0f, c1 still the correctly rounded product
    c, G = BC.case(N, D), model_grid(N)
    save, _, _ = model_forward(c, G, False)
    dbn, dgamma, dbeta, coef = model_backward(c, save, G, False, training=False)
    BC.check_backward(c["cols"], dbn, c["a1"], save, c["gamma"], dgamma, dbeta, coef, G, False,
                      training=False).assert_ok()


def test_eval_branch_of_the_model():
    c = BC.case(33, 64)
    rm, rv = c["rm"].astype(np.float64), c["rv"].astype(np.float64)
    inv = 1.0 / np.sqrt(rv + float(BC.EPS))
    alpha = c["gamma"].astype(np.float64) * inv
    save = np.stack([rm, inv, alpha, c["beta"].astype(np.float64) - rm * alpha]).astype(F32)
    BC.check_eval(c["cols"], save, c["gamma"], c["beta"], c["rm"], c["rv"]).assert_ok()
    save[1] = np.nextafter(np.nextafter(save[1], F32(9)), F32(9))     # two ulps off
    assert not BC.check_eval(c["cols"], save, c["gamma"], c["beta"], c["rm"], c["rv"]).ok()


MUTANTS = {
    # name: (what is wrong, the path it lives on)
    "n_rounded_up": ("divide by N rounded up to the tile", False),
    "b1_leak": ("one row of b1 leaked into the sums", False),
    "fp32_sums": ("fp32 accumulation of the sums", False),
    "lo_dropped": ("the lo word dropped: 2^-32 resolution", True),
    "biased_running": ("unbiased factor missing", False),
    "momentum_flipped": ("momentum applied as 1 - f", False),
    "sx_sd_swapped": ("sx and sd swapped in c2 / c3", False),
    "c2_sign": ("sign of c2 flipped", False),
    "c1_from_alpha": ("c1 from alpha32, one more rounding", False),
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_checker_rejects_mutant(mut):
    """Each wrong kernel fails on at least one case; the catching case and quantity are named."""
    what, acc = MUTANTS[mut]
    caught = None
    for N in (33, 2, 1031, 1):
        for D in (128, 32):
            fwd, bwd = check_model(N, D, acc, mut)
            fails = fwd.fails + bwd.fails
            if fails:
                q, ch, cls, ratio = max(fails, key=lambda t: t[3])
                caught = (N, D, q, ch, cls, ratio, len(fails))
                break
        if caught:
            break
    assert caught, f"mutant '{what}' passed every case: the table or a bound is too weak"
    N, D, q, ch, cls, ratio, n = caught
    print(f"BNMUTANT {mut} ({what}): caught at N={N} D={D} by {q} of channel {ch} "
          f"({'/'.join(cls)}) ratio={ratio:.3g}; {n} failures in that case")


def test_record_conditioning_of_the_one_pass_variance():
    """Recorded, not asserted: the smallest cond = (Q / N + mean^2) / (var + eps) at which the
    model's invstd is more than 2 fp32 ulp from exact (a property of var = s2 / N - mean^2)."""
    worst = None
    for N in BC.SIZES:
        c, G = BC.case(N, 128), model_grid(N)
        save, _, _ = model_forward(c, G, False)
        sums = BC.forward_sums(N, 128)
        for col in range(128):
            ch = O.forward_channel(sums, col, c["gamma"][col], c["beta"][col], BC.EPS)
            mean = O.mpf(ch["mean"])
            cond = float((O.mpf(ch["Q"]) / N + mean * mean) /
                         (O.mpf(ch["var"]) + O.mpf(O.frac(BC.EPS))))
            ulps = float(abs(O.mpf(float(save[1, col])) - ch["invstd"]) /
                         O.mpf(float(np.spacing(F32(float(ch["invstd"]))))))
            if ulps > 2 and (worst is None or cond < worst[0]):
                worst = (cond, ulps, N, c["cols"][col][0])
    assert worst is not None, "no channel of the table stresses the one-pass variance"
    print("BNCOND smallest cond with invstd more than 2 fp32 ulp off: cond=%.3g (%.3g ulp, N=%d, "
          "class %s)" % worst)
