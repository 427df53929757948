"""CPU: the high-precision oracle of the fused CRPS losses (tests/loss_oracle.py) is anchored,
and the fp64 torch formulation is measured against it on the row table of tests/loss_cases.py.

(a) oracle values: the reference's own rows and means (tests/golden/), forecast_oracle's closed
    forms, twcrps_oracle's closed forms, and mpmath.quad of int (F(x) - 1{x >= y})^2 dx;
(b) oracle gradients: central differences of the oracle's own values;
(c) the measurement that sets the kernels' bounds (loss_cases.MEASURED / BOUNDS), and the
    conditions on the table.
"""
import os

import mpmath as mp
import numpy as np
import pytest

import loss_cases as LC
import loss_oracle as LO
import twcrps_oracle as TO
from conftest import GOLDEN
from forecast_oracle import Dist

FIXTURE = {"normal": "normal", "mixed_normal": "normal_mixed", "mixed": "mixed", "mixed_u": "mixed_u"}
# one combination per kind and xi for the anchoring tests (the table's first u, c and t)
ANCHOR = [(k, cb) for k, cb in LC.ALL
          if cb["c"] == LC.C and cb["t"] == 5.0 and cb["u"] in (None, LC.f32(1.71))]
ANCHOR_IDS = [LC.combo_id(k, cb) for k, cb in ANCHOR]


# ------------------------------------------------------------------------------ (a) the values
@pytest.mark.parametrize("kind", list(FIXTURE))
def test_oracle_matches_the_reference_rows(kind):
    """The reference's closed forms evaluated in float64 (``*_crps64``; xi 0.5, u 1.71, t 5):
    2e-14 of max(|row|, 1) for the three censored kinds; the normal kind's rows carry the
    reference's fp32 1/sqrt(pi) and sqrt(2 pi), 1.2e-7 (tests/test_forecast.py): 1e-6.  The
    fixture's "mixed_u" rows are the hard-switch form at each row's own u (the scored
    distribution), which the oracle has as the tw term at the threshold c; the sigmoid blend is
    held by the reduced loss of reference_heads.npz below."""
    g = np.load(os.path.join(GOLDEN, "reference_crps_rows.npz"))
    name = FIXTURE[kind]
    pp, y, ref = g[f"{name}_pp"].astype(np.float64), g[f"{name}_y64"], g[f"{name}_crps64"]
    rows = [i for i in range(len(y)) if not np.isnan(y[i])][:48]
    xi, u = LC.f32(float(g["xi"][0])), LC.f32(float(g["u_fixed"][0]))
    worst = 0.0
    for i in rows:
        if kind == "mixed_u":
            v = LO.tw(kind, list(pp[i]), float(y[i]), LC.C, xi=xi).v
        else:
            v, _ = LO.row(kind, list(pp[i]), float(y[i]), xi=xi, u=u)
        worst = max(worst, abs(float(v) - ref[i]) / max(abs(ref[i]), 1.0))
    print(f"{kind}: {worst:.2e}")
    assert worst <= (1e-6 if kind == "normal" else 2e-14), worst


@pytest.mark.parametrize("kind", list(FIXTURE))
def test_oracle_mean_matches_the_reference_loss(kind):
    """The reference's reduced loss on its fp32 tensors (reference_heads.npz), at the project's
    loss bound 1e-6 relative."""
    g = np.load(os.path.join(GOLDEN, "reference_heads.npz"))
    name = FIXTURE[kind]
    val, _ = LO.rows(kind, g[f"{name}_pp"], g[f"{name}_y"], xi=LC.f32(0.5), u=LC.f32(1.71))
    ok = ~np.isnan(g[f"{name}_y"])
    assert not np.isnan(val[ok]).any() and np.isnan(val[~ok]).all()
    mean, ref = LC.fsum_mean(val[ok]), float(g[f"{name}_loss"][0])
    assert abs(mean - ref) <= 1e-6 * abs(ref), (mean, ref)


@pytest.mark.parametrize("kind,cb", [a for a in ANCHOR if a[0] != "mixed_u"],
                         ids=[i for a, i in zip(ANCHOR, ANCHOR_IDS) if a[0] != "mixed_u"])
def test_oracle_matches_forecast_oracle_closed_forms(kind, cb):
    """Dist.crps_rows (fp64, scipy) on the regular rows: forecast_cases' CRPS-row bound, 1e-12 of
    the largest row."""
    P, y, _ = LC.table(kind, cb)
    n = LC.N_REGULAR
    ref = Dist(kind, P[:n].astype(np.float64), u=cb["u"], xi=cb["xi"]).crps_rows(y[:n].astype(np.float64))
    val, _ = LC.oracle(kind, cb)
    assert np.abs(val[:n] - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("kind,cb", ANCHOR, ids=ANCHOR_IDS)
def test_oracle_tw_term_matches_twcrps_oracle_closed_forms(kind, cb):
    """twcrps_oracle.closed_rows (fp64, a second route through erfcx far up) at every threshold of
    the table, on the regular rows: its bound, 1e-12 of the largest row."""
    P, y, _ = LC.table(kind, cb)
    n = LC.N_REGULAR
    dist = Dist(kind, P[:n].astype(np.float64), u=cb["u"], xi=cb["xi"], c=cb["c"])
    for t in LC.thresholds(kind, cb):
        ref = TO.closed_rows(dist, y[:n].astype(np.float64), float(t))
        val, _ = LC.oracle(kind, cb, t, 1.0)
        assert np.abs(val[:n] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), t


def _quad_rows(kind, cb):
    """Edge rows and three regular ones with y >= c: below c the atom kinds' closed forms are not
    the integral, and the fp32 log(0.01) of a dry target is 6e-8 below the fp64 c."""
    P, y, tags = LC.table(kind, cb)
    want = ["y == c", "y == u", "y = u + 0.2", "p = 1e-7, y above u", "large scales"]
    ok = [i for i in range(len(y)) if kind == "normal" or float(y[i]) >= cb["c"]]
    return [i for i in ok if tags[i] in want] + [i for i in ok if i < LC.N_REGULAR][:3]


@pytest.mark.parametrize("kind,cb", ANCHOR, ids=ANCHOR_IDS)
def test_oracle_matches_quadrature_of_the_definition(kind, cb):
    """int (F(x) - 1{x >= y})^2 dx by mpmath.quad at 25 digits: the plain loss over the whole line
    (not for "mixed_u", whose sigmoid blend is no distribution's CRPS), the tw term from t' on
    with y' = max(y, t') at every threshold.  1e-13 of the term scale."""
    P, y, tags = LC.table(kind, cb)
    worst = 0.0
    for i in _quad_rows(kind, cb):
        pred, yi = [float(x) for x in P[i]], float(y[i])
        forms = [None] if kind != "mixed_u" else []
        forms += list(LC.thresholds(kind, cb))[1::2] if i >= LC.N_REGULAR else [LC.thresholds(kind, cb)[2]]
        for t in forms:
            scale = float(LC.term_scale(kind, P[i:i + 1], y[i:i + 1], cb, t)[0])
            if t is None:
                got = LO.plain(kind, pred, yi, cb["xi"], cb["u"], cb["c"], cb["t"]).v
                ref = LO.quad_crps(kind, pred, yi, cb["xi"], cb["u"], cb["c"])
            else:
                got = LO.tw(kind, pred, yi, t, cb["xi"], cb["u"], cb["c"]).v
                tp = t if kind == "normal" else max(t, cb["c"])
                ref = LO.quad_crps(kind, pred, max(yi, tp), cb["xi"], cb["u"], cb["c"], lower=tp)
            err = float(abs(got - ref)) / scale
            worst = max(worst, err)
            assert err <= 1e-13, (tags[i], t, float(got), float(ref))
    print(f"{LC.combo_id(kind, cb)}: {worst:.1e} of the term scale")


# --------------------------------------------------------------------------- (b) the gradients
@pytest.mark.parametrize("kind,cb", ANCHOR, ids=ANCHOR_IDS)
def test_oracle_gradient_matches_central_differences(kind, cb):
    """(f(x + h) - f(x - h)) / 2h of the oracle's own 50-digit values, h = 1e-18 |x| (truncation
    h^2 f''' / 6: 1e-30 or less here), on regular rows and on the edge rows that sit on no switch
    of the differentiated column, for the plain loss and two tw forms: 1e-20 of max(|g|, 1)."""
    P, y, tags = LC.table(kind, cb)
    edge = [i for i, t in enumerate(tags) if t in (
        "y == c", "y < c", "y = u + 50 sigma_u", "y = u + 0.2", "sigma 1e-3, y == c", "p = 1e-7",
        "mu far above u", "large scales", "u at its range's end")]
    ths = LC.thresholds(kind, cb)
    worst = 0.0
    for i in list(range(6)) + edge:
        pred, yi = [mp.mpf(float(x)) for x in P[i]], float(y[i])
        for tw_t, tw_w in ((None, 0.0), (ths[2], 0.3), (ths[4], 1.0)):
            kw = dict(xi=cb["xi"], u=cb["u"], c=cb["c"], t=cb["t"], tw_t=tw_t, tw_w=tw_w)
            _, g = LO.row(kind, pred, yi, **kw)
            big = max(max(abs(e) for e in g), 1)
            for k in range(len(pred)):
                h = mp.mpf(10) ** -18 * max(abs(pred[k]), mp.mpf(10) ** -3)
                hi, lo = list(pred), list(pred)
                hi[k], lo[k] = pred[k] + h, pred[k] - h
                fd = (LO.row(kind, hi, yi, **kw)[0] - LO.row(kind, lo, yi, **kw)[0]) / (2 * h)
                err = float(abs(fd - g[k]) / big)
                worst = max(worst, err)
                assert err <= 1e-20, (tags[i], tw_t, k, float(fd), float(g[k]))
    print(f"{LC.combo_id(kind, cb)}: {worst:.1e}")


def test_oracle_conventions_at_the_switches():
    """The chosen branch alone is differentiated: y == u takes loss_2 (y < u is false) and
    d|y - u| = 0; y' == t' leaves the tw term's first integral and its derivatives at 0; all mass
    on the atom gives a gradient of exactly 0 after rounding."""
    cb = dict(xi=LC.f32(0.2), u=LC.f32(1.71), c=LC.C, t=5.0)
    pred = [0.4, 0.9, 0.3, 0.7]
    at, above = (LO.plain("mixed", pred, yy, cb["xi"], cb["u"], cb["c"]) for yy in (cb["u"], cb["u"] + 1e-9))
    assert abs(at.v - above.v) < 2e-9
    # d/d sigma_u of sigma_u |y - u| / sigma_u is 0 on both sides; the rest is continuous
    assert all(abs(a - b) < 1e-8 for a, b in zip(at.d, above.d))
    P, y, tags = LC.table("mixed", cb)
    i = tags.index("all mass on the atom, y == c")
    val, grad = LC.oracle("mixed", cb)
    assert np.all(grad[i] == 0.0) and abs(val[i] - (float(y[i]) - cb["c"])) < 1e-300
    tw_at = LO.tw("mixed_normal", pred[:3], -3.0, -1.0)         # y' = t' = -1
    tw_lo = LO.tw("mixed_normal", pred[:3], -9.0, -1.0)
    assert tw_at.v == tw_lo.v and tw_at.d == tw_lo.d


# ------------------------------------------------------------------------- (c) the measurement
def _measure(kind, cb):
    """-> {class: [value, gradient]} worst errors of the fp64 reference over the combination's
    forms, the number of rows whose torch gradient is not finite, and the table's conditions."""
    P, y, tags = LC.table(kind, cb)
    cls = LC.row_class(kind, P)
    half = cb["xi"] is None or cb["xi"] == LC.f32(0.5)
    worst, skipped = {}, 0
    for tw_t, tw_w in LC.forms(kind, cb):
        ov, og = LC.oracle(kind, cb, tw_t, tw_w)
        assert np.isfinite(ov).all() and np.isfinite(og).all()
        rv, rg = LC.reference(kind, P, y, cb, tw_t, tw_w)
        ev, eg = LC.row_errors(kind, P, y, cb, rv, rg, ov, og, tw_t)
        assert np.isfinite(ev).all(), "a row of the table with a non-finite reference value"
        bad = ~np.isfinite(eg)
        # torch.where's NaN gradient from the branch not taken, only at xi != 0.5 and nothing else:
        # (1) the plain term below u - sigma_u / xi (pow of a negative base), (2) the tw term in
        # its tail form, whose unused body form has 1 - cdf rounded to 0 and pow's slope infinite
        # there, from (t' - u) / sigma_u = (2^(53 xi) - 1) / xi on (7.8e3 at xi = 0.2)
        if bad.any():
            assert not half
            u = P[:, 4].astype(np.float64) if kind == "mixed_u" else cb["u"]
            r = (y.astype(np.float64) - u) / P[:, 3]
            one = (r <= -1.0 / cb["xi"] + 1e-6) & (tw_w != 1.0)
            two = np.zeros(len(y), dtype=bool)
            if tw_t is not None:
                two = (max(tw_t, cb["c"]) - u) / P[:, 3] >= (2.0 ** (53 * cb["xi"]) - 1) / cb["xi"]
            assert np.all((one | two)[bad])
        skipped += int(bad.sum())
        for name in LC.CLASSES:
            sel = (cls == name) & ~bad
            if sel.any():
                LC.merge(worst, {name: [float(ev[sel].max()), float(eg[sel].max())]})
    return worst, skipped


@pytest.fixture(scope="module")
def measured():
    worst, skipped = {}, 0
    for kind, cb in LC.ALL:
        w, s = _measure(kind, cb)
        LC.merge(worst, w)
        skipped += s
    return worst, skipped


def test_reference_measurement(measured):
    """The fp64 torch formulation against the oracle on every row of the table, every
    combination of xi, u, c and t, the plain loss and every tw threshold and weight: the worst
    per-row errors of each class are the ones loss_cases.MEASURED records (so the kernels'
    bounds, 16 times them, stand on what this run reproduces)."""
    worst, skipped = measured
    for name in LC.CLASSES:
        print(f"{name}: value {worst[name][0]:.2e}, gradient {worst[name][1]:.2e}; "
              f"bounds {LC.BOUNDS[name][0]:.1e}, {LC.BOUNDS[name][1]:.1e}")
    print(f"rows x forms with a NaN torch gradient (xi != 0.5): {skipped}")
    for name in LC.CLASSES:
        for got, rec in zip(worst[name], LC.MEASURED[name]):
            # what is recorded is what this run finds: no worse than twice it (another libm's
            # last places), and the record is no padding
            assert got <= 2.0 * rec, (name, got, rec)
            assert rec <= max(4.0 * got, 2.0 ** -51), (name, got, rec)


def test_bounds_are_derived():
    for name in LC.CLASSES:
        for rec, bound in zip(LC.MEASURED[name], LC.BOUNDS[name]):
            assert bound == max(16.0 * rec, 64 * 2.0 ** -52)


def test_table_covers_what_it_claims():
    for kind, cb in LC.ALL:
        P, y, tags = LC.table(kind, cb)
        assert P.dtype == np.float32 and y.dtype == np.float32 and not np.isnan(y).any()
        cls = LC.row_class(kind, P)
        assert set(cls) == set(LC.CLASSES)
        yd = y.astype(np.float64)
        if kind in ("mixed", "mixed_u"):
            u = P[:, 4].astype(np.float64) if kind == "mixed_u" else np.full(len(y), cb["u"])
            assert (yd == u).any() and (yd < u).any() and (yd > u).any()
            for t in LC.thresholds(kind, cb):  # both forms of the tw term, and the censored one
                tp = max(t, cb["c"])
                if t == LC.thresholds(kind, cb)[3]:
                    assert (tp >= u).any()
                    assert kind == "mixed" or ((tp < u).any() and not (tp == u).any())
            assert (max(LC.thresholds(kind, cb)[4], cb["c"]) > u).all()
        assert (y == np.float32(cb["c"])).any() and (yd < cb["c"]).any()
        assert (P[:, 1] == np.float32(1e-6)).any() and (P[:, 1] == np.float32(30.0)).any()
        if kind != "normal":
            assert {0.0, 1.0} <= set(P[:, 2].tolist())
