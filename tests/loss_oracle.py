"""Independent high-precision oracle of the fused CRPS losses (csrc/gine_loss.hip): per row, the
loss value and its gradient with respect to the K prediction columns, in 50-digit mpmath
arithmetic.  Shares no code with the package.

Semantics, as the kernel header restates models/loss.py (z(x) = (x - mu) / sigma, q = 1 - p,
Phi / phi the standard normal cdf / pdf, U = 1 - Phi taken from erfc):

  normal        sigma (z_y (2 Phi(z_y) - 1) + 2 phi(z_y) - 1/sqrt(pi))
  mixed_normal  sigma (t1 + t2 + t3 + t4 + t5) with P_c = p + q Phi(z_c),
                t1 = z_y (2 (p + q Phi(z_y)) - 1), t2 = -z_c P_c^2, t3 = -2 q phi(z_c) P_c,
                t4 = 2 q phi(z_y), t5 = -q^2 U(sqrt2 z_c) / sqrt(pi);  y is taken as it is
  mixed         y < u: loss_1 = body(y) + pareto(u),  else loss_2 = pareto(y) + upper, with
                a = q U(z_u) = 1 - m_u, T = z_u a^2 - z_c P_c^2 - 2 q (phi(z_c) P_c + phi(z_u) a)
                - q^2 (Phi(sqrt2 z_u) - Phi(sqrt2 z_c)) / sqrt(pi),
                body(y) = sigma (t1 + t4 + T), upper = sigma (z_u + T + 2 q phi(z_u) - 2 z_u a),
                pareto(x) = sigma_u (|r| - 2 a (1 - S^(1 - xi)) / (1 - xi) + a^2 / (2 - xi)),
                r = (x - u) / sigma_u, S = 1 (r <= 0), (1 + xi r)^(-1/xi) (r > 0)
  mixed_u       sigmoid(t (u - y)) (loss_1 - loss_2) + loss_2 with the row's own u (column 4)

Threshold-weighted term (tests/twcrps_oracle.py's definitions): twCRPS_t = CRPS(F_t', y') with
t' = max(t, c) (t for "normal"), y' = max(y, t'), F_t' the distribution censored at t':
mixed_normal's form with c := t', y := y' (p = 0 for "normal"); for the kinds with a tail the
hard-switch "mixed" form with c := t', y := y' where t' < u (the row's u for "mixed_u"), and
where t' >= u, with w(x) = 1 + xi (x - u) / sigma_u,
  (y' - t') + 2 a sigma_u (w(y')^e1 - w(t')^e1) / (1 - xi) + a^2 sigma_u w(t')^e2 / (2 - xi),
  e1 = -(1 - xi) / xi, e2 = -(2 - xi) / xi.
The row's loss is (1 - w) L + w twCRPS_t.

Gradient: exact differentiation of these forms, carried beside the value.  Every switch (y < u,
r <= 0, t' < u, max) is decided at the point and only the chosen branch is differentiated;
d|x|/dx = 0 at 0.  tests/test_loss_rows.py holds it to central differences of the values.

``xi`` and a fixed ``u`` are to be given as the fp32-rounded numbers the loss classes pass.
"""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
C = math.log(0.01)
WIDTH = {"normal": 2, "mixed_normal": 3, "mixed": 4, "mixed_u": 5}
_SQRT2 = mp.sqrt(2)
_SQRTPI = mp.sqrt(mp.pi)
_SQRT2PI = mp.sqrt(2 * mp.pi)


class V:
    """A value and its partial derivatives with respect to the K prediction columns."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def lift(x, k):
        return x if isinstance(x, V) else V(mp.mpf(x), [mp.mpf(0)] * k)

    def _o(self, x):
        return V.lift(x, len(self.d))

    def chain(self, f, df):
        return V(f, [df * e for e in self.d])

    def __add__(self, o):
        o = self._o(o)
        return V(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, [-a for a in self.d])

    def __sub__(self, o):
        return self + (-self._o(o))

    def __rsub__(self, o):
        return self._o(o) - self

    def __mul__(self, o):
        o = self._o(o)
        return V(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._o(o)
        r = self.v / o.v
        return V(r, [(a - r * b) / o.v for a, b in zip(self.d, o.d)])

    def __rtruediv__(self, o):
        return self._o(o) / self

    def pow(self, e):  # constant exponent, positive base
        return self.chain(self.v ** e, e * self.v ** (e - 1))

    def abs(self):
        return self.chain(abs(self.v), mp.sign(self.v))


def _pdf(z):
    f = mp.exp(-z.v * z.v / 2) / _SQRT2PI
    return z.chain(f, -z.v * f)


def _Phi(z):
    return z.chain(mp.erfc(-z.v / _SQRT2) / 2, mp.exp(-z.v * z.v / 2) / _SQRT2PI)


def _U(z):  # 1 - Phi
    return z.chain(mp.erfc(z.v / _SQRT2) / 2, -mp.exp(-z.v * z.v / 2) / _SQRT2PI)


def _sigmoid(x):
    s = 1 / (1 + mp.exp(-x.v))
    return x.chain(s, s * (1 - s))


def _normal(mu, s, y):
    z = (y - mu) / s
    return s * (z * (2 * _Phi(z) - 1) + 2 * _pdf(z) - 1 / _SQRTPI)


def _mixed_normal(mu, s, p, y, c):
    zy, zc = (y - mu) / s, (c - mu) / s
    q = 1 - p
    Pc = p + q * _Phi(zc)
    t1 = zy * (2 * (p + q * _Phi(zy)) - 1)
    return s * (t1 - zc * Pc * Pc - 2 * q * _pdf(zc) * Pc + 2 * q * _pdf(zy)
                - q * q * _U(_SQRT2 * zc) / _SQRTPI)


def _pareto(x, u, a, su, xi):
    r = (x - u) / su
    if r.v > 0:
        gain = 1 - (1 + xi * r).pow(-(1 - xi) / xi)  # 1 - S^(1 - xi)
    else:
        gain = 0
    return su * (r.abs() - 2 * a * gain / (1 - xi) + a * a / (2 - xi))


def _mixed_branches(mu, s, p, su, u, y, c, xi):
    zy, zc, zu = (y - mu) / s, (c - mu) / s, (u - mu) / s
    q = 1 - p
    a = q * _U(zu)
    Pc = p + q * _Phi(zc)
    T = (zu * a * a - zc * Pc * Pc - 2 * q * (_pdf(zc) * Pc + _pdf(zu) * a)
         - q * q * (_Phi(_SQRT2 * zu) - _Phi(_SQRT2 * zc)) / _SQRTPI)
    body = s * (zy * (2 * (p + q * _Phi(zy)) - 1) + 2 * q * _pdf(zy) + T)
    upper = s * (zu + T + 2 * q * _pdf(zu) - 2 * zu * a)
    return body + _pareto(u, u, a, su, xi), _pareto(y, u, a, su, xi) + upper


def _mixed_hard(mu, s, p, su, u, y, c, xi):
    l1, l2 = _mixed_branches(mu, s, p, su, u, y, c, xi)
    return l1 if y.v < u.v else l2


def _tail(mu, s, p, su, u, yp, tp, xi):
    a = (1 - p) * _U((u - mu) / s)
    wy, wt = 1 + xi * ((yp - u) / su), 1 + xi * ((tp - u) / su)
    e1, e2 = -(1 - xi) / xi, -(2 - xi) / xi
    return (yp - tp) + 2 * a * su * (wy.pow(e1) - wt.pow(e1)) / (1 - xi) \
        + a * a * su * wt.pow(e2) / (2 - xi)


def _columns(kind, pred):
    k = WIDTH[kind]
    assert len(pred) == k
    return [V(mp.mpf(x), [mp.mpf(int(i == j)) for j in range(k)]) for i, x in enumerate(pred)]


def plain(kind, pred, y, xi=None, u=None, c=C, t=5.0):
    """The loss of one row -> V (value and gradient)."""
    v = _columns(kind, pred)
    k = len(v)
    y, c = V.lift(y, k), V.lift(c, k)
    if kind == "normal":
        return _normal(v[0], v[1], y)
    if kind == "mixed_normal":
        return _mixed_normal(v[0], v[1], v[2], y, c)
    xi = mp.mpf(xi)
    if kind == "mixed":
        return _mixed_hard(v[0], v[1], v[2], v[3], V.lift(u, k), y, c, xi)
    l1, l2 = _mixed_branches(v[0], v[1], v[2], v[3], v[4], y, c, xi)
    return _sigmoid(mp.mpf(t) * (v[4] - y)) * (l1 - l2) + l2


def tw(kind, pred, y, tw_t, xi=None, u=None, c=C):
    """The threshold-weighted term of one row at threshold ``tw_t`` -> V."""
    v = _columns(kind, pred)
    k = len(v)
    tp = mp.mpf(tw_t) if kind == "normal" else max(mp.mpf(tw_t), mp.mpf(c))
    yp = max(mp.mpf(y), tp)
    yp, tp = V.lift(yp, k), V.lift(tp, k)
    if kind == "normal":
        return _mixed_normal(v[0], v[1], V.lift(0, k), yp, tp)
    if kind == "mixed_normal":
        return _mixed_normal(v[0], v[1], v[2], yp, tp)
    xi = mp.mpf(xi)
    uu = v[4] if kind == "mixed_u" else V.lift(u, k)
    if tp.v < uu.v:
        return _mixed_hard(v[0], v[1], v[2], v[3], uu, yp, tp, xi)
    return _tail(v[0], v[1], v[2], v[3], uu, yp, tp, xi)


def row(kind, pred, y, xi=None, u=None, c=C, t=5.0, tw_t=None, tw_w=0.0):
    """(1 - tw_w) L + tw_w twCRPS of one row -> (value, [K partial derivatives]) as mpf.
    ``pred`` / ``y``: numbers or mpf; floats are taken exactly."""
    if tw_t is None or tw_w == 0.0:
        r = plain(kind, pred, y, xi, u, c, t)
    else:
        w = mp.mpf(tw_w)
        r = w * tw(kind, pred, y, tw_t, xi, u, c)
        if tw_w != 1.0:
            r = r + (1 - w) * plain(kind, pred, y, xi, u, c, t)
    return r.v, r.d


def rows(kind, P, y, **kw):
    """``P [N, K]``, ``y [N]`` (NaN: a masked row) -> (values [N] float64, NaN where masked;
    gradients [N, K] float64, 0 where masked), each rounded once from the 50-digit result."""
    P, y = np.asarray(P), np.asarray(y)
    val = np.full(len(y), np.nan)
    grad = np.zeros((len(y), WIDTH[kind]))
    for i in range(len(y)):
        if np.isnan(y[i]):
            continue
        v, d = row(kind, [float(x) for x in P[i]], float(y[i]), **kw)
        val[i] = float(v)
        grad[i] = [float(e) for e in d]
    return val, grad


# --------------------------------------------------------------------- the definition, by quadrature
def quad_crps(kind, pred, y, xi=None, u=None, c=C, lower=None, digits=25):
    """int_lower^inf (F(x) - 1{x >= y})^2 dx of one row by mpmath.quad, F from the definition
    (the hard-switch distribution for "mixed_u", u = pred[4]); lower = None: the whole line (from
    c for the kinds with an atom: F = 0 below, so only y >= c is the closed forms' case)."""
    with mp.workdps(digits):
        f = [mp.mpf(x) for x in pred]
        mu, s = f[0], f[1]
        p = f[2] if kind != "normal" else mp.mpf(0)
        tail = kind in ("mixed", "mixed_u")
        y = mp.mpf(y)
        if tail:
            su, xi = f[3], mp.mpf(xi)
            uu = f[4] if kind == "mixed_u" else mp.mpf(u)
            a = (1 - p) * mp.erfc((uu - mu) / s / mp.sqrt(2)) / 2

        def S(x):  # 1 - F
            if tail and x >= uu:
                return a * (1 + xi * (x - uu) / su) ** (-1 / xi)
            return (1 - p) * mp.erfc((x - mu) / s / mp.sqrt(2)) / 2

        lo = lower if lower is not None else (-mp.inf if kind == "normal" else mp.mpf(c))
        lo = mp.mpf(lo)
        assert y >= lo
        cuts = sorted({lo, y, mp.inf} | ({uu} if tail and uu > lo else set())
                      | {x for x in (mu - 8 * s, mu, mu + 8 * s) if x > lo})
        total = mp.mpf(0)
        for a_, b_ in zip(cuts[:-1], cuts[1:]):
            if b_ <= y:
                total += mp.quad(lambda x: (1 - S(x)) ** 2, [a_, b_])
            else:
                total += mp.quad(lambda x: S(x) ** 2, [a_, b_])
        return total
