"""Threshold-weighted CRPS (twCRPS; Gneiting & Ranjan 2011, Allen et al. 2023) of the
predictive distribution of :mod:`raincast_gnn.forecast`, weight ``w(x) = 1{x >= t}``:

    twCRPS_t(F, y) = int_t^inf (F(x) - 1{x >= y})^2 dx = CRPS(F_t, max(y, t))

with ``F_t`` the distribution of ``max(Y, t)``: a proper score that looks only at the part of the
distribution above ``t``.  Everything is in model space ``log(mm + 0.01)``, fp64, per row.

``F_t`` is ``F`` censored at ``t' = max(t, c)`` (``t' = t`` for ``normal``, which has no ``c``), so
with ``y' = max(y, t')`` the closed forms of the losses give it:

* ``normal``: the ``mixed_normal`` form with ``p = 0``, ``c := t'``, ``y := y'``;
* ``mixed_normal``: its own form with ``c := t'``, ``y := y'``; both evaluated in upper
  probabilities (``_censored``), which keeps the relative accuracy far up the tail;
* ``mixed`` / ``mixed_u``, ``t' < u`` (the row's own ``u`` for ``mixed_u``): the ``MixedLoss`` form,
  ``where(y' < u, loss_1, loss_2)``, with ``c := t'``, ``y := y'``;
* ``mixed`` / ``mixed_u``, ``t' >= u``: only the tail is left.  With ``a = 1 - m_u``,
  ``w(x) = 1 + xi (x - u) / sigma_u``, ``e1 = -(1 - xi)/xi``, ``e2 = -(2 - xi)/xi``::

      (y' - t') + 2 a sigma_u/(1 - xi) (w(y')^e1 - w(t')^e1) + a^2 sigma_u/(2 - xi) w(t')^e2

  which is ``pareto_crps(y', u, m_u, sigma_u, xi)`` at ``t' = u``, where the body form's ``upper``
  term is 0: the two branches meet continuously.  ``a = (1 - p) Phi(-z(u))``, from erfc.

A threshold of ``-inf`` gives the CRPS at ``max(y, c)`` (at ``y`` for ``normal``), ``+inf`` gives
0, NaN gives NaN.  This module is the fp64 torch formulation (differentiable: the loss classes
use it with autograd where the fused kernel does not apply); the kernels are
``gine_forecast_twcrps`` and ``gine_crps_tw_fwd`` (csrc/gine_forecast.hip, csrc/gine_loss.hip).
"""
from __future__ import annotations

import math

import torch

from . import _lib

_SQRT2 = math.sqrt(2.0)
_LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
_INV_SQRT_PI = 1.0 / math.sqrt(math.pi)


def _Phi(z):
    return 0.5 * (1 + torch.erf(z / _SQRT2))


def _upper_Phi(z):
    return 0.5 * torch.special.erfc(z / _SQRT2)


def _phi(z):
    return torch.exp(-0.5 * z * z - _LOG_SQRT_2PI)


_MILLS_FROM = 3.0


def _mills(z):
    """(1 - Phi(z)) / phi(z), z >= 0."""
    return math.sqrt(math.pi / 2.0) * torch.special.erfcx(z / _SQRT2)


def _normal(mu, sigma, y):
    z = (y - mu) / sigma
    return sigma * (z * (2.0 * _Phi(z) - 1.0) + 2.0 * _phi(z) - _INV_SQRT_PI)


def _censored(mu, sigma, p, y, c):
    """CRPS at y >= c of a normal with an atom p, censored at c: the MixedNormalCRPS closed form
    rewritten in upper probabilities S = (1 - p) (1 - Phi),
        (y - c) - 2 int_c^y S dx + int_c^inf S^2 dx,
    so that no term is larger than the result where c lies far up the tail (the lower form
    subtracts O(sigma z) terms there: an absolute error of 1e-15 on values of 1e-5)."""
    yt = (y - mu) / sigma
    ct = (c - mu) / sigma
    q = 1.0 - p
    Uy, Uc = _upper_Phi(yt), _upper_Phi(ct)
    G = (yt * Uy - _phi(yt)) - (ct * Uc - _phi(ct))          # int_ct^yt (1 - Phi)
    # y = c: exactly 0, and so are its derivatives (autograd would add and subtract the two
    # sides' and absorb the O(S^2) gradient of H between them where S is tiny)
    G = torch.where(y > c, G, torch.zeros_like(G))
    H = -(ct * Uc * Uc) + 2.0 * _phi(ct) * Uc - _INV_SQRT_PI * _upper_Phi(_SQRT2 * ct)
    # from z(c) = 3 on through the Mills ratio R = (1 - Phi) / phi (erfcx): the three terms are
    # 2 z^2 times their sum, and as products of exp() each also carries that function's
    # argument rounding z^2 eps / 2 -- z^4 eps, 1e-10 of a value at z = 26; factored as
    # phi(z)^2 (2 R - z R^2 - sqrt2 R(sqrt2 z)) only the 2 z^2 is left
    zc = torch.clamp(ct, min=_MILLS_FROM)  # (the other side of the where stays finite)
    R, R2 = _mills(zc), _mills(_SQRT2 * zc)
    far = _phi(zc) ** 2 * (2.0 * R - zc * R * R - _SQRT2 * R2)
    H = torch.where(ct >= _MILLS_FROM, far, H)
    return (y - c) + sigma * (q * (q * H - 2.0 * G))


def _pareto(y, u, m, s, xi):
    t = (y - u) / s
    base = 1.0 + xi * torch.clamp(t, min=0.0)  # only read where t > 0
    cdf = torch.where(t <= 0, torch.zeros_like(base), 1.0 - torch.pow(base, -1.0 / xi))
    om = 1.0 - m
    return s * (torch.abs(t) - 2.0 / (1.0 - xi) * (om * (1.0 - torch.pow(1.0 - cdf, 1.0 - xi)))
                + om * om / (2.0 - xi))


def _mixed(mu, sigma, p, su, u, y, c, xi):
    """The MixedLoss closed form, where(y < u, loss_1, loss_2), censored at c < u."""
    ct = (c - mu) / sigma
    ut = (u - mu) / sigma
    yt = (y - mu) / sigma
    q = 1.0 - p
    m_u = p + q * _Phi(ut)
    Pc = p + q * _Phi(ct)
    Pu = q * (1.0 - _Phi(ut))
    t2 = ut * Pu * Pu - ct * Pc * Pc
    t3 = -2.0 * (q * _phi(ct) * Pc + q * _phi(ut) * Pu)
    t5 = -_INV_SQRT_PI * (q * q * (_Phi(_SQRT2 * ut) - _Phi(_SQRT2 * ct)))
    t1 = yt * (2.0 * (p + q * _Phi(yt)) - 1.0)
    loss1 = sigma * (t1 + t2 + t3 + 2.0 * (q * _phi(yt)) + t5) + _pareto(u, u, m_u, su, xi)
    upper = sigma * (ut + t2 + t3 - 2.0 * (-(q * _phi(ut)) + ut * Pu) + t5)
    return torch.where(y < u, loss1, _pareto(y, u, m_u, su, xi) + upper)


def _tail(mu, sigma, p, su, u, y, t, xi):
    """t >= u: what is left of the Pareto tail above t (y >= t)."""
    a = (1.0 - p) * _upper_Phi((u - mu) / sigma)
    wy = 1.0 + xi * ((y - u) / su)
    wt = 1.0 + xi * ((t - u) / su)
    e1, e2 = -(1.0 - xi) / xi, -(2.0 - xi) / xi
    d = torch.pow(wy, e1) - torch.pow(wt, e1)
    d = torch.where(y > t, d, torch.zeros_like(d))  # y = t: exactly 0, derivatives too
    return (y - t) + (2.0 / (1.0 - xi) * (a * su * d)
                      + 1.0 / (2.0 - xi) * (a * a * su * torch.pow(wt, e2)))


def tw_rows(kind: int, mu, sigma, p, su, u, y, t, c: float, xi: float) -> torch.Tensor:
    """twCRPS of the rows: ``mu, sigma, p, su, u, y`` fp64 ``[N, 1]`` (``p`` / ``su`` / ``u`` are
    not read for the kinds without them; ``u`` may be a number), ``t`` fp64 thresholds ``[1, T]``
    -> ``[N, T]``.  ``y`` must hold no NaN.  Gradients flow to the parameters through whichever
    branch a row takes."""
    atom = kind != _lib.LOSS_NORMAL
    tail = kind in (_lib.LOSS_MIXED, _lib.LOSS_MIXED_U)
    inf = float("inf")
    zero = torch.zeros_like(t)
    t_nan = torch.isnan(t)
    tp = torch.where(t_nan, zero, t)
    if atom:
        tp = torch.clamp(tp, min=c)
    t_pinf, t_ninf = tp == inf, tp == -inf
    tp = torch.where(t_pinf | t_ninf, zero, tp)  # both replaced below
    yp = torch.maximum(y, tp)
    if not atom:
        out = _censored(mu, sigma, torch.zeros_like(mu), yp, tp)
        out = torch.where(t_ninf, _normal(mu, sigma, y), out)  # the censored form's limit
    elif not tail:
        out = _censored(mu, sigma, p, yp, tp)
    else:
        u = u if torch.is_tensor(u) else torch.full_like(mu, float(u))
        body = _mixed(mu, sigma, p, su, u, yp, tp, xi)
        # the tail form on arguments that keep w >= 1 where the body is what is taken
        tl = _tail(mu, sigma, p, su, u, torch.maximum(yp, u), torch.maximum(tp, u), xi)
        out = torch.where(tp >= u, tl, body)
    out = torch.where(t_pinf, torch.zeros_like(out), out)  # nothing above
    return torch.where(t_nan, torch.full_like(out, float("nan")), out)


def tw_rows_of(kind: int, pred: torch.Tensor, y: torch.Tensor, t: torch.Tensor, u_fixed, c: float,
               xi: float) -> torch.Tensor:
    """:func:`tw_rows` from a prediction ``[N, K]`` (any float dtype) and ``y [N, 1]``."""
    P = pred.double()
    col = lambda k: P[:, k:k + 1]  # noqa: E731
    p = col(2) if kind != _lib.LOSS_NORMAL else None
    su = col(3) if kind in (_lib.LOSS_MIXED, _lib.LOSS_MIXED_U) else None
    u = col(4) if kind == _lib.LOSS_MIXED_U else u_fixed
    return tw_rows(kind, col(0), col(1), p, su, u, y.double(), t, c, xi)
