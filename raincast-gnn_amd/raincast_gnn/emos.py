"""EMOS, the baseline a post-processing model has to beat: per station, fitted by minimum CRPS.

Ensemble model output statistics (Gneiting et al. 2005) maps a handful of summary statistics
of the raw ensemble affinely to the parameters of the predictive distribution and fits the
coefficients per station.  Here the distribution is the model's own kind, so the result is a
``pred [N, K]`` in the model's format and every verification of :mod:`raincast_gnn.forecast`,
:mod:`raincast_gnn.compare` and :mod:`raincast_gnn.reliability` applies to it unchanged.

Definition.  Rows are in collated order (``row = day * S + station``).  Per row,
with ``x_i = shift + scale * member_i`` (a NaN member is missing, ``m`` valid ones) and ``c``
the censoring point, in fp64 and summed in member order::

    mean = (1/m) sum x_i    sd = sqrt((1/m) sum (x_i - mean)^2)    dry = #{x_i <= c} / m

Kinds ``normal`` (K = 2), ``mixed_normal`` (K = 3) and ``mixed`` with its fixed ``u`` (K = 4);
``mixed_u`` is rejected: its ``u`` is a per-row network output and EMOS has none.  With
``theta [P = 2K]``, ``z = (mean, sd, dry, sd)`` and ``raw_k = theta[2k] + theta[2k+1] z_k`` the
links are those of :class:`raincast_gnn.postprocess.PostProcess` in fp64: ``mu = raw_0``,
``sigma = softplus(raw_1) + 1e-6``, ``p = sigmoid(raw_2)``, ``sigma_u = softplus(raw_3) + 1e-6``
with ``softplus(x) = max(x, 0) + log1p(exp(-|x|))`` (no threshold, unlike
``torch.nn.functional.softplus``).  Per group over its ``n`` valid rows (a target and
``m >= 1``)::

    J(theta) = (1/n) sum crps(pred(theta; row), y_row) + ridge |theta - theta0|^2

``crps`` is the loss's closed form of the kind, ``theta0 = (0, 1, b, 0, 0, 0, b, 0)`` truncated
to ``P`` with ``b = log(e - 1)`` (the raw ensemble's mean with unit spread).  The ridge is part
of the definition: without it the mixed kinds' sigmoid separates and the minimiser runs off.

Optimiser: BFGS on the inverse Hessian from ``H = I``; stop (status 0) when
``max|g| <= gtol max(1, |J|)``; ``d = -H g``, and ``H = I``, ``d = -g`` unless ``g . d < 0``;
Armijo backtracking (``c1 = 1e-4``) over the steps ``1, 1/2, ..., 2^-40``, a non-finite ``J``
failing; ``H`` updated when ``s . y > 1e-10 |s| |y|``; at most ``max_iter`` iterations.  Status
1: iteration limit; 2: no decrease along ``d`` (``theta`` is the last accepted point); 3: fewer
than ``min_rows`` valid rows (``theta = theta0``, ``J`` NaN).

HIP tensors with at most 64 members go to ``gine_emos_predictors`` / ``gine_emos_fit`` /
``gine_emos_predict`` (csrc/gine_emos.hip: one 256-thread workgroup per group for the whole
optimisation, one launch each); CPU tensors, and ensembles with more members, go to the fp64
torch formulation of the same definition and the same optimiser below, batched over the groups.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .ensemble import RawEnsemble
from .forecast import C_DEFAULT, KINDS, Forecast

EMOS_KINDS = (_lib.LOSS_NORMAL, _lib.LOSS_MIXED_NORMAL, _lib.LOSS_MIXED)
_WIDTH = {_lib.LOSS_NORMAL: 2, _lib.LOSS_MIXED_NORMAL: 3, _lib.LOSS_MIXED: 4}
SOFTPLUS_ONE = math.log(math.e - 1.0)  # softplus(b) = 1
LINK_EPS = 1e-6
ARMIJO = 1e-4
MAX_HALVINGS = 40
CURVATURE = 1e-10
STATUS = {0: "converged", 1: "iteration limit", 2: "no decrease along the direction",
          3: "too few valid rows"}


@dataclass
class EmosFit:
    """What :meth:`Emos.fit` returns, one entry per group (station, or one global group):
    ``theta [G, 2K]``, the ``objective`` J, the mean ``crps`` without the ridge term,
    ``grad_max = max|g|`` at ``theta`` (fp64), and the ``iterations``, ``evaluations``, valid
    ``rows`` and ``status`` (int64; :data:`STATUS`).  Tensors on the data's device."""
    theta: torch.Tensor
    objective: torch.Tensor
    crps: torch.Tensor
    grad_max: torch.Tensor
    iterations: torch.Tensor
    evaluations: torch.Tensor
    rows: torch.Tensor
    status: torch.Tensor


def theta_start(P: int, device=None) -> torch.Tensor:
    """``theta0``: the start and the ridge's centre."""
    b = SOFTPLUS_ONE
    return torch.tensor([0.0, 1.0, b, 0.0, 0.0, 0.0, b, 0.0][:P], dtype=torch.float64,
                        device=device)


def softplus(x: torch.Tensor) -> torch.Tensor:
    """``max(x, 0) + log1p(exp(-|x|))``: ``logaddexp(x, 0)``, which evaluates exactly that."""
    return torch.logaddexp(x, torch.zeros_like(x))


class Emos:
    """EMOS for the distribution ``kind`` (``"normal"``, ``"mixed_normal"``, ``"mixed"`` or the
    matching ``GINE_LOSS_*`` value); ``u``, ``xi``, ``c`` as :class:`Forecast` takes them."""

    def __init__(self, kind, u=None, xi=None, c: float = C_DEFAULT, ridge: float = 1e-3,
                 gtol: float = 1e-8, max_iter: int = 200, min_rows: int = 30):
        k = KINDS[kind] if isinstance(kind, str) else int(kind)
        if k == _lib.LOSS_MIXED_U:
            raise ValueError("EMOS has no 'mixed_u': that kind's u is a per-row network output; "
                             "fit the 'mixed' kind with a fixed u instead")
        if k not in EMOS_KINDS:
            raise ValueError(f"unknown kind {kind!r}")
        self.kind, self.K = k, _WIDTH[k]
        self.c = float(c)
        self.u = 0.0 if u is None else float(u)
        self.xi = 0.5 if xi is None else float(xi)
        if k == _lib.LOSS_MIXED:
            if xi is None or not 0.0 < self.xi < 1.0:
                raise ValueError(f"kind 'mixed' needs 0 < xi < 1, got {xi!r}")
            if u is None or not self.u > self.c:
                raise ValueError(f"kind 'mixed' needs a fixed u > c, got {u!r}")
        if not (ridge >= 0.0 and math.isfinite(ridge)):
            raise ValueError(f"ridge must be finite and >= 0, got {ridge!r}")
        if not (gtol >= 0.0 and math.isfinite(gtol)):
            raise ValueError(f"gtol must be finite and >= 0, got {gtol!r}")
        if not 0 <= int(max_iter) <= _lib.EMOS_MAX_ITER:
            raise ValueError(f"max_iter must lie in 0..{_lib.EMOS_MAX_ITER}, got {max_iter!r}")
        if int(min_rows) < 1:
            raise ValueError(f"min_rows must be at least 1, got {min_rows!r}")
        self.ridge, self.gtol = float(ridge), float(gtol)
        self.max_iter, self.min_rows = int(max_iter), int(min_rows)

    @classmethod
    def from_model(cls, model, **kw) -> "Emos":
        """EMOS for the distribution that ``model`` predicts: ``loss`` / ``grad_u`` / ``u`` /
        ``xi`` read and rounded to fp32 as :meth:`Forecast.from_model` does."""
        loss = model.loss
        c = getattr(getattr(model, "loss_fn", None), "c", C_DEFAULT)
        if loss == "NormalCRPS":
            return cls(_lib.LOSS_NORMAL, c=C_DEFAULT, **kw)
        if loss == "MixedNormalCRPS":
            return cls(_lib.LOSS_MIXED_NORMAL, c=float(c), **kw)
        if loss == "MixedLoss":
            if model.grad_u == "True":
                return cls(_lib.LOSS_MIXED_U)  # raises: no EMOS for a learned u
            return cls(_lib.LOSS_MIXED, u=float(np.float32(model.u)),
                       xi=float(np.float32(model.xi)), c=float(c), **kw)
        raise ValueError(f"unknown loss '{loss}'")

    # ------------------------------------------------------------------ public
    def predictors(self, raw: RawEnsemble) -> torch.Tensor:
        """``(mean, sd, dry)`` of every row of ``raw``, fp64 ``[N, 3]`` in the rows' order; NaN
        for a row without a valid member."""
        if raw.on_kernel:
            return self._pack_hip(raw, None, 0)[:, :3]
        return self._predictors_torch(raw)

    def fit(self, raw: RawEnsemble, y: torch.Tensor, num_stations: int | None = None) -> EmosFit:
        """Fit ``theta`` per station on the rows of ``raw`` and the targets ``y [N]`` (model
        space, NaN = missing), rows in collated order with ``N`` a multiple of
        ``num_stations``.  ``num_stations=None`` fits one global parameter set: on the device
        that is a single workgroup, serial in the rows -- meant for comparison, not speed."""
        N, S = raw.members.size(0), self._stations(raw, num_stations)
        y = y.detach().to(raw.device).float().reshape(-1).contiguous()
        if y.numel() != N:
            raise ValueError(f"y must have {N} entries, got {y.numel()}")
        G, T = (S, N // S) if S > 0 else (1, N)
        if raw.on_kernel:
            return self._fit_hip(raw, y, S, G, T)
        z = self._group_major(self._predictors_torch(raw), S)
        return self._fit_torch(z.reshape(G, T, 3), self._group_major(y.double(), S).reshape(G, T))

    def predict(self, raw: RawEnsemble, fit: EmosFit, num_stations: int | None = None):
        """The EMOS prediction ``pred [N, K]`` fp32 for the rows of ``raw`` (collated order, the
        stations of the fit), in the model's own format; NaN rows without a valid member."""
        N, S = raw.members.size(0), self._stations(raw, num_stations)
        theta = fit.theta.to(raw.device).double().contiguous()
        if theta.shape != (max(S, 1), 2 * self.K):
            raise ValueError(f"theta must be [{max(S, 1)}, {2 * self.K}], got "
                             f"{tuple(theta.shape)}")
        if raw.on_kernel:
            pack = self._pack_hip(raw, None, S)
            pred = torch.empty(N, self.K, dtype=torch.float32, device=raw.device)
            _lib.call("gine_emos_predict", _lib.ptr(pack), _lib.ptr(theta), N, S, self.kind,
                      _lib.ptr(pred), _lib.stream_handle(raw.device))
            return pred
        z = self._predictors_torch(raw)
        th = theta[torch.arange(N, device=raw.device) % S] if S > 0 else theta.expand(N, -1)
        pred = torch.stack(self._links(self._raw(th, z)), dim=1)
        nan = torch.full_like(pred, float("nan"))
        return torch.where(torch.isnan(z[:, 0:1]), nan, pred).float()

    def forecast(self, raw: RawEnsemble, fit: EmosFit, num_stations: int | None = None):
        """:meth:`predict` as a :class:`raincast_gnn.forecast.Forecast`."""
        return Forecast(self.predict(raw, fit, num_stations), self.kind,
                        u=self.u if self.kind == _lib.LOSS_MIXED else None,
                        xi=self.xi if self.kind == _lib.LOSS_MIXED else None, c=self.c)

    # ------------------------------------------------------------------ arguments
    @staticmethod
    def _stations(raw: RawEnsemble, num_stations) -> int:
        S = 0 if num_stations is None else int(num_stations)
        if num_stations is not None and S < 1:
            raise ValueError(f"num_stations must be positive or None, got {num_stations!r}")
        if S > 0 and raw.members.size(0) % S != 0:
            raise ValueError(f"{raw.members.size(0)} rows are not a multiple of {S} stations")
        return S

    @staticmethod
    def _group_major(t: torch.Tensor, S: int) -> torch.Tensor:
        """Collated rows ``[T * S, ...]`` reordered station by station."""
        if S <= 0:
            return t
        return t.reshape(t.size(0) // S, S, *t.shape[1:]).transpose(0, 1).contiguous()

    # ------------------------------------------------------------------ HIP
    def _pack_hip(self, raw: RawEnsemble, y, S: int) -> torch.Tensor:
        mem = raw.members
        N = mem.size(0)
        pack = torch.empty(N, 4, dtype=torch.float64, device=mem.device)
        _lib.call("gine_emos_predictors", _lib.ptr(mem), mem.stride(0), mem.stride(1),
                  mem.size(1), raw.scale, raw.shift, self.c, _lib.ptr(y), N, S, _lib.ptr(pack),
                  _lib.stream_handle(mem.device))
        return pack

    def _fit_hip(self, raw: RawEnsemble, y: torch.Tensor, S: int, G: int, T: int) -> EmosFit:
        dev = raw.device
        pack = self._pack_hip(raw, y, S)
        ptr = torch.arange(G + 1, dtype=torch.int64, device=dev) * T
        return self.fit_pack(pack, ptr)

    def fit_pack(self, pack: torch.Tensor, ptr: torch.Tensor) -> EmosFit:
        """The fit kernel on a pack ``[R, 4]`` fp64 ``(mean, sd, dry, y)`` and contiguous
        segments ``ptr [G + 1]`` (int64, ``ptr[0] = 0``, non-decreasing, ``ptr[G] = R``): groups
        of any sizes.  HIP tensors only."""
        _lib.require_device(pack, "Emos.fit_pack")
        if pack.dim() != 2 or pack.size(1) != 4 or pack.dtype != torch.float64:
            raise ValueError(f"pack must be fp64 [R, 4], got {pack.dtype} {tuple(pack.shape)}")
        pack = pack.contiguous()
        ptr = ptr.to(device=pack.device, dtype=torch.int64).contiguous()
        R, G = pack.size(0), ptr.numel() - 1
        if G < 1 or int(ptr[0]) != 0 or int(ptr[-1]) != R or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError("ptr must start at 0, not decrease and end at the number of rows")
        theta = torch.empty(G, 2 * self.K, dtype=torch.float64, device=pack.device)
        report = torch.empty(G, 8, dtype=torch.float64, device=pack.device)
        _lib.call("gine_emos_fit", _lib.ptr(pack), _lib.ptr(ptr), G, R, self.kind, self.u,
                  self.xi, self.c, self.ridge, self.gtol, self.max_iter, self.min_rows,
                  _lib.ptr(theta), _lib.ptr(report), _lib.stream_handle(pack.device))
        return EmosFit(theta, report[:, 0], report[:, 1], report[:, 2], report[:, 3].long(),
                       report[:, 4].long(), report[:, 5].long(), report[:, 6].long())

    # ------------------------------------------------------------------ torch (fp64)
    def _predictors_torch(self, raw: RawEnsemble) -> torch.Tensor:
        v = raw.values()
        ok = ~torch.isnan(v)
        m = ok.sum(1).double()
        zero = torch.zeros_like(v)
        mean = torch.where(ok, v, zero).sum(1) / m
        dev = torch.where(ok, v - mean.unsqueeze(1), zero)
        sd = torch.sqrt((dev * dev).sum(1) / m)
        dry = (ok & (v <= self.c)).sum(1).double() / m
        return torch.stack([mean, sd, dry], dim=1)  # 0 / 0 = NaN without members

    def _raw(self, theta: torch.Tensor, z: torch.Tensor):
        """``raw_k = theta[..., 2k] + theta[..., 2k+1] z_k`` for ``z [..., 3]``."""
        cols = (z[..., 0], z[..., 1], z[..., 2], z[..., 1])
        return [theta[..., 2 * k] + theta[..., 2 * k + 1] * cols[k] for k in range(self.K)]

    def _links(self, raw):
        out = [raw[0], softplus(raw[1]) + LINK_EPS]
        if self.K > 2:
            out.append(torch.sigmoid(raw[2]))
        if self.K > 3:
            out.append(softplus(raw[3]) + LINK_EPS)
        return out

    def crps_rows(self, theta: torch.Tensor, z: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The closed-form CRPS of ``y [...]`` under ``pred(theta; z)`` (fp64, differentiable in
        ``theta``): ``theta [..., P]`` broadcast against ``z [..., 3]``.  Inputs must not hold
        NaN; mask rows before and after."""
        return self.crps_columns(self._links(self._raw(theta, z)), y)

    def crps_columns(self, cols, y: torch.Tensor) -> torch.Tensor:
        """The closed-form CRPS of ``y`` under the ``K`` prediction columns ``cols`` (fp64
        tensors of ``y``'s shape): the loss's form, as :mod:`raincast_gnn.forecast` restates it."""
        mu, sigma = cols[0], cols[1]
        atom, tail = self.K > 2, self.K > 3
        p = cols[2] if atom else torch.zeros_like(mu)
        r = dict(mu=mu, sigma=sigma, p=p, q=1.0 - p, atom=atom, tail=tail,
                 su=cols[3] if tail else torch.ones_like(mu), u=torch.full_like(mu, self.u))
        closed = Forecast(torch.zeros(0, self.K), self.kind,
                          u=self.u if tail else None, xi=self.xi if tail else None, c=self.c)
        return closed._crps_cpu(r, y)

    def objective(self, theta: torch.Tensor, z: torch.Tensor, y: torch.Tensor):
        """``J [G]`` and the mean CRPS ``[G]`` of ``theta [G, P]`` on the groups' rows
        ``z [G, T, 3]``, ``y [G, T]`` (fp64; a NaN in a row makes it invalid)."""
        ok = ~(torch.isnan(z[..., 0]) | torch.isnan(y))
        safe = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=z.device)
        zz = torch.where(ok.unsqueeze(-1), z, safe)
        yy = torch.where(ok, y, torch.zeros_like(y))
        rows = self.crps_rows(theta.unsqueeze(1), zz, yy)
        crps = torch.where(ok, rows, torch.zeros_like(rows)).sum(1) / ok.sum(1).double()
        d = theta - theta_start(theta.size(-1), theta.device)
        return crps + self.ridge * (d * d).sum(1), crps

    def _value_grad(self, theta, z, y):
        th = theta.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            J, crps = self.objective(th, z, y)
            (g,) = torch.autograd.grad(J.sum(), th)
        return J.detach(), crps.detach(), g

    def _fit_torch(self, z: torch.Tensor, y: torch.Tensor) -> EmosFit:
        """The optimiser of the module docstring, all groups at once: every step is taken per
        group under a mask, so a group's path is the one it would take alone."""
        dev, G, P = z.device, z.size(0), 2 * self.K
        f64 = dict(dtype=torch.float64, device=dev)
        rows = (~(torch.isnan(z[..., 0]) | torch.isnan(y))).sum(1)
        eye = torch.eye(P, **f64).expand(G, P, P)
        theta = theta_start(P, dev).expand(G, P).clone()
        H = eye.clone()
        status = torch.where(rows < self.min_rows, 3, -1)
        it = torch.zeros(G, dtype=torch.int64, device=dev)
        nev = torch.zeros_like(it)
        nan = torch.full((G,), float("nan"), **f64)

        def ended(run, J, g, it):
            gmax = g.abs().amax(1)
            conv = gmax <= self.gtol * torch.clamp(J.abs(), min=1.0)
            return torch.where(run & conv, 0, torch.where(run & (it >= self.max_iter), 1, -1)), gmax

        run = status < 0
        J, crps, g = self._value_grad(theta, z, y)
        nev += run
        st, gmax = ended(run, J, g, it)
        status = torch.where(run, st, status)
        for _ in range(self.max_iter):
            run = status < 0
            if not bool(run.any()):
                break
            d = -(H @ g.unsqueeze(2)).squeeze(2)
            gd = (g * d).sum(1)
            reset = run & ~(gd < 0)
            H = torch.where(reset.reshape(G, 1, 1), eye, H)
            d = torch.where(reset.unsqueeze(1), -g, d)
            gd = torch.where(reset, -(g * g).sum(1), gd)
            alpha = torch.ones(G, **f64)
            found = torch.zeros(G, dtype=torch.bool, device=dev)
            nt, nJ, nc, ng = theta.clone(), J.clone(), crps.clone(), g.clone()
            for _k in range(MAX_HALVINGS + 1):
                need = run & ~found
                if not bool(need.any()):
                    break
                trial = torch.where(need.unsqueeze(1), theta + alpha.unsqueeze(1) * d, theta)
                Jt, ct, gt = self._value_grad(trial, z, y)
                nev += need
                good = need & torch.isfinite(Jt) & (Jt <= J + ARMIJO * alpha * gd)
                nt = torch.where(good.unsqueeze(1), trial, nt)
                ng = torch.where(good.unsqueeze(1), gt, ng)
                nJ, nc = torch.where(good, Jt, nJ), torch.where(good, ct, nc)
                found = found | good
                alpha = torch.where(need & ~good, 0.5 * alpha, alpha)
            status = torch.where(run & ~found, 2, status)
            acc = run & found
            s, yv = nt - theta, ng - g
            theta, g, J, crps = nt, ng, nJ, nc
            it += acc
            st, gm = ended(acc, J, g, it)
            status = torch.where(acc, st, status)
            gmax = torch.where(acc, gm, gmax)
            sy = (s * yv).sum(1)
            upd = acc & (sy > CURVATURE * s.norm(dim=1) * yv.norm(dim=1))
            rho = 1.0 / torch.where(upd, sy, torch.ones_like(sy))
            Hy = (H @ yv.unsqueeze(2)).squeeze(2)
            coef = rho * rho * (yv * Hy).sum(1) + rho
            sHy = s.unsqueeze(2) * Hy.unsqueeze(1)
            Hn = H - rho.reshape(G, 1, 1) * (sHy + sHy.transpose(1, 2)) \
                + coef.reshape(G, 1, 1) * (s.unsqueeze(2) * s.unsqueeze(1))
            H = torch.where(upd.reshape(G, 1, 1), Hn, H)
        status = torch.where(status < 0, 1, status)
        few = status == 3
        return EmosFit(theta, torch.where(few, nan, J), torch.where(few, nan, crps),
                       torch.where(few, nan, gmax), it, torch.where(few, 0, nev), rows, status)
