"""Inference / checkpoint-ensemble evaluation on the engine (eval.py:57-69, 153-218).

``predict_model`` runs the model in eval mode under ``no_grad`` over batches (BatchNorm from
its running statistics: the GINE layers' node MLP then takes the eval branch of
``gine_bn_fwd_finalize``) and concatenates the predictions; ``predict_ensemble`` averages
the predictions of several checkpoints (``stack(...).mean(0)``, eval.py:208-212) and
``ensemble_crps`` scores them with the model's own loss, as eval.py:216-218 does.
Checkpoints load with ``torch.load(weights_only=True)``: a state_dict is plain tensors.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable

import torch

from .data import restore_node_order


@torch.no_grad()
def predict_model(model: torch.nn.Module, batches: Iterable, device,
                  fused: bool = False) -> torch.Tensor:
    """eval.py:57-69: eval mode, one forward per batch, predictions concatenated on the CPU
    (rows in the collated order of each batch, whatever order the batch is stored in).
    ``fused``: the forward of the model's :class:`raincast_gnn.inference.Predictor` (one launch
    per GINE layer; same bits), kept on the model (``inference.predictor_for``) so that later
    calls replay what earlier ones captured.  Only batches that come back as the same
    device-resident ``edge_index`` / ``edge_attr`` tensors are replayed; host batches are new
    tensors after every ``.to(device)`` and run eager."""
    model.eval()
    if fused:
        from .inference import predictor_for
        fwd = predictor_for(model)
    else:
        fwd = model
    # batches in the engine's station order come back in the reference (collated) order
    out = [restore_node_order(fwd(b.to(device)), b).cpu() for b in batches]
    return torch.cat(out, dim=0)


def predict_ensemble(make_model, checkpoints, batches, device,
                     fused: bool = False, stack: bool = False) -> torch.Tensor:
    """eval.py:178-212: one model per checkpoint (state_dict path or dict), predictions
    averaged over checkpoints.  ``batches`` is re-iterated per checkpoint.
    ``fused``: one model and its ``Predictor`` for all checkpoints, each loaded into the model
    in place (``load_state_dict`` copies into the parameters' storage, which the captured
    forward reads).  The batches are moved to the device once, so every checkpoint sees the
    same tensors: per distinct edge list (up to the Predictor's ``max_captures``) one eager
    call and one capture, then a replay per further checkpoint.
    ``stack``: the checkpoints' predictions as they are, ``[M, N, K]``, for
    :class:`raincast_gnn.pool.ForecastPool`; the mean over parameter rows is left to the
    caller (``.mean(0)`` is the default return)."""
    batches = [b.to(device) for b in batches] if fused else list(batches)
    preds = []
    model = None
    for ck in checkpoints:
        if not fused or model is None:
            model = make_model().to(device)
        state = torch.load(ck, map_location=device, weights_only=True) if isinstance(ck, str) \
            else ck
        model.load_state_dict(state)
        preds.append(predict_model(model, batches, device, fused))
    if stack:
        return torch.stack(preds, dim=0)
    if len(preds) == 1:
        return preds[0]
    return torch.stack(preds, dim=0).mean(dim=0)


def ensemble_crps(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor):
    """eval.py:216-218: the CRPS of the averaged predictions under the model's loss."""
    return model.loss_fn.crps(preds, targets)


def verify(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor, thresholds,
           unit: str = "mm"):
    """Verification of the predictions as forecasts (:mod:`raincast_gnn.forecast`): per-row
    CRPS and PIT interval, and the Brier score of exceeding each threshold (``unit``: the
    thresholds', millimetres by default; the targets are the dataset's ``log(mm + 0.01)``).
    On a HIP device one launch; returns a :class:`raincast_gnn.forecast.ForecastScore`."""
    from .forecast import Forecast
    return Forecast.from_model(model, preds).score(targets, thresholds, unit=unit)


@dataclass
class PoolVerification:
    """What :func:`verify_pool` returns.  ``pool``: the :class:`raincast_gnn.pool.PoolScore` of
    the linear pool; ``average``: the :class:`raincast_gnn.forecast.ForecastScore` of the
    parameter average (what :func:`verify` gives for ``stacked.mean(0)``); the means over the
    valid rows obey ``pool_crps = member_crps - diversity``."""
    pool: object
    average: object
    pool_crps: torch.Tensor
    average_crps: torch.Tensor
    member_crps: torch.Tensor
    diversity: torch.Tensor


def verify_pool(model: torch.nn.Module, stacked: torch.Tensor, targets: torch.Tensor, thresholds,
                unit: str = "mm", weights=None) -> PoolVerification:
    """The checkpoints' forecasts ``stacked [M, N, K]`` (``predict_ensemble(..., stack=True)``)
    scored as their linear pool (:mod:`raincast_gnn.pool`) beside the parameter average: the
    two scores, the mean CRPS of each, the weighted mean member CRPS and the mean diversity
    over the rows with a target."""
    from .forecast import Forecast
    from .pool import ForecastPool
    pool = ForecastPool.from_model(model, stacked, weights=weights).score(targets, thresholds,
                                                                          unit=unit)
    average = Forecast.from_model(model, stacked.mean(dim=0)).score(targets, thresholds,
                                                                    unit=unit)
    ok = ~torch.isnan(pool.crps_rows)
    diversity = torch.where(ok, pool.diversity_rows, torch.zeros_like(pool.diversity_rows)).sum() \
        / pool.valid[0]
    member = torch.nansum(pool.member_crps_rows) / pool.valid[0]
    return PoolVerification(pool, average, pool.crps, average.crps, member, diversity)


def fit_pool(model: torch.nn.Module, stacked: torch.Tensor, targets: torch.Tensor, folds=5):
    """The weights of minimum mean CRPS for the linear pool of ``stacked [M, N, K]`` on the rows
    with a target, cross-validated over ``folds`` contiguous blocks of rows
    (:meth:`raincast_gnn.pool.ForecastPool.fit_weights`).  Returns the
    :class:`raincast_gnn.pool.PoolFit` and the pool under the fitted weights (the members of
    weight 0 dropped)."""
    from .pool import ForecastPool
    pool = ForecastPool.from_model(model, stacked)
    fit = pool.fit_weights(targets, folds=folds)
    return fit, pool.reweighted(fit.weights)


@dataclass
class EnsembleVerification:
    """What :func:`verify_against_ensemble` returns; unpacks as ``(forecast, ensemble,
    crpss)``.  The two mean CRPS values and ``crpss`` are over ``valid`` rows: those with a
    target and at least one raw member (the rows both scores cover)."""
    forecast: object
    ensemble: object
    crpss: torch.Tensor
    model_crps: torch.Tensor
    ensemble_crps: torch.Tensor
    valid: torch.Tensor

    def __iter__(self):
        return iter((self.forecast, self.ensemble, self.crpss))


def verify_against_ensemble(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor,
                            raw, thresholds, unit: str = "mm") -> EnsembleVerification:
    """:func:`verify` beside the raw ensemble's own scores (``raw``: a
    :class:`raincast_gnn.ensemble.RawEnsemble` of the same rows) and the skill score
    ``CRPSS = 1 - CRPS_model / CRPS_ensemble``, both means over the rows valid in both."""
    from .ensemble import skill
    fs = verify(model, preds, targets, thresholds, unit=unit)
    es = raw.score(targets, thresholds, unit=unit)
    both = ~torch.isnan(fs.crps_rows) & ~torch.isnan(es.crps_rows)
    count = both.sum().double()
    zero = torch.zeros_like(fs.crps_rows)
    model_crps = torch.where(both, fs.crps_rows, zero).sum() / count
    ens_crps = torch.where(both, es.crps_rows, zero).sum() / count
    return EnsembleVerification(fs, es, skill(model_crps, ens_crps), model_crps, ens_crps, count)


def fit_emos(model: torch.nn.Module, raw_train, y_train: torch.Tensor, num_stations=None, **kw):
    """The EMOS baseline of the model's own distribution, fitted per station by minimum CRPS on
    the training rows (``raw_train``: a :class:`raincast_gnn.ensemble.RawEnsemble`, rows in
    collated order; ``num_stations=None``: one global parameter set).  Keywords go to
    :class:`raincast_gnn.emos.Emos` (``ridge``, ``gtol``, ``max_iter``, ``min_rows``).  Returns
    the :class:`raincast_gnn.emos.EmosFit`."""
    from .emos import Emos
    return Emos.from_model(model, **kw).fit(raw_train, y_train, num_stations)


@dataclass
class EmosVerification:
    """What :func:`verify_against_emos` returns; unpacks as ``(forecast, emos, crpss)``.
    ``forecast`` / ``emos``: the :class:`raincast_gnn.forecast.ForecastScore` of the model and
    of EMOS on the same rows; the two mean CRPS values and ``crpss = 1 - model / emos`` are
    over the ``valid`` rows (a value in both); ``model_rows`` / ``emos_rows`` are the two
    ``crps_rows`` on one device, as :func:`compare` takes them."""
    forecast: object
    emos: object
    crpss: torch.Tensor
    model_crps: torch.Tensor
    emos_crps: torch.Tensor
    valid: torch.Tensor
    model_rows: torch.Tensor
    emos_rows: torch.Tensor

    def __iter__(self):
        return iter((self.forecast, self.emos, self.crpss))


def verify_against_emos(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor, raw,
                        fit, num_stations, thresholds, unit: str = "mm") -> EmosVerification:
    """:func:`verify` beside the same scores of the EMOS baseline ``fit`` (:func:`fit_emos`, on
    training rows) applied to ``raw``, the raw ensemble of the rows of ``preds``, and the skill
    ``CRPSS = 1 - CRPS_model / CRPS_emos`` over the rows valid in both: the skill that says
    something, the raw ensemble being uncalibrated."""
    from .emos import Emos
    from .ensemble import skill
    fs = verify(model, preds, targets, thresholds, unit=unit)
    es = Emos.from_model(model).forecast(raw, fit, num_stations).score(targets, thresholds,
                                                                       unit=unit)
    er = es.crps_rows.to(fs.crps_rows.device)
    both = ~torch.isnan(fs.crps_rows) & ~torch.isnan(er)
    count = both.sum().double()
    zero = torch.zeros_like(fs.crps_rows)
    model_crps = torch.where(both, fs.crps_rows, zero).sum() / count
    emos_crps = torch.where(both, er, zero).sum() / count
    return EmosVerification(fs, es, skill(model_crps, emos_crps), model_crps, emos_crps, count,
                            fs.crps_rows, er)


@dataclass
class FieldVerification:
    """What :func:`verify_fields` returns: the :class:`raincast_gnn.fields.FieldScore` of the
    model's ECC members and of the raw ensemble, and the skills ``1 - model / ensemble`` of the
    mean energy score, the mean variogram score and the mean area CRPS, each mean over the
    ``valid`` graphs (those with a value in both)."""
    model: object
    ensemble: object
    energy_skill: torch.Tensor
    variogram_skill: torch.Tensor
    area_skill: torch.Tensor
    valid: torch.Tensor


def verify_fields(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor, raw, ptr,
                  p: float = 0.5, levels: str = "uniform",
                  stat: str = "max") -> FieldVerification:
    """The model's predictions as fields beside the raw ensemble's: the predictive distribution
    turned back into members by ECC (``Forecast.ecc(raw, levels)``), both sets of members
    scored per graph of ``ptr`` (``GraphBatch.ptr``) by :class:`raincast_gnn.fields.MemberFields`
    -- energy score, variogram score of order ``p``, CRPS of the area ``stat`` in mm -- and the
    three skills, means over the graphs valid in both as :func:`verify_against_ensemble` does
    per row."""
    from .ensemble import skill
    from .fields import MemberFields
    from .forecast import Forecast
    members = Forecast.from_model(model, preds).ecc(raw, levels=levels)
    y = targets.to(raw.device)
    raw_fields = MemberFields.from_raw(raw, torch.as_tensor(ptr).to(raw.device))
    es = raw_fields.score(y, p=p, stat=stat)
    ms = raw_fields.with_members(members).score(y, p=p, stat=stat)

    def mean_skill(a, b):
        b = b.to(a.device)
        both = ~torch.isnan(a) & ~torch.isnan(b)
        zero = torch.zeros_like(a)
        count = both.sum().double()
        return skill(torch.where(both, a, zero).sum() / count,
                     torch.where(both, b, zero).sum() / count), count

    energy, valid = mean_skill(ms.es, es.es)
    vario, _ = mean_skill(ms.vs, es.vs)
    area, _ = mean_skill(ms.area.crps, es.area.crps)
    return FieldVerification(ms, es, energy, vario, area, valid)


def feature_importance(model: torch.nn.Module, dataset, **kw):
    """Which inputs the model uses: the permutation importance of each feature group of
    ``dataset`` (a :class:`raincast_gnn.batching.DeviceDataset`) in CRPS, and in twCRPS with
    ``thresholds``; :func:`raincast_gnn.importance.permutation_importance` with its keywords."""
    from .importance import permutation_importance
    return permutation_importance(model, dataset, **kw)


def compare(model_rows: torch.Tensor, other_rows: torch.Tensor, num_stations: int, **kw):
    """Is the difference between two sets of per-row scores more than noise?  ``[N]`` rows in
    collated order (what :func:`predict_model` returns; ``N = days * num_stations``), e.g. the
    ``crps_rows`` of :func:`verify` beside the raw ensemble's, or ``[N, K]`` rows with one
    comparison per column (the twCRPS rows of ``K`` thresholds, read in place): skill and mean
    difference overall and per station, moving-block bootstrap intervals and Diebold-Mariano
    tests; :func:`raincast_gnn.compare.compare` with its keywords."""
    from .compare import compare as paired
    return paired(model_rows, other_rows, num_stations, **kw)


@dataclass
class TwVerification:
    """What :func:`verify_tw` returns, per threshold: the model's and the raw ensemble's mean
    twCRPS over the ``valid`` rows (those with a value in both), and the skill
    ``1 - model / ensemble``; ``thresholds`` in model space."""
    model: torch.Tensor
    ensemble: torch.Tensor
    skill: torch.Tensor
    valid: torch.Tensor
    thresholds: torch.Tensor


def verify_tw(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor, raw, thresholds,
              unit: str = "mm") -> TwVerification:
    """The threshold-weighted CRPS of the predictions beside the raw ensemble's (``raw``: a
    :class:`raincast_gnn.ensemble.RawEnsemble` of the same rows) at each threshold (``unit``:
    millimetres by default), and the skill ``1 - model / ensemble``: how much better than the
    ensemble the model is above the threshold.  Means over the rows valid in both, as
    :func:`verify_against_ensemble`."""
    from .ensemble import skill
    from .forecast import Forecast
    ft = Forecast.from_model(model, preds).twcrps(targets, thresholds, unit=unit, rows=True)
    et = raw.twcrps(targets.to(raw.device), thresholds, unit=unit)
    er = et.rows.to(ft.rows.device)
    both = ~torch.isnan(ft.rows) & ~torch.isnan(er)
    count = both.sum(0).double()
    zero = torch.zeros_like(ft.rows)
    m = torch.where(both, ft.rows, zero).sum(0) / count
    e = torch.where(both, er, zero).sum(0) / count
    return TwVerification(m, e, skill(m, e), count, ft.thresholds)


@dataclass
class ReliabilityVerification:
    """What :func:`verify_reliability` returns for one forecast: the
    :class:`raincast_gnn.reliability.Reliability`, its fit and, with ``replicates > 0``, its
    consistency bands (else None)."""
    reliability: object
    fit: object
    bands: object


def verify_reliability(model: torch.nn.Module, preds: torch.Tensor, targets: torch.Tensor,
                       thresholds, raw=None, unit: str = "mm", levels: int = 1000,
                       raw_levels: int | None = None, replicates: int = 1000, seed: int = 0,
                       level: float = 0.9, max_bytes: int = 256 << 20):
    """Reliability of the predictions' exceedance probabilities at ``thresholds`` (``unit``:
    millimetres by default): the CORP curve, the Brier score split into MCB, DSC and UNC, the
    AUC, and with ``replicates > 0`` the consistency band at ``level`` and the Monte-Carlo
    p-value (:mod:`raincast_gnn.reliability`).  With ``raw`` (a
    :class:`raincast_gnn.ensemble.RawEnsemble` of the same rows) returns ``(model, ensemble)``,
    the ensemble's frequencies on a lattice of ``raw_levels`` steps (its member count by
    default)."""
    from .forecast import Forecast

    def one(rel):
        bands = rel.resample(replicates, seed=seed, level=level,
                             max_bytes=max_bytes) if replicates > 0 else None
        return ReliabilityVerification(rel, rel.fit(), bands)

    mine = one(Forecast.from_model(model, preds).reliability(targets, thresholds, unit=unit,
                                                             levels=levels))
    if raw is None:
        return mine
    return mine, one(raw.reliability(targets.to(raw.device), thresholds, unit=unit,
                                     levels=raw_levels))
