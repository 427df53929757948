"""Generate tests/golden/reference_crps_rows.npz from the REFERENCE's own losses.

Run in the build container only (needs /root/reference; the GPU box does not have it):
    python tests/golden/make_reference_crps_rows.py

Imports models/loss.py and models/model_utils.py (PostProcess) from /root/reference, as
make_reference_heads.py does, and stores, for 257 seeded rows per kind, the post-processed
parameters, the targets and the reference's per-row CRPS (reduce=False):
    normal        crps_no_avg
    normal_mixed  MixedNormalCRPS(reduce=False)
    mixed         MixedLoss(grad_u=False, u=1.71, xi=0.5, reduce=False)
    mixed_u       MixedLoss(grad_u=False, u=float(u_i), xi=0.5, reduce=False), one call per row
                  (the CRPS of the row's distribution; grad_u=True would blend with a sigmoid)
Targets: about half at the censoring point, about 5 % NaN (NaN rows: NaN stored).  Two
evaluations of the same reference code are kept:
    {name}_crps    on the fp32 tensors a model hands over (pp, y as float32): what a user of
                   the reference gets, with its fp32 sub-expressions
    {name}_crps64  on the same numbers as float64 (pp.double(), y64): the reference's closed
                   form without rounding noise, for the quadrature check of the distribution.
                   y64 holds log(0.01) itself on the censored rows (its float32 image, which
                   {name}_y holds, lies 6.4e-8 below: below the distribution's support)
Nothing from the reference is copied; only these numbers are committed.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("RAINCAST_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_crps_rows.npz")

CASES = [  # (name, loss, grad_u string as in params.json, out_channels)
    ("normal", "NormalCRPS", "False", 2),
    ("normal_mixed", "MixedNormalCRPS", "False", 3),
    ("mixed", "MixedLoss", "False", 4),
    ("mixed_u", "MixedLoss", "True", 5),
]
U_FIXED, XI = 1.71, 0.5


def main():
    sys.path.insert(0, REF)
    from models.loss import MixedLoss, MixedNormalCRPS, crps_no_avg  # noqa: E402
    from models.model_utils import PostProcess  # noqa: E402

    c = float(np.log(0.01))
    g = torch.Generator().manual_seed(4321)
    n = 257
    arrays = {}
    for name, loss, grad_u, out in CASES:
        raw = torch.randn(n, out, generator=g, dtype=torch.float32)
        raw[:, 0] = raw[:, 0] * 2.0 - 1.0                     # mu spread around log-space
        censored = torch.rand(n, generator=g) < 0.5
        wet = (torch.randn(n, generator=g) * 1.5 + 0.5).to(torch.float32).clamp_min(-4.0)
        y = torch.where(censored, torch.full((n,), c), wet).to(torch.float32)
        y64 = torch.where(censored, torch.full((n,), c, dtype=torch.float64), wet.double())
        missing = torch.rand(n, generator=g) < 0.05
        y[missing] = float("nan")
        y64[missing] = float("nan")
        with torch.no_grad():
            pp = PostProcess(loss, grad_u)(raw)
        ok = ~missing

        def rows(pred, yy):
            pred, yy = pred[ok], yy[ok]
            if loss == "NormalCRPS":
                return crps_no_avg(pred, yy)
            if loss == "MixedNormalCRPS":
                return MixedNormalCRPS(reduce=False).crps(pred, yy)
            if grad_u == "False":
                return MixedLoss(grad_u=False, u=U_FIXED, xi=XI, reduce=False).crps(pred, yy)
            vals = [MixedLoss(grad_u=False, u=float(pred[i, 4]), xi=XI, reduce=False)
                    .crps(pred[i:i + 1, :4], yy[i:i + 1]) for i in range(pred.size(0))]
            return torch.cat(vals)

        for key, pred, yy in (("crps", pp, y), ("crps64", pp.double(), y64)):
            full = np.full(n, np.nan)
            full[ok.numpy()] = rows(pred, yy).reshape(-1).double().numpy()
            arrays[f"{name}_{key}"] = full
        arrays[f"{name}_pp"] = pp.numpy()
        arrays[f"{name}_y"] = y.numpy()
        arrays[f"{name}_y64"] = y64.numpy()
        if loss == "MixedLoss":
            u_row = pp[:, 4].double() if grad_u == "True" else \
                torch.full((n,), float(np.float32(U_FIXED)), dtype=torch.float64)
            above = int((ok & (y64 > u_row)).sum())
            assert above >= 20, (name, above)
            print(f"{name}: {above} valid rows with y > u")
    arrays["u_fixed"] = np.array([U_FIXED])
    arrays["xi"] = np.array([XI])
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
