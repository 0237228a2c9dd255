"""Matcher metrics -- counterpart of gluefactory/models/utils/metrics.py (`matcher_metrics`), on
`gfc_lg_validation_metrics` (csrc/lg_validation.hip; the loss columns of that launch are not used here).

`average_precision` is the reference's `ranking_ap` in closed form: its sum multiplies every recall increment by the
LAST precision point, so it equals p_last * (r_last - r_first); r_first belongs to the top-scoring key point, taken as
the lowest index among equal maxima (torch.argsort is not stable, so the reference itself does not fix that choice).
"""
import torch

from .losses import as_dict, validation_metrics

KEYS = ("match_recall", "match_precision", "accuracy", "average_precision")


@torch.no_grad()
def matcher_metrics(pred, data, prefix="", prefix_gt=None):
    if prefix_gt is None:
        prefix_gt = prefix
    m0, s0 = pred[f"{prefix}matches0"], pred[f"{prefix}matching_scores0"]
    g0 = data[f"gt_{prefix_gt}matches0"]
    b, m = m0.shape
    # the metrics read no log assignment: an empty one ([B, M+1, 1], N = 0) keeps the launch to the M key points
    la = torch.zeros((b, m + 1, 1), dtype=torch.float32, device=m0.device)
    g1 = torch.empty((b, 0), dtype=torch.long, device=m0.device)
    out = validation_metrics(la, g0, g1, None, m0, s0)
    return {f"{prefix}{k}": v for k, v in as_dict(out, KEYS).items()}
