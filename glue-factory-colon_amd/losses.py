"""Validation NLL of an assignment -- counterpart of gluefactory/models/utils/losses.py (NLLLoss), forward only.

The arithmetic runs in `gfc_lg_validation_metrics` (csrc/lg_validation.hip), which never builds the (M+1) x (N+1)
weight matrix of `nll_loss` and returns the matcher metrics of the same pair from the same launch.  The second element
of the reference's result -- that weight matrix, re-used only by the per-layer terms of the TRAINING loss -- is None here.
"""
import torch
from torch import nn

from . import _native as nat
from .base_model import merge

OUT_KEYS = ("nll_pos", "nll_neg", "num_matchable", "num_unmatchable", "assignment_nll", "row_norm", "match_recall",
            "match_precision", "accuracy", "average_precision")


def validation_metrics(log_assignment, gt_matches0, gt_matches1, gt_assignment, matches0, matching_scores0,
                       nll_balancing=0.5):
    """One call of gfc_lg_validation_metrics for B equal-sized pairs: log_assignment [B,M+1,N+1], gt_matches0 [B,M],
    gt_matches1 [B,N], gt_assignment [B,M,N] bool or None (the positives are then la[i, gt_matches0[i]]), the predicted
    matches0 / matching_scores0 [B,M] -> [B,10] float32 in OUT_KEYS order, on the device."""
    nat.require_cuda(log_assignment, "log_assignment")
    dev = log_assignment.device
    b, m, n = log_assignment.shape[0], log_assignment.shape[1] - 1, log_assignment.shape[2] - 1
    if tuple(gt_matches0.shape) != (b, m) or tuple(gt_matches1.shape) != (b, n) or tuple(matches0.shape) != (b, m) \
            or tuple(matching_scores0.shape) != (b, m):
        raise ValueError(f"log_assignment {tuple(log_assignment.shape)} does not fit gt_matches0 "
                         f"{tuple(gt_matches0.shape)}, gt_matches1 {tuple(gt_matches1.shape)}, matches0 "
                         f"{tuple(matches0.shape)}, matching_scores0 {tuple(matching_scores0.shape)}")
    if gt_assignment is not None:
        if tuple(gt_assignment.shape) != (b, m, n):
            raise ValueError(f"gt_assignment {tuple(gt_assignment.shape)} is not [{b},{m},{n}]")
        gt_assignment = gt_assignment.to(device=dev).ne(0).contiguous()
    out = torch.empty((b, len(OUT_KEYS)), dtype=torch.float32, device=dev)
    nat.call("gfc_lg_validation_metrics", log_assignment.float().contiguous(),
             gt_matches0.to(device=dev, dtype=torch.long).contiguous(),
             gt_matches1.to(device=dev, dtype=torch.long).contiguous(), gt_assignment,
             matches0.to(device=dev, dtype=torch.long).contiguous(),
             matching_scores0.to(device=dev, dtype=torch.float32).contiguous(), b, m, n, float(nll_balancing), out)
    return out


def as_dict(out, keys):
    return {k: out[:, OUT_KEYS.index(k)] for k in keys}


class NLLLoss(nn.Module):
    default_conf = {
        "nll_balancing": 0.5,
        "gamma_f": 0.0,  # focal loss: accepted and unused, as in the reference
    }

    def __init__(self, conf):
        super().__init__()
        self.conf = merge(self.default_conf, conf)

    def forward(self, pred, data, weights=None):
        """(nll [B], None, {assignment_nll, nll_pos, nll_neg, num_matchable, num_unmatchable}); `data` holds
        gt_matches0/1 and optionally gt_assignment.  A prediction without matches0 / matching_scores0 is scored as
        matching nothing (only the metrics, which this function does not return, read them)."""
        if weights is not None:
            raise NotImplementedError("NLLLoss: re-used weights belong to the per-layer training loss, which is not built")
        la = pred["log_assignment"]
        g0 = data["gt_matches0"]
        m0 = pred.get("matches0", torch.full_like(g0, -1))
        s0 = pred.get("matching_scores0", torch.zeros(g0.shape, dtype=torch.float32, device=g0.device))
        out = validation_metrics(la, g0, data["gt_matches1"], data.get("gt_assignment"), m0, s0,
                                 self.conf["nll_balancing"])
        d = as_dict(out, ("assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable"))
        return d["assignment_nll"], None, d
