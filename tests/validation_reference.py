"""Restatement of the validation pass's arithmetic with torch operations, in the dtype of its inputs (float64 for the GPU
comparison): the checker of csrc/gt_matches.hip and csrc/lg_validation.hip.

  gt_matches_homography   gt_matches_from_homography (gluefactory/geometry/gt_generation.py:730-801) of ONE pair with
                          validity masks, independent thresholds and the dense assignment / reward, plus -- like
                          tests/hpatches_reference.py, whose DELTA and warp it uses -- which verdicts are UNDECIDED: resting
                          on a decision within DELTA of going the other way, where a float32 evaluation may differ.
  validation_row          NLLLoss.forward + row_norm + matcher_metrics (models/utils/losses.py, lightglue.py:606,
                          models/utils/metrics.py) of ONE pair: the ten values of gfc_lg_validation_metrics, in float64.
  ranking_ap_closed       what metrics.py's ranking_ap sums to: p_last (r_last - r_first).

`rule=` selects a deliberately WRONG variant (WRONG_RULES); the host test shows the fixture rejects each.
"""
import torch

from hpatches_reference import DELTA, warp

WRONG_RULES = ("pos_le", "masked_negatives", "last_index_ties")
OUT_KEYS = ("nll_pos", "nll_neg", "num_matchable", "num_unmatchable", "assignment_nll", "row_norm", "match_recall",
            "match_precision", "accuracy", "average_precision")
INF = float("inf")


def _argmin(D, dim, rule):
    if rule == "last_index_ties":
        return D.shape[dim] - 1 - D.flip(dim).min(dim).indices
    return D.min(dim).indices  # first index among equals; 0 for a row of +inf


def _second(D, arg, pts, dim):
    """The smallest distance along `dim` to a candidate that is no bit-identical twin of the winner."""
    win = pts[arg]  # [rows, 2]
    twin = (pts[None] == win[:, None]).all(-1)  # [rows, candidates]
    if dim == 0:
        twin = twin.T
    return torch.where(twin, torch.full_like(D, INF), D).min(dim).values


def gt_matches_homography(kp0, kp1, H, pos_th=3.0, neg_th=3.0, valid0=None, valid1=None, rule=None, Hinv=None):
    """kp0 [M,2], kp1 [N,2], H [3,3] (M, N >= 1) -> matches0/1, proj_0to1/1to0, assignment [M,N] bool, reward [M,N],
    undecided0/1 (key points), undecided_dense [M,N] (elements of assignment / reward)."""
    M, N = kp0.shape[0], kp1.shape[0]
    if Hinv is None:
        Hinv = torch.linalg.inv(H)
    v0 = torch.ones(M, dtype=torch.bool) if valid0 is None else valid0.bool()
    v1 = torch.ones(N, dtype=torch.bool) if valid1 is None else valid1.bool()
    k01, k10 = warp(kp0, H, 1e-5), warp(kp1, Hinv, 1e-5)
    D0 = ((k01[:, None] - kp1[None]) ** 2).sum(-1)
    D1 = ((kp0[:, None] - k10[None]) ** 2).sum(-1)
    vis = v0[:, None] & v1[None]
    D = torch.where(vis, torch.maximum(D0, D1), torch.full_like(D0, INF))
    pos2, neg2 = pos_th**2, neg_th**2
    below = (D <= pos2) if rule == "pos_le" else (D < pos2)
    reward = below.to(D.dtype) - (D > neg2).to(D.dtype)
    min0, min1 = _argmin(D, 1, rule), _argmin(D, 0, rule)
    rows, cols = torch.arange(M), torch.arange(N)
    ismin0 = torch.zeros_like(vis)
    ismin1 = torch.zeros_like(vis)
    ismin0[rows, min0] = True
    ismin1[min1, cols] = True
    positive = ismin0 & ismin1 & below
    src0, src1 = (D, D) if rule == "masked_negatives" else (D0, D1)
    neg0 = (src0.min(1).values > neg2) & v0
    neg1 = (src1.min(0).values > neg2) & v1
    m0 = torch.where(positive.any(1), min0, torch.full_like(min0, -2))
    m1 = torch.where(positive.any(0), min1, torch.full_like(min1, -2))
    m0 = torch.where(neg0, torch.full_like(m0, -1), m0)
    m1 = torch.where(neg1, torch.full_like(m1, -1), m1)
    # margins
    rb, cb = D.min(1).values, D.min(0).values
    rs, cs = _second(D, min0, kp1, 1), _second(D, min1, kp0, 0)

    def near(best, second):
        return (second.sqrt() - best.sqrt() < 2 * DELTA) & (best.sqrt() < pos_th + DELTA)

    def at(d2, th):
        return (d2.sqrt() - th).abs() < DELTA

    rn, cn = near(rb, rs), near(cb, cs)
    und0 = at(rb, pos_th) | (at(D0.min(1).values, neg_th) & v0) | rn | cn[min0]
    und1 = at(cb, pos_th) | (at(D1.min(0).values, neg_th) & v1) | cn | rn[min1]
    und_dense = at(D, pos_th) | at(D, neg_th) | ((rn[:, None] | cn[None]) & (D.sqrt() < pos_th + DELTA))
    return {"matches0": m0, "matches1": m1, "proj_0to1": k01, "proj_1to0": k10, "assignment": positive,
            "reward": reward, "undecided0": und0, "undecided1": und1, "undecided_dense": und_dense}


def ranking_ap_closed(m, gt, scores):
    """m, gt [M] long, scores [M] -> p_last (r_last - r_first) as a Python float; the top element is the lowest index
    among equal maxima."""
    M = m.shape[0]
    if M == 0:
        return 0.0
    tp = m == gt
    p_mask, r_mask = (m > -1) & (gt >= -1), gt > -1
    p_last = float((tp & p_mask).sum()) / (1e-8 + float(p_mask.sum()))
    R = 1e-8 + float(r_mask.sum())
    top = int(torch.argmax(scores.double()))  # torch.argmax: the first of equal maxima
    top = int(torch.nonzero(scores == scores[top])[0])
    return p_last * (float((tp & r_mask).sum()) / R - float(tp[top] & r_mask[top]) / R)


def ranking_ap_sorted(m, gt, scores):
    """The long way round, in float64: walk the key points by falling score (a stable order), keep the running recall,
    and add every recall increment times the precision over ALL predictions -- the sum the reference's ranking_ap forms."""
    tp = m == gt
    p_mask, r_mask = (m > -1) & (gt >= -1), gt > -1
    p_last = float((tp & p_mask).sum()) / (1e-8 + float(p_mask.sum()))
    R = 1e-8 + float(r_mask.sum())
    order = sorted(range(m.shape[0]), key=lambda i: (-float(scores[i]), i))
    total, hits, previous = 0.0, 0, None
    for i in order:
        hits += int(tp[i] & r_mask[i])
        recall = hits / R
        if previous is not None:
            total += (recall - previous) * p_last
        previous = recall
    return total


def validation_row(la, gt0, gt1, gt_assignment, m0, scores0, nll_balancing=0.5):
    """la [M+1,N+1] (its own dtype; exp and sums in float64), gt0 [M], gt1 [N], gt_assignment [M,N] bool or None, the
    prediction m0 / scores0 [M] -> the ten values in OUT_KEYS order, a float64 tensor."""
    M, N = la.shape[0] - 1, la.shape[1] - 1
    L = la.double()
    if gt_assignment is not None:
        pos = gt_assignment.bool()
    else:
        pos = torch.zeros((M, N), dtype=torch.bool)
        i = torch.nonzero(gt0 > -1).flatten()
        pos[i, gt0[i]] = True
    neg0, neg1 = gt0 == -1, gt1 == -1
    num_pos = max(float(pos.sum()), 1.0)
    nn0, nn1 = max(float(neg0.sum()), 1.0), max(float(neg1.sum()), 1.0)
    nll_pos = -float(L[:M, :N][pos].sum()) / num_pos
    nll_neg = -(float(L[:M, N][neg0].sum()) + float(L[M, :N][neg1].sum())) / (nn0 + nn1)
    row_norm = float(L[:M].exp().sum(1).mean()) if M else float("nan")
    tp = m0 == gt0

    def ratio(mask):
        return float((tp & mask).sum()) / (1e-8 + float(mask.sum()))

    return torch.tensor([nll_pos, nll_neg, num_pos, (nn0 + nn1) / 2.0,
                         nll_balancing * nll_pos + (1 - nll_balancing) * nll_neg, row_norm, ratio(gt0 > -1),
                         ratio((m0 > -1) & (gt0 >= -1)), ratio(gt0 >= -1), ranking_ap_closed(m0, gt0, scores0)],
                        dtype=torch.float64)
