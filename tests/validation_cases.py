"""Inputs of the validation-pass tests, shared by tests/golden/make_golden_validation.py (which runs the reference on
them) and the tests (which read the reference's answers from tests/golden/validation.npz).  Everything that is cheap to
rebuild bit for bit is built here from integers; only what came out of a random generator is stored in the fixture.
"""
import numpy as np
import torch

LA_SCALE = 64.0  # log assignments of the loss cases are multiples of 1/64 in [-16, 0]: stored as int16


def loss_case(seed, m, n, kind="plain"):
    """One pair for the loss / metrics: la_q [m+1,n+1] int16 (log assignment = la_q / 64), gt0 [m], gt1 [n], assignment
    [m,n] bool, the prediction m0 [m] / scores0 [m].  The ground truth is a random partial permutation (about 40 %
    matched, the rest unmatched or ignored in equal parts); the prediction repeats it with every 5th row dropped and
    every 7th moved to another column; scores are distinct multiples of 2^-12, so the top score is unique.
    kind: plain / nopos (no positive) / noneg (no negative on either side) / allignore / nopred (no predicted match)."""
    g = torch.Generator().manual_seed(seed)
    la_q = torch.clamp((torch.randn((m + 1, n + 1), generator=g) * 2 - 3) * LA_SCALE, -16 * LA_SCALE, 0).round().to(torch.int16)
    k = int(0.4 * min(m, n)) if kind == "plain" or kind == "noneg" or kind == "nopred" else 0
    if min(m, n) == 1 and kind == "plain":
        k = 1
    rows, cols = torch.randperm(m, generator=g)[:k], torch.randperm(n, generator=g)[:k]
    fill = {"noneg": (-2, -2), "allignore": (-2, -2)}.get(kind)
    gt0 = torch.full((m,), -2, dtype=torch.long)
    gt1 = torch.full((n,), -2, dtype=torch.long)
    if fill is None:
        gt0[torch.rand(m, generator=g) < 0.5] = -1
        gt1[torch.rand(n, generator=g) < 0.5] = -1
    gt0[rows], gt1[cols] = cols, rows
    assignment = torch.zeros((m, n), dtype=torch.bool)
    assignment[rows, cols] = True
    m0 = gt0.clone()
    m0[m0 == -2] = -1
    extra = torch.nonzero(gt0 < 0).flatten()[::3]  # a third of the unmatchable rows get a (wrong) prediction
    m0[extra] = torch.randint(0, n, (len(extra),), generator=g)
    m0[::5] = -1
    m0[1::7] = torch.where(m0[1::7] > -1, (m0[1::7] + 1) % n, m0[1::7])
    if kind == "nopred":
        m0[:] = -1
    scores0 = (torch.randperm(4095, generator=g)[:m] + 1).float() / 4096.0
    scores0[m0 < 0] = 0.0
    return {"la_q": la_q, "gt0": gt0, "gt1": gt1, "assignment": assignment, "m0": m0, "scores0": scores0}


def la_of(la_q):
    return torch.as_tensor(la_q).float() / LA_SCALE


LOSS_CASES = (("1x1", 1, 1, "plain"), ("131x68", 131, 68, "plain"), ("nopos", 131, 68, "nopos"),
              ("noneg", 131, 68, "noneg"), ("allignore", 131, 68, "allignore"), ("nopred", 131, 68, "nopred"),
              ("300x257", 300, 257, "plain"))


def ap_cases(seed=3):
    """Small inputs of ranking_ap: (name, m [M], gt [M], scores [M]).  Random ones of several lengths with distinct
    scores, and the degenerate ones: one key point, no score above zero, everything ignored, nothing matchable, the top
    score a true / a false positive, a top score on an unmatched prediction."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for M in (1, 2, 3, 17, 40, 40):
        gt = torch.randint(-2, max(M // 2, 1), (M,), generator=g)
        m = torch.where(torch.rand(M, generator=g) < 0.6, gt.clamp(min=-1), torch.randint(-1, max(M // 2, 1), (M,), generator=g))
        s = (torch.randperm(4095, generator=g)[:M] + 1).float() / 4096.0
        s[m < 0] = 0.0
        out.append((f"random{len(out)}_{M}", m, gt, s))
    m, gt, s = (t.clone() for t in out[-1][1:])
    out.append(("zero_scores", torch.full_like(m, -1), gt, torch.zeros_like(s)))  # no score above zero: no prediction
    out.append(("all_ignore", m, torch.full_like(gt, -2), s))
    out.append(("none_matchable", m, torch.full_like(gt, -1), s))
    top_tp, top_fp = m.clone(), m.clone()
    i = int(torch.argmax(s))
    gt_tp = gt.clone()
    gt_tp[i] = top_tp[i] = 5
    out.append(("top_true_positive", top_tp, gt_tp, s))
    top_fp[i] = 4
    out.append(("top_false_positive", top_fp, gt_tp, s))
    s2 = s.clone()
    j = int(torch.nonzero(m < 0)[0])
    s2[j] = 1.0
    out.append(("top_unmatched", m, gt, s2))
    return out


def descriptors_for(kp, partner=None, seed=0):
    """Unit 256-d descriptors that are a smooth function of position (so that true correspondences look alike):
    normalised cos(kp @ W + phase) with W, phase from integers.  partner [K,2]: positions to describe instead."""
    rs = np.random.RandomState(seed)
    W = torch.from_numpy(rs.randint(-40, 41, size=(2, 256)).astype(np.float64)) / 4096.0
    phase = torch.from_numpy(rs.randint(0, 64, size=(256,)).astype(np.float64)) / 10.0
    p = (kp if partner is None else partner).double()
    d = torch.cos(p @ W + phase)
    return torch.nn.functional.normalize(d, dim=-1).float()
