"""Float64 restatement of the reference's training-mode loss of LightGlue, written from its text:
TokenConfidence.loss (gluefactory/models/matchers/lightglue.py:82-95), the layer loop of LightGlue.loss
(lightglue.py:597-630), NLLLoss / weight_loss (models/utils/losses.py:6-73), filter_matches (lightglue.py:294-319),
matcher recall / precision (models/utils/metrics.py) and the predicate of check_if_stop (lightglue.py:577-580), plus the
per-layer report of `LightGlue.layer_loss`.  Test infrastructure: CPU torch only.

`variant` switches ONE deliberate mistake on; the host test shows that each of them misses the reference fixture.
"""
import torch

VARIANTS = ("no_dustbin", "own_matches", "bce_on_probabilities", "gamma_l_plus_1", "no_one_in_weight_sum",
            "confidence_not_averaged", "confidence_not_in_total", "joint_neg_clamp", "confident_le")


def argmax_low(x, dim):
    """Arg-max along `dim` with the lower index among equal maxima and NaN entries skipped (the rule of
    gfc_lg_layer_scores; the reference leaves ties to torch.max).  No entry above -inf: index 0."""
    x = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
    top = x.max(dim, keepdim=True).values
    shape = [1] * x.dim()
    shape[dim] = x.shape[dim]
    idx = torch.arange(x.shape[dim]).view(shape).expand_as(x)
    big = x.shape[dim]
    first = torch.where((x == top) & (top > -float("inf")), idx, torch.full_like(idx, big)).min(dim).values
    return torch.where(first == big, torch.zeros_like(first), first)


def filter_matches(la, threshold=0.0):
    """lightglue.py:294-319 -> m0 [B,M], m1 [B,N], scores0 [B,M]."""
    core = la[:, :-1, :-1]
    m0, m1 = argmax_low(core, 2), argmax_low(core, 1)
    b, m, n = core.shape
    i0, i1 = torch.arange(m)[None], torch.arange(n)[None]
    mutual0 = i0 == m1.gather(1, m0)
    mutual1 = i1 == m0.gather(1, m1)
    max0 = core.max(2).values.exp()
    zero = max0.new_tensor(0)
    s0 = torch.where(mutual0, max0, zero)
    s1 = torch.where(mutual1, s0.gather(1, m1), zero)
    valid0 = mutual0 & (s0 > threshold)
    valid1 = mutual1 & valid0.gather(1, m1)
    return torch.where(valid0, m0, -1), torch.where(valid1, m1, -1), s0


def token_targets(la_now, la_final, variant=None):
    """correct0 [B,M], correct1 [B,N] (lightglue.py:86-91): the dustbin column / row takes part in the arg-max."""
    if variant == "no_dustbin":
        r = lambda la: argmax_low(la[:, :-1, :-1], 2)
        c = lambda la: argmax_low(la[:, :-1, :-1], 1)
    else:
        r = lambda la: argmax_low(la[:, :-1, :], 2)
        c = lambda la: argmax_low(la[:, :, :-1], 1)
    if variant == "own_matches":  # against the layer's own mutual matches (unmatched = the dustbin)
        m0, m1, _ = filter_matches(la_now)
        m, n = la_now.shape[1] - 1, la_now.shape[2] - 1
        return r(la_now) == torch.where(m0 < 0, n, m0), c(la_now) == torch.where(m1 < 0, m, m1)
    return r(la_final) == r(la_now), c(la_final) == c(la_now)


def bce_with_logits(x, y):
    return x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))


def token_bce(logit0, logit1, correct0, correct1, variant=None):
    """(bce0, bce1) [B]: the two means of lightglue.py:93-94."""
    y0, y1 = correct0.to(logit0.dtype), correct1.to(logit1.dtype)
    if variant == "bce_on_probabilities":
        f = lambda x, y: bce_with_logits(torch.sigmoid(x), y)
    else:
        f = bce_with_logits
    return f(logit0, y0).mean(-1), f(logit1, y1).mean(-1)


def confident_counts(logit0, logit1, threshold, variant=None):
    """#{ !(sigmoid(logit) < threshold) } per side (lightglue.py:577-580), the sigmoid in the logits' precision."""
    p0, p1 = torch.sigmoid(logit0), torch.sigmoid(logit1)
    if variant == "confident_le":
        return (~(p0 <= threshold)).sum(-1), (~(p1 <= threshold)).sum(-1)
    return (~(p0 < threshold)).sum(-1), (~(p1 < threshold)).sum(-1)


def layer_scores(la_layer, la_final, logit0, logit1, threshold, variant=None):
    """What gfc_lg_layer_scores returns, in the inputs' precision: out [B,6] = agree0, agree1, bce0, bce1, conf0, conf1
    and correct0 / correct1."""
    c0, c1 = token_targets(la_layer, la_final, variant)
    b0, b1 = token_bce(logit0, logit1, c0, c1, variant)
    n0, n1 = confident_counts(logit0, logit1, threshold, variant)
    out = torch.stack([c0.sum(-1).to(b0.dtype), c1.sum(-1).to(b0.dtype), b0, b1, n0.to(b0.dtype), n1.to(b0.dtype)], -1)
    return out, c0, c1


def nll_weights(la, data):
    """NLLLoss.nll_loss (losses.py:62-73); without gt_assignment the positives are (i, gt_matches0[i]) where > -1."""
    g0, g1 = data["gt_matches0"], data["gt_matches1"]
    b, m, n = la.shape[0], la.shape[1] - 1, la.shape[2] - 1
    w = torch.zeros_like(la)
    if data.get("gt_assignment") is not None:
        w[:, :m, :n] = data["gt_assignment"].to(la.dtype)
    else:
        bi, ii = torch.nonzero(g0 > -1, as_tuple=True)
        w[bi, ii, g0[bi, ii]] = 1
    w[:, :m, -1] = (g0 == -1).to(la.dtype)
    w[:, -1, :n] = (g1 == -1).to(la.dtype)
    return w


def weighted_nll(la, w, balancing=0.5, variant=None):
    """weight_loss + NLLLoss.forward (losses.py:6-60) -> dict of [B] values."""
    m, n = la.shape[1] - 1, la.shape[2] - 1
    sc = la * w
    neg0, neg1 = w[:, :m, -1].sum(-1), w[:, -1, :n].sum(-1)
    if variant == "joint_neg_clamp":
        den = (neg0 + neg1).clamp(min=1.0)
    else:
        den = neg0.clamp(min=1.0) + neg1.clamp(min=1.0)
    num_pos = w[:, :m, :n].sum((-1, -2)).clamp(min=1.0)
    nll_pos = -sc[:, :m, :n].sum((-1, -2)) / num_pos
    nll_neg = (-sc[:, :m, -1].sum(-1) - sc[:, -1, :n].sum(-1)) / den
    nll = balancing * nll_pos + (1 - balancing) * nll_neg
    return {"assignment_nll": nll, "nll_pos": nll_pos, "nll_neg": nll_neg, "num_matchable": num_pos,
            "num_unmatchable": den / 2.0}


def recall_precision(m0, gt0):
    """match_recall, match_precision of metrics.py (x / (1e-8 + count))."""
    hit = (m0 == gt0).to(torch.float64)
    rec_mask = (gt0 > -1).to(torch.float64)
    prec_mask = ((m0 > -1) & (gt0 >= -1)).to(torch.float64)
    return (hit * rec_mask).sum(1) / (1e-8 + rec_mask.sum(1)), (hit * prec_mask).sum(1) / (1e-8 + prec_mask.sum(1))


def layer_loss(las, logits0, logits1, data, thresholds, gamma=1.0, balancing=0.5, filter_threshold=0.0, variant=None):
    """las: the L log assignments [B,M+1,N+1] of the layers' own heads (the last one the final assignment); logits0/1:
    the L - 1 token logits [B,M] / [B,N]; thresholds: the L - 1 confidence thresholds.  -> (losses, report, targets)
    as LightGlue.layer_loss defines them; targets = [(correct0, correct1)] per layer."""
    nl = len(las)
    b, m, n = las[0].shape[0], las[0].shape[1] - 1, las[0].shape[2] - 1
    final = las[-1]
    w = nll_weights(final, data)
    per = [weighted_nll(la, w, balancing, variant) for la in las]
    last = per[-1]
    losses = {"last": last["assignment_nll"].clone(), **last, "row_norm": final.exp()[:, :-1].sum(2).mean(1)}
    total = last["assignment_nll"]
    sum_weights = 0.0 if variant == "no_one_in_weight_sum" else 1.0
    confidence = torch.zeros_like(total)
    targets, agree, bce, ratio = [], [], [], []
    for i in range(nl - 1):
        if gamma > 0.0:
            weight = gamma ** (i + 1) if variant == "gamma_l_plus_1" else gamma ** (nl - i - 1)
        else:
            weight = i + 1
        sum_weights += weight
        total = total + per[i]["assignment_nll"] * weight
        out, c0, c1 = layer_scores(las[i], final, logits0[i], logits1[i], thresholds[i], variant)
        tc = (out[:, 2] + out[:, 3]) / 2.0
        confidence = confidence + (tc if variant == "confidence_not_averaged" else tc / (nl - 1))
        targets.append((c0, c1))
        agree.append((out[:, 0] + out[:, 1]) / (m + n))
        bce.append(tc)
        ratio.append((out[:, 4] + out[:, 5]) / (m + n))
    total = total / sum_weights
    if variant != "confidence_not_in_total":
        total = total + confidence
    losses.update(total=total, confidence=confidence)
    rp = [recall_precision(filter_matches(la, filter_threshold)[0], data["gt_matches0"]) for la in las]
    stack = lambda xs: torch.stack(xs, 1) if xs else torch.zeros((b, 0), dtype=final.dtype)
    report = {"layer_nll": stack([p["assignment_nll"] for p in per]), "layer_nll_pos": stack([p["nll_pos"] for p in per]),
              "layer_nll_neg": stack([p["nll_neg"] for p in per]), "layer_recall": stack([r for r, _ in rp]),
              "layer_precision": stack([p for _, p in rp]), "layer_agree": stack(agree), "layer_token_bce": stack(bce),
              "layer_ratio_confident": stack(ratio)}
    return losses, report, targets
