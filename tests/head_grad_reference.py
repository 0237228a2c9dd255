"""Float64 closed form of the gradients of LightGlue's training loss with respect to its assignment heads and exit
tokens, and of the direct gradient at every layer's descriptors (the trunk not followed), written from the reference's
text: MatchAssignment and sigmoid_log_double_softmax (gluefactory/models/matchers/lightglue.py:257-288), NLLLoss /
weight_loss (models/utils/losses.py:6-73), TokenConfidence.loss (lightglue.py:82-95) and the layer loop of
LightGlue.loss (lightglue.py:597-630).  Test infrastructure: CPU torch only.  No autograd: the host test holds the
closed form to the reference's own autograd (tests/golden/head_grad*.npz).

One layer, one pair, d = 256, s = d^-1/4; lambda = nll_balancing; g = grad_total[b] w_l / sum_w:
    md0 = s (x0 Wf^T + bf)         S = md0 md1^T          z0 = x0 . wm + bm
    W, n0, n1, P, Q, r_i, c_j       the labels (include/gfc_amd_head_backward.h states them)
    a = g lambda / P                c = g (1 - lambda) / Q
    G_ij  = a (r_i softmax_row(S)_ij + c_j softmax_col(S)_ij - 2 W_ij)
    dz0_i = -a r_i sigmoid(-z0_i) + c n0_i sigmoid(z0_i)
    dmd0 = G md1, dmd1 = G^T md0, dWf = s (dmd0^T x0 + dmd1^T x1), dbf = s sum_rows(dmd0, dmd1)
    dwm = sum dz x, dbm = sum dz, dx0 = s dmd0 Wf + dz0 (x) wm
Token of layer l < L - 1: dlogit0_i = grad_total[b] (sigmoid(logit0_i) - correct0_i) / (2 M (L - 1)), dlogit1_j with N.

Beside every output element stands its ABS-SUM: the sum of the absolute values of the terms added into it.  The factors
of a term enter with their float64 magnitudes (|md|, |x|, |Wf|, the soft-max and sigmoid values): the analysis is of
first order, a computed factor carries a relative error that `c` counts.  Where a term is itself a sum of terms of both
signs (dmd = G md), its abs-sum is carried on instead of its magnitude (abs(dmd) = abs(G) |md|, abs(dWf) = s abs(dmd)^T
|x|).  A soft-max factor is multiplied by (1 + abs(S_ij) + max abs(S)) with abs(S_ij) = sum_k |md0_ik md1_jk| and the
maximum taken along the soft-max's line, a sigmoid by (1 + abs(z)): the relative error of exp equals the absolute
error of its argument, and S_ij and the log-sum-exp of its line each carry an error proportional to those sums.  An
fp32 evaluation in another order differs from the float64 value by at most  c * 2^-23 * abs-sum  per element, where c
counts the roundings along the deepest chain into that element (`head_c`, `token_c`).

Derivation of c.  The rounding error of a sum of K terms evaluated in fp32 grows like sqrt(K) u times its abs-sum
when the terms share a sign and stays near u times it when they do not (the random-walk model of rounding: Higham &
Mary, SIAM J. Sci. Comput. 41 (2019), A2815; u = 2^-24).  In units of 2^-23 = 2 u a chain of length K is charged
E(K) = sqrt(K) + 1, twice the same-sign estimate, for either kind:
    md   = E(256) + 2                       (bias, the scale is a power of two)                        e_md  = 19
    S    = 2 e_md + E(256)                  (both factors computed, one chain of 256)                  e_S   = 55
    z    = E(256) + 1                                                                                  e_z   = 18
    G    = e_S + E(max(M, N)) + 8           (the log-sum-exp's sum, its log, the subtraction, exp, the
                                             products with r / c and a, the sum of three terms)        e_G
    dz   = e_z + 8                          (exp, the division, the products, the sum of two terms)    e_dz
    dmd0 = e_G + e_md + E(N), dmd1 = e_G + e_md + E(M)
    dWf, dbf = max(dmd0, dmd1) + E(B max(M, N)) + 2
    dwm, dbm = e_dz + E(B (M + N)) + 2
    dx   = max(dmd0, dmd1) + e_dz + E(256) + 4
    token weight / bias = e_z + 8 + E(B (M + N)) + 2
c is a function of the shape alone; it is not fitted to any result.

`variant` switches ONE deliberate mistake on; the host test shows that each of them misses a bound by 100 x or more.
"""
import math

import torch

import layer_loss_reference as lr

U = 2.0 ** -23
D = 256
VARIANTS = ("w_factor_1", "row_softmax_only", "p_unclamped", "q_unclamped", "q_half", "gamma_l_plus_1", "sigma_sign",
            "token_mean_m_plus_n", "s_once", "minus2_negative", "r_binary", "dwf_transposed")


def _e(k):
    return math.sqrt(k) + 1.0


def head_c(b, m, n):
    """{output: c} of one head for B pairs of M + N points, as derived in the module docstring."""
    e_md, e_z = _e(D) + 2, _e(D) + 1
    e_s = 2 * e_md + _e(D)
    e_g = e_s + _e(max(m, n)) + 8
    e_dz = e_z + 8
    dmd = max(e_g + e_md + _e(n), e_g + e_md + _e(m))
    red = dmd + _e(b * max(m, n)) + 2
    vec = e_dz + _e(b * (m + n)) + 2
    return {"dWf": red, "dbf": red, "dwm": vec, "dbm": vec, "dx": dmd + e_dz + _e(D) + 4}


def token_c(b, m, n):
    return _e(D) + 1 + 8 + _e(b * (m + n)) + 2


def trunk_c(nl):
    """What a comparison ACROSS two evaluations of the trunk adds to c (the reference's float32 run, or the GPU's
    descriptors against the reference's float64 gradients): the descriptors of the last layer have passed 2 L residual
    blocks, each a chain of four matrix products of length 256 to 512, a soft-max and a LayerNorm -- 4 E(512) + 2 E(256)
    + 32, about 160 units -- whose errors add as independent terms over the blocks.  About 680 for L = 9."""
    return (4 * _e(512) + 2 * _e(D) + 32) * math.sqrt(2 * nl)


def layer_weights(nl, gamma, variant=None):
    """w_l / sum_w for l = 0 .. L - 1 (lightglue.py:597,611-626): the last layer has weight 1."""
    w = []
    for i in range(nl - 1):
        if gamma > 0.0:
            w.append(gamma ** (i + 1) if variant == "gamma_l_plus_1" else gamma ** (nl - i - 1))
        else:
            w.append(float(i + 1))
    w.append(1.0)
    total = sum(w)
    return [x / total for x in w]


def labels(gt0, gt1, gta, n, variant=None):
    """W [B,M,N], n0 [B,M], n1 [B,N] in float64."""
    b, m = gt0.shape
    if gta is not None:
        w = gta.ne(0).double()
    else:
        w = torch.zeros((b, m, n), dtype=torch.float64)
        bi, ii = torch.nonzero((gt0 > -1) & (gt0 < n), as_tuple=True)
        w[bi, ii, gt0[bi, ii]] = 1.0
    if variant == "minus2_negative":
        return w, (gt0 < 0).double(), (gt1 < 0).double()
    return w, (gt0 == -1).double(), (gt1 == -1).double()


def head_forward(x0, x1, wf, bf, wm, bm):
    """The log assignment [B,M+1,N+1] of one head in the precision of its inputs."""
    s = D ** -0.25
    md0, md1 = s * (x0 @ wf.t() + bf), s * (x1 @ wf.t() + bf)
    sim = md0 @ md1.transpose(1, 2)
    z0, z1 = x0 @ wm + bm, x1 @ wm + bm
    b, m, n = sim.shape
    la = sim.new_zeros((b, m + 1, n + 1))
    ls = torch.nn.functional.logsigmoid
    la[:, :m, :n] = 2 * sim - torch.logsumexp(sim, 2, keepdim=True) - torch.logsumexp(sim, 1, keepdim=True) \
        + ls(z0)[:, :, None] + ls(z1)[:, None, :]
    la[:, :m, n] = ls(-z0)
    la[:, m, :n] = ls(-z1)
    return la


def head_grad(x0, x1, wf, bf, wm, bm, gt0, gt1, gta, g, lam=0.5, variant=None):
    """x0 [B,M,256], x1 [B,N,256], wf [256,256], bf [256], wm [256], bm scalar tensor, g [B], all float64.
    -> (grads, abs_sums), each {dWf, dbf, dwm, dbm, dx0 [B,M,256], dx1 [B,N,256]}."""
    s = D ** -0.25
    b, m, _ = x0.shape
    n = x1.shape[1]
    w, n0, n1 = labels(gt0, gt1, gta, n, variant)
    r, c = w.sum(2), w.sum(1)
    if variant == "r_binary":
        r, c = r.clamp(max=1.0), c.clamp(max=1.0)
    p_sum, q0, q1 = w.sum((1, 2)), n0.sum(1), n1.sum(1)
    big_p = p_sum if variant == "p_unclamped" else p_sum.clamp(min=1.0)
    big_q = (q0 + q1) if variant == "q_unclamped" else q0.clamp(min=1.0) + q1.clamp(min=1.0)
    if variant == "q_half":
        big_q = big_q / 2.0
    a = (g * lam / big_p)[:, None, None]
    cq = (g * (1.0 - lam) / big_q)[:, None]
    ax0, ax1, awf = x0.abs(), x1.abs(), wf.abs()

    md0, md1 = s * (x0 @ wf.t() + bf), s * (x1 @ wf.t() + bf)
    amd0, amd1 = md0.abs(), md1.abs()
    sim = md0 @ md1.transpose(1, 2)
    asim = amd0 @ amd1.transpose(1, 2)
    z0, z1 = x0 @ wm + bm, x1 @ wm + bm
    az0, az1 = z0.abs(), z1.abs()
    pr = torch.softmax(sim, 2)
    pc = torch.zeros_like(pr) if variant == "row_softmax_only" else torch.softmax(sim, 1)
    two = 1.0 if variant == "w_factor_1" else 2.0
    big_g = a * (r[:, :, None] * pr + c[:, None, :] * pc - two * w)
    top_r, top_c = asim.max(2, keepdim=True).values, asim.max(1, keepdim=True).values
    abig_g = a.abs() * (r[:, :, None] * pr * (1 + asim + top_r) + c[:, None, :] * pc * (1 + asim + top_c) + 2.0 * w)
    sig = torch.sigmoid
    if variant == "sigma_sign":
        dz0 = -a[:, :, 0] * r * sig(z0) + cq * n0 * sig(-z0)
        dz1 = -a[:, :, 0] * c * sig(z1) + cq * n1 * sig(-z1)
    else:
        dz0 = -a[:, :, 0] * r * sig(-z0) + cq * n0 * sig(z0)
        dz1 = -a[:, :, 0] * c * sig(-z1) + cq * n1 * sig(z1)
    adz0 = (a[:, :, 0].abs() * r * sig(-z0) + cq.abs() * n0 * sig(z0)) * (1 + az0)
    adz1 = (a[:, :, 0].abs() * c * sig(-z1) + cq.abs() * n1 * sig(z1)) * (1 + az1)
    dmd0, dmd1 = big_g @ md1, big_g.transpose(1, 2) @ md0
    admd0, admd1 = abig_g @ amd1, abig_g.transpose(1, 2) @ amd0
    s_out = 1.0 if variant == "s_once" else s
    flat = lambda t: t.reshape(-1, t.shape[-1])
    dwf = s_out * (flat(dmd0).t() @ flat(x0) + flat(dmd1).t() @ flat(x1))
    if variant == "dwf_transposed":
        dwf = dwf.t().contiguous()
    grads = {"dWf": dwf, "dbf": s_out * (flat(dmd0).sum(0) + flat(dmd1).sum(0)),
             "dwm": dz0.reshape(-1) @ flat(x0) + dz1.reshape(-1) @ flat(x1), "dbm": dz0.sum() + dz1.sum(),
             "dx0": s_out * (dmd0 @ wf) + dz0[:, :, None] * wm, "dx1": s_out * (dmd1 @ wf) + dz1[:, :, None] * wm}
    sums = {"dWf": s * (flat(admd0).t() @ flat(ax0) + flat(admd1).t() @ flat(ax1)),
            "dbf": s * (flat(admd0).sum(0) + flat(admd1).sum(0)),
            "dwm": adz0.reshape(-1) @ flat(ax0) + adz1.reshape(-1) @ flat(ax1), "dbm": adz0.sum() + adz1.sum(),
            "dx0": s * (admd0 @ awf) + adz0[:, :, None] * wm.abs(), "dx1": s * (admd1 @ awf) + adz1[:, :, None] * wm.abs()}
    return grads, sums


def token_grad(x0, x1, tw, tb, correct0, correct1, g, nl, variant=None, logit0=None, logit1=None):
    """x0 [B,M,256], x1 [B,N,256], tw [256], tb scalar tensor, correct0 [B,M], correct1 [B,N], g [B] = grad_total.
    logit0/1: the logits the gradient is evaluated at (default: x . tw + tb).  -> (grads, abs_sums), each {dw, db}."""
    b, m, _ = x0.shape
    n = x1.shape[1]
    l0 = x0 @ tw + tb if logit0 is None else logit0
    l1 = x1 @ tw + tb if logit1 is None else logit1
    al0, al1 = l0.abs(), l1.abs()
    if variant == "token_mean_m_plus_n":
        inv0 = inv1 = 1.0 / ((m + n) * (nl - 1))
    else:
        inv0, inv1 = 1.0 / (2.0 * m * (nl - 1)), 1.0 / (2.0 * n * (nl - 1))
    y0, y1 = correct0.double(), correct1.double()
    d0 = g[:, None] * (torch.sigmoid(l0) - y0) * inv0
    d1 = g[:, None] * (torch.sigmoid(l1) - y1) * inv1
    a0 = g.abs()[:, None] * (torch.sigmoid(l0) * (1 + al0) + y0) * inv0
    a1 = g.abs()[:, None] * (torch.sigmoid(l1) * (1 + al1) + y1) * inv1
    flat = lambda t: t.reshape(-1, t.shape[-1])
    grads = {"dw": d0.reshape(-1) @ flat(x0) + d1.reshape(-1) @ flat(x1), "db": d0.sum() + d1.sum()}
    sums = {"dw": a0.reshape(-1) @ flat(x0.abs()) + a1.reshape(-1) @ flat(x1.abs()), "db": a0.sum() + a1.sum()}
    return grads, sums


def head_params(sd, layer):
    p = f"log_assignment.{layer}."
    return (sd[p + "final_proj.weight"].double(), sd[p + "final_proj.bias"].double(),
            sd[p + "matchability.weight"].double().reshape(-1), sd[p + "matchability.bias"].double().reshape(()))


def token_params(sd, layer):
    p = f"token_confidence.{layer}.token.0."
    return sd[p + "weight"].double().reshape(-1), sd[p + "bias"].double().reshape(())


def model_grads(xs0, xs1, sd, data, gamma=1.0, lam=0.5, grad_total=None, variant=None, descriptor_grads=False):
    """xs0 / xs1: the L layers' descriptors [B,M,256] / [B,N,256] (float64); sd: the state dict; data: gt_matches0/1
    and gt_assignment (or None).  -> (grads, abs_sums, c): dicts keyed by the reference's state-dict names (and
    `grad_ref_descriptors0/1` [B,L,M/N,256] with descriptor_grads), c[name] the constant of that output's bound."""
    nl = len(xs0)
    b, m, _ = xs0[0].shape
    n = xs1[0].shape[1]
    gt0, gt1, gta = data["gt_matches0"], data["gt_matches1"], data.get("gt_assignment")
    gtot = torch.full((b,), 1.0 / b, dtype=torch.float64) if grad_total is None else grad_total.double()
    wl = layer_weights(nl, gamma, variant)
    las = [head_forward(xs0[i], xs1[i], *head_params(sd, i)) for i in range(nl)]
    grads, sums, cs = {}, {}, {}
    hc, tc = head_c(b, m, n), token_c(b, m, n)
    dxs0, dxs1, adxs0, adxs1 = [], [], [], []
    for i in range(nl):
        g, s = head_grad(xs0[i], xs1[i], *head_params(sd, i), gt0, gt1, gta, gtot * wl[i], lam, variant)
        p = f"log_assignment.{i}."
        for key, k in (("final_proj.weight", "dWf"), ("final_proj.bias", "dbf"), ("matchability.weight", "dwm"),
                       ("matchability.bias", "dbm")):
            shape = (1, D) if k == "dwm" else (1,) if k == "dbm" else g[k].shape
            grads[p + key], sums[p + key], cs[p + key] = g[k].reshape(shape), s[k].reshape(shape), hc[k]
        dxs0.append(g["dx0"]), dxs1.append(g["dx1"]), adxs0.append(s["dx0"]), adxs1.append(s["dx1"])
        if i < nl - 1:
            c0, c1 = lr.token_targets(las[i], las[-1])
            g, s = token_grad(xs0[i], xs1[i], *token_params(sd, i), c0, c1, gtot, nl, variant)
            p = f"token_confidence.{i}.token.0."
            grads[p + "weight"], sums[p + "weight"], cs[p + "weight"] = g["dw"].reshape(1, D), s["dw"].reshape(1, D), tc
            grads[p + "bias"], sums[p + "bias"], cs[p + "bias"] = g["db"].reshape(1), s["db"].reshape(1), tc
    if descriptor_grads:
        for side, dx, adx in (("0", dxs0, adxs0), ("1", dxs1, adxs1)):
            k = "grad_ref_descriptors" + side
            grads[k], sums[k], cs[k] = torch.stack(dx, 1), torch.stack(adx, 1), hc["dx"]
    return grads, sums, cs


def total_loss(xs0, xs1, sd, data, gamma=1.0, lam=0.5):
    """`total` [B] of the training loss (lightglue.py:597-630) of the layers' descriptors under the heads and tokens of
    `sd`, in float64: the function whose gradient `model_grads` states."""
    nl = len(xs0)
    las = [head_forward(xs0[i], xs1[i], *head_params(sd, i)) for i in range(nl)]
    lo0 = [xs0[i] @ token_params(sd, i)[0] + token_params(sd, i)[1] for i in range(nl - 1)]
    lo1 = [xs1[i] @ token_params(sd, i)[0] + token_params(sd, i)[1] for i in range(nl - 1)]
    losses, _, _ = lr.layer_loss(las, lo0, lo1, data, [0.5] * (nl - 1), gamma=gamma, balancing=lam)
    return losses["total"]
