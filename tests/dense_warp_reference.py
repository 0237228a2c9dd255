"""Restatement of the dense-warp ground truth (cycle_dist, gluefactory/utils/image.py:260-270; sample_dense and
gt_matches_from_roma, gluefactory/geometry/gt_generation.py:127-134, 149-269) with torch operations in float64: the
checker of csrc/gt_dense_warp.hip, plus the inputs of its tests.  Everything is for ONE pair (no batch axis).

  grid_sample   F.grid_sample(bilinear, zeros, align_corners=False) on a channel-last field, with a PER-ELEMENT bound
  cycle_dist    stage 1, with its bound
  sample_dense  stage 2: proj, certainty_kp, cycle_kp (from a field, or from the other warp at the taps), with bounds
  roma_labels   stage 3: the twenty keys' label part and which verdicts are UNDECIDED
  run           the three stages on a case; make_case / tie_case the inputs

The bound of a sample (u = 2^-24, a float32 evaluation of the same float32 inputs against this one):
  * the position.  c = x / (w - 1) * 2 - 1: the division rounds once (relative u of a value <= 2 after the doubling), the
    subtraction once (u |c|): |dc| <= 3 u max(1, |c|).  ix = ((c + 1) W - 1) / 2: the sum rounds once (u |c + 1|), the
    product once (u |c + 1| W), the difference once (u |c + 1| W, as the product is the larger operand), the halving is
    exact: |d ix| <= ((3 + 2) u W + 2 u |c + 1| W) / 2 <= 4.5 u W max(1, |c|) for |c + 1| <= 2.  DELTA_OPS = 5 is used:
    delta_x = 5 u W max(1, |c_x|), delta_y alike with H.  For cycle_dist c is an input (no normalisation): the same
    formula over-covers.
  * the interpolant is continuous in the position, across cell borders and across the border of the field (zero padding
    is a tap like any other), with slope per axis at most the spread (max - min) of the taps around it.  So a shift of
    the position moves the sample by at most (delta_x + delta_y) * spread, where the spread is taken over the taps of
    the three positions p - delta, p, p + delta (a float32 floor may land in the neighbouring cell).  A key point within
    half a field pixel of the border has padding zeros among its taps: its spread is the full value.
  * the arithmetic at a fixed position.  A weight is two differences (relative u each) and a product (u): 3 u; a term
    v * w adds u: 4 u |v| w, and the weights sum to 1: 4 u max|tap|; three additions of partial sums <= max|tap|: 3 u
    max|tap|.  7 in all; C_OPS = 8 is used.
  bound(sample) = (delta_x + delta_y) spread + 8 u max|tap| + sum_taps w * bound(tap)   (the last term for taps that are
  themselves computed: the cycle error of a tap pixel).
  De-normalisation (s + 1) / 2 * (t - 1) = scale (s + 1), scale = (t - 1) / 2: the sum rounds once (u (|s| + 1)), the
  product once (u |result|):  bound(proj) = scale (bound(s) + u (|s| + 1)) + u |proj|.
  cycle error e = |g - b|, b the de-normalised sample: |de| <= |db_x| + |db_y| + 4 u (e + |g|) (two differences, two
  squares, a sum and a root; the differences round relative to operands as large as |g|).
A sample is NaN-UNDECIDED when a tap of the shifted positions is not finite while this evaluation is finite.

A verdict is undecided when a compared quantity (distance, certainty, cycle error) lies within the element's own bound of
its threshold, or a distance within the bounds of the runner-up of an arg-min; key points whose valid_pos is undecided
are counted in AND out, and whatever changes with them is undecided.  The bound of a distance of the pair (i, j) is
sqrt(2) max(bound(proj0[i]), bound(proj1[j])) + 4 u (d + max|coordinate|).

`rule=` selects a deliberately WRONG variant (WRONG_SAMPLING, WRONG_LABELS); the host test shows the fixture rejects each.
"""
import math

import torch

U = 2.0 ** -24
DELTA_OPS, C_OPS = 5.0, 8.0
INF = float("inf")
WRONG_SAMPLING = ("align_corners", "w_not_w_minus_1", "image_size_for_field", "half_pixel_repaired")
WRONG_LABELS = ("neg_far_unmasked", "neg_far_symmetric", "negative_overrides_positive", "mask_pos_is_positive",
                "scores_01")
MASK_KEYS = ("mask_pos", "mask_neg_far", "mask_neg_unreliable", "mask_ign")
# (pos_th, neg_th, pos_cert_th, pos_cycle_error_th, neg_cert_th, neg_cycle_error_th, cycle fields given)
SETTINGS = ((3.0, 5.0, 0.05, 2.0, 5e-4, 20.0, True), (3.0, 5.0, None, None, None, None, False),
            (3.0, 5.0, 0.05, 2.0, 5e-4, None, True), (6.0, 5.0, 0.05, 2.0, 5e-4, 20.0, True))
FIELD0, FIELD1, IMG0, IMG1 = (48, 64), (40, 56), (120, 160), (96, 128)  # (h, w) each
# The fixture's cases (m, n, field of warp1)
CASES = ((257, 130, FIELD1), (65, 1, FIELD1), (1, 65, FIELD1))


# ---- stage 0: grid_sample ------------------------------------------------------------------------------------------------
def _taps(field, ix, iy):
    """values [P,4,C] (zeros outside), weights [P,4], inside [P,4] of the four taps around (ix, iy)."""
    H, W = field.shape[:2]
    x0, y0 = ix.floor(), iy.floor()
    xs = torch.stack([x0, x0 + 1, x0, x0 + 1], -1)
    ys = torch.stack([y0, y0, y0 + 1, y0 + 1], -1)
    wx = torch.stack([x0 + 1 - ix, ix - x0, x0 + 1 - ix, ix - x0], -1)
    wy = torch.stack([y0 + 1 - iy, y0 + 1 - iy, iy - y0, iy - y0], -1)
    inside = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
    xi, yi = xs.clamp(0, W - 1).nan_to_num().long(), ys.clamp(0, H - 1).nan_to_num().long()
    vals = torch.where(inside[..., None], field[yi, xi], torch.zeros((), dtype=field.dtype))
    return vals, wx * wy, inside


def grid_sample(field, c, tap_bound=None, rule=None, image_hw=None):
    """field [H,W,C] float64, c [P,2] normalised positions -> (sample [P,C], bound [P,C], nan_undecided [P]).
    tap_bound [H,W,C]: the bound of the field's own values (None: the field is an input)."""
    H, W = field.shape[:2]
    if rule == "image_size_for_field":
        sh, sw = image_hw
    else:
        sh, sw = H, W
    if rule == "align_corners":
        ix, iy = (c[:, 0] + 1) / 2 * (sw - 1), (c[:, 1] + 1) / 2 * (sh - 1)
    else:
        ix, iy = ((c[:, 0] + 1) * sw - 1) / 2, ((c[:, 1] + 1) * sh - 1) / 2
    vals, w, inside = _taps(field, ix, iy)
    finite_pos = torch.isfinite(ix) & torch.isfinite(iy)
    # every inside tap is multiplied through (0 * NaN = NaN); a tap outside adds nothing
    terms = torch.where(inside[..., None], vals * w[..., None], torch.zeros((), dtype=field.dtype))
    out = terms[:, 0] + terms[:, 1] + terms[:, 2] + terms[:, 3]
    out = torch.where(finite_pos[:, None], out, torch.full_like(out, float("nan")))
    dx = DELTA_OPS * U * W * c[:, 0].abs().clamp(min=1).nan_to_num(posinf=0)
    dy = DELTA_OPS * U * H * c[:, 1].abs().clamp(min=1).nan_to_num(posinf=0)
    around = [vals] + [_taps(field, ix + s * dx, iy + s * dy)[0] for s in (-1.0, 1.0)]
    allv = torch.cat(around, 1)  # [P,12,C]
    shaky = ~torch.isfinite(allv).all(1).all(-1) & torch.isfinite(out).all(-1)
    fin = allv.nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
    spread = fin.max(1).values - fin.min(1).values
    bound = (dx + dy)[:, None] * spread + C_OPS * U * fin.abs().max(1).values
    if tap_bound is not None:
        tb = _taps(tap_bound, ix, iy)[0].nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
        bound = bound + (tb * w[..., None].abs()).sum(1) + (dx + dy)[:, None] * tb.max(1).values
    return out, bound, shaky


def normalize(kp, hw, rule=None):
    h, w = hw
    if rule == "w_not_w_minus_1":
        return torch.stack([kp[:, 0] / w * 2 - 1, kp[:, 1] / h * 2 - 1], -1)
    return torch.stack([kp[:, 0] / (w - 1) * 2 - 1, kp[:, 1] / (h - 1) * 2 - 1], -1)


def denormalize(s, bound, hw):
    """denormalize_coords with its bound: (value [P,2], bound [P,2])."""
    scale = torch.tensor([(hw[1] - 1) / 2, (hw[0] - 1) / 2], dtype=s.dtype)
    v = (s + 1) / 2 * torch.tensor([hw[1] - 1, hw[0] - 1], dtype=s.dtype)
    return v, scale * (bound + U * (s.abs() + 1)) + U * v.abs()


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------
def cycle_dist(q, r, rule=None):
    """q [H,W,2], r [Hr,Wr,2] float64 -> (error [H,W], bound [H,W], nan_undecided [H,W])."""
    H, W = q.shape[:2]
    s, sb, shaky = grid_sample(r, q.reshape(-1, 2))
    b, bb = denormalize(s, sb, (H, W))  # hw=None: the size of the sampled tensor, which has the shape of q
    ys, xs = torch.meshgrid(torch.arange(H, dtype=q.dtype), torch.arange(W, dtype=q.dtype), indexing="ij")
    g = torch.stack([xs, ys], -1).reshape(-1, 2) + (0.0 if rule == "half_pixel_repaired" else 0.5)
    e = (g - b).norm(dim=-1)
    bound = bb.sum(-1) + 4 * U * (e + g.abs().max(-1).values)
    return e.reshape(H, W), bound.nan_to_num(nan=0.0, posinf=0.0).reshape(H, W), shaky.reshape(H, W)


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------
def sample_dense(kp, warp, cert, q_hw, out_hw, cyc=None, other=None, rule=None):
    """One direction.  cyc [H,W]: the cycle field as an INPUT; other [Hr,Wr,2]: cycle error at the taps (the field is
    computed here, with its bound); both None: zeros.  Returns a dict of values, bounds and the NaN-undecided flags."""
    c = normalize(kp, q_hw, rule)
    kw = {"rule": rule, "image_hw": q_hw}
    s, sb, shaky = grid_sample(warp, c, **kw)
    proj, pb = denormalize(s, sb, out_hw)
    ce, cb, shaky_c = grid_sample(cert[..., None], c, **kw)
    out = {"proj": proj, "proj_bound": pb.max(-1).values, "cert": ce[:, 0], "cert_bound": cb[:, 0],
           "shaky": shaky | shaky_c}
    if cyc is None and other is None:
        out["cyc"], out["cyc_bound"] = torch.zeros_like(ce[:, 0]), torch.zeros_like(ce[:, 0])
        return out
    tb = None
    if cyc is None:
        cyc, tb, tap_shaky = cycle_dist(warp, other, rule)
        tb = tb[..., None]
        # a tap pixel whose own cycle error may be NaN in float32 only
        ts = grid_sample(tap_shaky[..., None].to(warp.dtype), c)[0][:, 0]
        out["shaky"] = out["shaky"] | (ts.nan_to_num(nan=1.0) > 0)
    e, eb, shaky_e = grid_sample(cyc[..., None], c, tap_bound=tb, **kw)
    out["cyc"], out["cyc_bound"], out["shaky"] = e[:, 0], eb[:, 0], out["shaky"] | shaky_e
    return out


# ---- stage 3 ---------------------------------------------------------------------------------------------------------------
def _valid_pos(valid, proj, cert, cyc, pc, pcy):
    v = valid & torch.isfinite(proj).all(-1) & torch.isfinite(cert)
    if pc is not None:
        v = v & (cert > pc)
    if pcy is not None:
        v = v & torch.isfinite(cyc) & (cyc < pcy)
    return v


def _core(kp0, kp1, p01, p10, c0, c1, e0, e1, valid0, valid1, vp0, vp1, th, rule):
    pos_th, neg_th, pc, pcy, nc, ncy = th
    M, N = kp0.shape[0], kp1.shape[0]
    D0 = ((p01[:, None] - kp1[None]) ** 2).sum(-1)
    D1 = ((kp0[:, None] - p10[None]) ** 2).sum(-1)
    pair = vp0[:, None] & vp1[None]
    inf = torch.full_like(D0, INF)
    D = torch.where(pair, torch.maximum(D0, D1), inf)
    min0, min1 = D.min(1).indices, D.min(0).indices
    ismin0, ismin1 = torch.zeros_like(pair), torch.zeros_like(pair)
    ismin0[torch.arange(M), min0] = True
    ismin1[min1, torch.arange(N)] = True
    positive = ismin0 & ismin1 & (D < pos_th ** 2)
    pos0, pos1 = positive.any(1), positive.any(0)
    if rule == "neg_far_unmasked":
        own0, own1 = D0.nan_to_num(nan=INF).min(1).values, D1.nan_to_num(nan=INF).min(0).values
    elif rule == "neg_far_symmetric":
        own0, own1 = D.min(1).values, D.min(0).values
    else:
        own0 = torch.where(vp1[None], D0, inf).min(1).values
        own1 = torch.where(vp0[:, None], D1, inf).min(0).values
    far0, far1 = vp0 & (own0 > neg_th ** 2), vp1 & (own1 > neg_th ** 2)
    un0, un1 = torch.zeros_like(valid0), torch.zeros_like(valid1)
    if nc is not None and ncy is not None:
        un0 = valid0 & torch.isfinite(c0) & torch.isfinite(e0) & (c0 < nc) & (e0 > ncy)
        un1 = valid1 & torch.isfinite(c1) & torch.isfinite(e1) & (c1 < nc) & (e1 > ncy)
    if rule == "negative_overrides_positive":
        neg0, neg1 = far0 | un0, far1 | un1
    else:
        neg0, neg1 = (far0 | un0) & ~pos0, (far1 | un1) & ~pos1
    m0 = torch.where(pos0, min0, torch.full_like(min0, -2))
    m1 = torch.where(pos1, min1, torch.full_like(min1, -2))
    m0, m1 = torch.where(neg0, -torch.ones_like(m0), m0), torch.where(neg1, -torch.ones_like(m1), m1)
    one = (lambda p, c: p.to(c.dtype)) if rule == "scores_01" else (lambda p, c: torch.where(p, c, torch.zeros_like(c)))
    reward = torch.maximum((pair & (D < pos_th ** 2)).to(D.dtype), positive.to(D.dtype)) \
        - (pair & (D > neg_th ** 2)).to(D.dtype)
    mp0, mp1 = (pos0, pos1) if rule == "mask_pos_is_positive" else (vp0, vp1)
    return {"matches0": m0, "matches1": m1, "matching_scores0": one(pos0, c0), "matching_scores1": one(pos1, c1),
            "mask_pos0": mp0, "mask_pos1": mp1, "mask_neg_far0": far0, "mask_neg_far1": far1,
            "mask_neg_unreliable0": un0, "mask_neg_unreliable1": un1, "mask_ign0": valid0 & ~pos0 & ~neg0,
            "mask_ign1": valid1 & ~pos1 & ~neg1, "assignment": positive, "reward": reward,
            "_D": D, "_own0": own0, "_own1": own1, "_min0": min0, "_min1": min1}


KP_KEYS = ("matches", "mask_pos", "mask_neg_far", "mask_neg_unreliable", "mask_ign")


def roma_labels(kp0, kp1, s0, s1, valid0, valid1, th, rule=None):
    """s0, s1: the dicts of sample_dense.  th = (pos_th, neg_th, pos_cert_th, pos_cycle_error_th, neg_cert_th,
    neg_cycle_error_th).  Returns the label keys plus undecided0 [M], undecided1 [N], undecided_dense [M,N]."""
    pos_th, neg_th, pc, pcy, nc, ncy = th
    valid0, valid1 = valid0.bool(), valid1.bool()
    args = lambda s: (s["proj"], s["cert"], s["cyc"])  # noqa: E731
    vp0, vp1 = _valid_pos(valid0, *args(s0), pc, pcy), _valid_pos(valid1, *args(s1), pc, pcy)

    def near(v, b, t):
        return torch.zeros_like(b, dtype=torch.bool) if t is None else ((v - t).abs() <= b) & torch.isfinite(v)

    def shaky_vp(s, valid):
        return valid & (s["shaky"] | near(s["cert"], s["cert_bound"], pc) | near(s["cyc"], s["cyc_bound"], pcy))

    sv0, sv1 = shaky_vp(s0, valid0), shaky_vp(s1, valid1)
    run = lambda a, b: _core(kp0, kp1, s0["proj"], s1["proj"], s0["cert"], s1["cert"], s0["cyc"], s1["cyc"], valid0,  # noqa: E731
                             valid1, a, b, th, rule)
    r = run(vp0, vp1)
    und0, und1 = sv0.clone(), sv1.clone()
    und_dense = torch.zeros_like(r["assignment"])
    if bool(sv0.any()) or bool(sv1.any()):
        for a, b in ((vp0 | sv0, vp1 | sv1), (vp0 & ~sv0, vp1 & ~sv1)):
            alt = run(a, b)
            for k in KP_KEYS:
                und0 |= alt[k + "0"] != r[k + "0"]
                und1 |= alt[k + "1"] != r[k + "1"]
            und_dense |= (alt["assignment"] != r["assignment"]) | (alt["reward"] != r["reward"])
    if nc is not None and ncy is not None:
        und0 |= valid0 & (near(s0["cert"], s0["cert_bound"], nc) | near(s0["cyc"], s0["cyc_bound"], ncy) | s0["shaky"])
        und1 |= valid1 & (near(s1["cert"], s1["cert_bound"], nc) | near(s1["cyc"], s1["cyc_bound"], ncy) | s1["shaky"])
    # distances
    D = r["_D"]
    d = D.sqrt()
    cm = max(float(kp0.abs().max()), float(kp1.abs().max()), 1.0)
    pb0 = s0["proj_bound"].nan_to_num(nan=0.0, posinf=0.0)
    pb1 = s1["proj_bound"].nan_to_num(nan=0.0, posinf=0.0)
    bd = math.sqrt(2.0) * torch.maximum(pb0[:, None], pb1[None]) + 4 * U * (d.nan_to_num(posinf=0.0) + cm)
    M, N = D.shape
    rows, cols = torch.arange(M), torch.arange(N)

    def second(dim, arg):
        """runner-up of the arg-min along dim, with the margin bound(best) + bound(second)"""
        masked = d.clone()
        if dim == 1:
            masked[rows, arg] = INF
            best, bbest = d[rows, arg], bd[rows, arg]
        else:
            masked[arg, cols] = INF
            best, bbest = d[arg, cols], bd[arg, cols]
        gap = (masked - best.unsqueeze(dim) - bd - bbest.unsqueeze(dim)).min(dim).values
        return (gap <= 0) & torch.isfinite(best) & (best <= pos_th + bbest)

    rn, cn = second(1, r["_min0"]), second(0, r["_min1"])
    best0, best1 = d[rows, r["_min0"]], d[r["_min1"], cols]
    at0 = ((best0 - pos_th).abs() <= bd[rows, r["_min0"]]) & torch.isfinite(best0)
    at1 = ((best1 - pos_th).abs() <= bd[r["_min1"], cols]) & torch.isfinite(best1)
    o0, o1 = r["_own0"].sqrt(), r["_own1"].sqrt()
    ob0 = math.sqrt(2.0) * pb0 + 4 * U * (o0.nan_to_num(posinf=0.0) + cm)
    ob1 = math.sqrt(2.0) * pb1 + 4 * U * (o1.nan_to_num(posinf=0.0) + cm)
    und0 |= at0 | rn | cn[r["_min0"]] | at1[r["_min0"]] | (((o0 - neg_th).abs() <= ob0) & torch.isfinite(o0))
    und1 |= at1 | cn | rn[r["_min1"]] | at0[r["_min1"]] | (((o1 - neg_th).abs() <= ob1) & torch.isfinite(o1))
    fin = torch.isfinite(d)
    und_dense |= fin & (((d - pos_th).abs() <= bd) | ((d - neg_th).abs() <= bd))
    und_dense |= (rn[:, None] | cn[None] | at0[:, None] | at1[None]) & fin & (d <= pos_th + bd)
    und_dense |= sv0[:, None] | sv1[None]
    out = {k: v for k, v in r.items() if not k.startswith("_")}
    out.update({"undecided0": und0, "undecided1": und1, "undecided_dense": und_dense})
    return out


def run(case, setting, i=0, rule=None, at_taps=False, dtype=torch.float64):
    """All three stages on pair i of a case.  With the setting's cycle flag the cycle fields are cycle_dist of the two
    warps (sampled from the field, or at the taps -- the same numbers here); without it the cycle error is 0."""
    *th, with_cycle = setting
    f = lambda k: case[k][i].to(dtype)  # noqa: E731
    srule = rule if rule in WRONG_SAMPLING else None
    o0 = o1 = None
    if with_cycle:
        o0, o1 = f("warp1"), f("warp0")
    s0 = sample_dense(f("kp0"), f("warp0"), f("certainty0"), case["img0_hw"], case["img1_hw"], other=o0, rule=srule)
    s1 = sample_dense(f("kp1"), f("warp1"), f("certainty1"), case["img1_hw"], case["img0_hw"], other=o1, rule=srule)
    out = roma_labels(f("kp0"), f("kp1"), s0, s1, case["scores0"][i] > 0, case["scores1"][i] > 0, tuple(th),
                      rule if rule in WRONG_LABELS else None)
    for q, s in (("0", s0), ("1", s1)):
        out["proj_" + ("0to1" if q == "0" else "1to0")] = s["proj"]
        out["certainty_kp" + q], out["cycle_error_kp" + q] = s["cert"], s["cyc"]
        out["proj_bound" + q], out["cert_bound" + q], out["cyc_bound" + q] = s["proj_bound"], s["cert_bound"], s["cyc_bound"]
        out["shaky" + q] = s["shaky"]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _forward(p, k):
    """A smooth map of [-1, 1]^2 into itself (float64), p [...,2]."""
    x, y = p[..., 0], p[..., 1]
    u = 0.86 * x + 0.07 * y + 0.03 + 0.03 * torch.sin(2.0 * y + k)
    v = -0.06 * x + 0.88 * y - 0.02 + 0.03 * torch.sin(2.5 * x - k)
    return torch.stack([u, v], -1)


def _inverse(q, k):
    p = q.clone()
    for _ in range(40):  # a contraction: the map is within 0.2 of the identity
        p = p + (q - _forward(p, k))
    return p


def _centres(hw):
    h, w = hw
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    return torch.stack([(xs + 0.5) / w * 2 - 1, (ys + 0.5) / h * 2 - 1], -1)


def make_case(seed, b, m, n, field0=FIELD0, field1=FIELD1, img0=IMG0, img1=IMG1, plant=True):
    """b pairs of m x n key points with their scores, two warps (a smooth map and its near-inverse plus a ripple) and two
    certainties, float32 CPU tensors.  plant: a block of each warp that disagrees with the other by far more than 20 px
    where the certainty is 1e-4, a few NaN / inf pixels, key points on the image borders and padded key points."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)  # noqa: E731
    out = {k: [] for k in ("kp0", "kp1", "scores0", "scores1", "warp0", "warp1", "certainty0", "certainty1")}
    for i in range(b):
        k = 0.3 * i + 0.1 * (seed % 7)
        c0, c1 = _centres(field0), _centres(field1)
        w0 = _forward(c0, k) + 0.004 * torch.sin(9.0 * c0.flip(-1) + k)
        w1 = _inverse(c1, k) + 0.004 * torch.cos(8.0 * c1 + k)
        ce0 = 0.55 + 0.4 * torch.sin(3.0 * c0[..., 0] + k) * torch.cos(2.0 * c0[..., 1])
        ce1 = 0.55 + 0.4 * torch.cos(2.5 * c1[..., 0]) * torch.sin(3.5 * c1[..., 1] - k)
        h0, w0s, h1, w1s = field0[0], field0[1], field1[0], field1[1]
        blk0 = (slice(h0 // 8, h0 // 8 + h0 // 5), slice(3 * w0s // 4, 3 * w0s // 4 + w0s // 5))
        blk1 = (slice(h1 // 2, h1 // 2 + h1 // 4), slice(w1s // 8, w1s // 8 + w1s // 4))
        if plant:
            w0[blk0][..., 0] -= 1.2
            ce0[blk0] = 1e-4
            w1[blk1][..., 0] += 1.2
            ce1[blk1] = 1e-4
            if h0 > 12 and w0s > 12 and h1 > 12 and w1s > 12:
                w0[h0 - 4, 5] = float("nan")
                w0[h0 - 6, w0s - 3, 1] = float("inf")
                w1[7, w1s - 5, 0] = float("-inf")
                ce0[h0 - 9, 11] = float("nan")
                ce1[2, 3] = float("inf")
        size0 = torch.tensor([img0[1] - 1, img0[0] - 1], dtype=torch.float64)
        size1 = torch.tensor([img1[1] - 1, img1[0] - 1], dtype=torch.float64)
        kp0, kp1 = rnd(m, 2) * size0, rnd(n, 2) * size1
        true = min(m, n) // 2 if min(m, n) > 1 else min(m, n)
        to1 = (_forward(kp0[:true] / size0 * 2 - 1, k) + 1) / 2 * size1
        noise = 1.5 * torch.randn((true, 2), generator=g, dtype=torch.float64)
        perm = torch.randperm(n, generator=g)[:true]
        kp1[perm] = torch.minimum(torch.maximum(to1 + noise, torch.zeros(2, dtype=torch.float64)), size1)
        s0, s1 = 0.1 + rnd(m), 0.1 + rnd(n)
        if plant and m >= 16:  # on the borders, inside the planted block, padded
            kp0[0, 0], kp0[1, 1], kp0[2, 0], kp0[3, 1] = 0.0, 0.0, size0[0], size0[1]
            kp0[4:8] = torch.stack([(blk0[1].start + 1 + rnd(4) * (w0s // 5 - 2)) / w0s,
                                    (blk0[0].start + 1 + rnd(4) * (h0 // 5 - 2)) / h0], -1) * size0
            s0[m - max(2, m // 10):] = 0.0
            kp0[m - max(2, m // 10):] = 0.0
        if plant and n >= 16:
            kp1[0, 0], kp1[1, 1], kp1[2, 0], kp1[3, 1] = 0.0, 0.0, size1[0], size1[1]
            kp1[4:8] = torch.stack([(blk1[1].start + 1 + rnd(4) * (w1s // 4 - 2)) / w1s,
                                    (blk1[0].start + 1 + rnd(4) * (h1 // 4 - 2)) / h1], -1) * size1
            s1[n - max(2, n // 10):] = 0.0
            kp1[n - max(2, n // 10):] = 0.0
        for key, v in (("kp0", kp0), ("kp1", kp1), ("scores0", s0), ("scores1", s1), ("warp0", w0), ("warp1", w1),
                       ("certainty0", ce0), ("certainty1", ce1)):
            out[key].append(v.float())
    case = {k: torch.stack(v) for k, v in out.items()}
    case.update({"img0_hw": tuple(img0), "img1_hw": tuple(img1)})
    return case


def tie_case(m, n):
    """Exact ties: images and fields of 33 x 33 (odd) with an identity warp (the normalised pixel centres, so a key
    point projects onto itself up to rounding), integer coordinates on a 10 x 10 lattice of 3-pixel steps that repeats
    every 100 key points: key points k, k + 100, k + 200, ... of a side are bit-identical, so their distances to anything
    are EQUAL floats, in other lanes (100 is no multiple of 16) and, from 300 on, in other tiles.  The first of them must
    win every arg-min: row k < 100 is matched to column k and no later twin is matched at all."""
    hw = (33, 33)
    ident = _centres(hw).float()
    lattice = lambda k: torch.stack([(torch.arange(k) % 10) * 3.0 + 3.0, ((torch.arange(k) // 10) % 10) * 3.0 + 3.0], -1)  # noqa: E731
    return {"kp0": lattice(m)[None], "kp1": lattice(n)[None], "scores0": torch.ones(1, m), "scores1": torch.ones(1, n),
            "warp0": ident[None].clone(), "warp1": ident[None].clone(), "certainty0": torch.full((1, 33, 33), 0.5),
            "certainty1": torch.full((1, 33, 33), 0.5), "img0_hw": hw, "img1_hw": hw}


def fixture_case(z, c):
    """Case c of tests/golden/dense_warp.npz in the form of make_case (the fields are stored once, with case 0)."""
    t = lambda k: torch.from_numpy(z[("c0_" if k.startswith(("warp", "certainty")) else f"c{c}_") + k])[None]  # noqa: E731
    case = {k: t(k) for k in ("kp0", "kp1", "scores0", "scores1", "warp0", "warp1", "certainty0", "certainty1")}
    hw = z[f"c{c}_hw"]
    case.update({"img0_hw": tuple(int(v) for v in hw[0]), "img1_hw": tuple(int(v) for v in hw[1])})
    return case


def large_cases():
    """The generated cases of the GPU test that no fixture holds: name -> (case, setting).  2 x 2048 x 2048 key points
    on fields of 560 x 560 (the training configuration's internal size) and 4000 x 3900, which no one-workgroup kernel
    takes."""
    return {"2x2048x2048": (make_case(11, 2, 2048, 2048, field0=(560, 560), field1=(560, 560), img0=(480, 640),
                                      img1=(448, 608)), SETTINGS[0]),
            "4000x3900": (make_case(12, 1, 4000, 3900, field0=(100, 140), field1=(90, 120), img0=(480, 640),
                                    img1=(448, 608)), SETTINGS[0])}
