"""Ground truth from dense warps (RoMa): everything the reference does AFTER the network, on the GPU.

`cycle_dist` (gluefactory/utils/image.py:260-270), `sample_dense` and `gt_matches_from_roma` (gluefactory/geometry/
gt_generation.py:61-269) through the entries of include/gfc_amd_dense_warp.h (csrc/gt_dense_warp.hip), which states the
sampling rule and the order of decisions.  The network itself (DINOv2 ViT-L plus a decoder) is not part of this package:
the caller supplies its output, `warp0/1` [B,H,W,2] in normalised coordinates and `certainty0/1` [B,H,W], optionally
`cycle_error0/1` [B,H,W].
MI355X additions: `add_cycle_error=True` without `cycle_error0/1` computes the cycle error at the four tap pixels of
every key point only (bit-equal to building both dense fields with `cycle_dist` and sampling them; no dense field is
allocated), and `dense=False` omits `assignment` and `reward` and never allocates them.
"""
import torch

from . import _native as nat

MASK_KEYS = ("mask_pos", "mask_neg_far", "mask_neg_unreliable", "mask_ign")  # the rows of masks0 / masks1
_workspace = nat.Workspace()


def _field(t, name, last=None):
    nat.require_cuda(t, name)
    t = t.float().contiguous()
    want = 4 if last else 3
    if t.ndim != want or (last and t.shape[-1] != last):
        raise ValueError(f"{name} must be [B,H,W{',2' if last else ''}], got {tuple(t.shape)}")
    return t


def cycle_dist(q_to_ref, ref_to_q):
    """cycle_dist(q_to_ref, ref_to_q, normalized=False) of the reference for channel-last fields [B,H,W,2] and
    [B,Hr,Wr,2] of normalised coordinates: the cycle-consistency error [B,H,W] in pixels of the field q_to_ref."""
    q, r = _field(q_to_ref, "q_to_ref", 2), _field(ref_to_q, "ref_to_q", 2)
    if q.shape[0] != r.shape[0]:
        raise ValueError("cycle_dist: the two fields differ in batch size")
    out = torch.empty(q.shape[:3], dtype=torch.float32, device=q.device)
    nat.call("gfc_dense_cycle_error", q, r, out, q.shape[0], q.shape[1], q.shape[2], r.shape[1], r.shape[2],
             device=q.device)
    return out


def sample_dense_warp(kpts, warp, certainty, q_hw, output_hw, cycle_error=None, other_warp=None):
    """sample_dense of the reference for one direction: key points [B,M,2] in pixels of the image of size q_hw, the
    warp towards the image of size output_hw.  Returns (proj [B,M,2], certainty_kp [B,M], cycle_kp [B,M]); cycle_kp is
    sampled from `cycle_error` when given, else computed at the taps from `other_warp` when given, else 0."""
    nat.require_cuda(kpts, "keypoints")
    k = kpts.float().contiguous()
    w, c = _field(warp, "warp", 2), _field(certainty, "certainty")
    b, m = k.shape[:2]
    if w.shape[0] != b or c.shape != w.shape[:3]:
        raise ValueError(f"sample_dense_warp: warp {tuple(w.shape)} / certainty {tuple(c.shape)} / keypoints {tuple(k.shape)}")
    e = o = None
    hr = wr = 0
    if cycle_error is not None:
        e = _field(cycle_error, "cycle_error")
        if e.shape != c.shape:
            raise ValueError("sample_dense_warp: cycle_error and certainty differ in shape")
    elif other_warp is not None:
        o = _field(other_warp, "other_warp", 2)
        hr, wr = o.shape[1], o.shape[2]
    proj = torch.empty((b, m, 2), dtype=torch.float32, device=k.device)
    cert_kp = torch.empty((b, m), dtype=torch.float32, device=k.device)
    cyc_kp = torch.empty((b, m), dtype=torch.float32, device=k.device)
    nat.call("gfc_gt_sample_dense_warp", k, w, c, e, o, b, m, w.shape[1], w.shape[2], hr, wr, int(q_hw[0]), int(q_hw[1]),
             int(output_hw[0]), int(output_hw[1]), proj, cert_kp, cyc_kp, device=k.device)
    return proj, cert_kp, cyc_kp


def roma_labels(kp0, kp1, proj_0to1, proj_1to0, certainty_kp0, certainty_kp1, cycle_kp0, cycle_kp1, valid0, valid1,
                pos_th, neg_th, pos_cert_th=None, pos_cycle_error_th=None, neg_cert_th=None, neg_cycle_error_th=None,
                dense=True):
    """The label part of gt_matches_from_roma (one call of gfc_gt_matches_roma): matches, scores, the eight masks and,
    with `dense`, assignment and reward."""
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    for name, v in (("pos_th", pos_th), ("neg_th", neg_th), ("pos_cert_th", pos_cert_th),
                    ("pos_cycle_error_th", pos_cycle_error_th), ("neg_cert_th", neg_cert_th),
                    ("neg_cycle_error_th", neg_cycle_error_th)):
        if v is not None and v < 0:
            raise ValueError(f"gt_matches_from_roma: {name} must not be negative")
    m0 = torch.empty((b, m), dtype=torch.long, device=dev)
    m1 = torch.empty((b, n), dtype=torch.long, device=dev)
    sc0 = torch.empty((b, m), dtype=torch.float32, device=dev)
    sc1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    masks0 = torch.empty((b, 4, m), dtype=torch.bool, device=dev)
    masks1 = torch.empty((b, 4, n), dtype=torch.bool, device=dev)
    assignment = reward = None
    if dense:
        assignment = torch.empty((b, m, n), dtype=torch.bool, device=dev)
        reward = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    nbytes = nat.call("gfc_gt_matches_roma_workspace_bytes", b, m, n)
    ws = _workspace.get(max(nbytes, 1), dev)
    none = lambda v: -1.0 if v is None else float(v)  # noqa: E731
    mask = lambda v, k: v.to(device=dev).reshape(b, k).ne(0).contiguous()  # noqa: E731
    nat.call("gfc_gt_matches_roma", kp0, kp1, proj_0to1, proj_1to0, certainty_kp0, certainty_kp1, cycle_kp0, cycle_kp1,
             mask(valid0, m), mask(valid1, n), b, m, n, float(pos_th), float(neg_th), none(pos_cert_th),
             none(pos_cycle_error_th), none(neg_cert_th), none(neg_cycle_error_th), m0, m1, sc0, sc1, masks0, masks1,
             assignment, reward, ws, nbytes, device=dev)
    out = {}
    if dense:
        out["assignment"], out["reward"] = assignment, reward
    out.update({"matches0": m0, "matches1": m1, "matching_scores0": sc0, "matching_scores1": sc1})
    for r, key in enumerate(MASK_KEYS):
        out[key + "0"], out[key + "1"] = masks0[:, r], masks1[:, r]
    return out


def gt_matches_from_roma(kp0, kp1, data=None, **kw):
    """Drop-in for the reference's function: its keyword names, its four ValueErrors and its twenty keys.  Additional
    keywords: `add_cycle_error` (cycle error at the taps when cycle_error0/1 are not given) and `dense`."""
    dense = bool(kw.get("dense", True))
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    b, m, n = k0.shape[0], k0.shape[1], k1.shape[1]
    valid0, valid1 = kw.get("valid0"), kw.get("valid1")
    if m == 0 or n == 0:  # gt_generation.py:62-94
        nat.require_cuda(kp0, "keypoints0")
        nat.require_cuda(kp1, "keypoints1")
        dev = k0.device
        z0 = torch.zeros((b, m), dtype=torch.bool, device=dev)
        z1 = torch.zeros((b, n), dtype=torch.bool, device=dev)
        out = roma_labels(k0, k1, None, None, None, None, None, None, z0, z1, 0.0, 0.0, dense=dense)  # reads none of them
        out.update({"proj_0to1": torch.empty_like(k0), "proj_1to0": torch.empty_like(k1),
                    "certainty_kp0": k0[:, :, 0], "certainty_kp1": k1[:, :, 0],
                    "cycle_error_kp0": k0[:, :, 0], "cycle_error_kp1": k1[:, :, 0]})
        if dense:
            out["assignment"].zero_()
            out["reward"].zero_()
        return out
    if valid0 is None or valid1 is None:
        raise ValueError("gt_matches_from_roma requires valid0 and valid1.")
    warp0, warp1 = kw.get("warp0"), kw.get("warp1")
    certainty0, certainty1 = kw.get("certainty0"), kw.get("certainty1")
    cycle_error0, cycle_error1 = kw.get("cycle_error0"), kw.get("cycle_error1")
    pos_th, neg_th = kw.get("pos_th"), kw.get("neg_th")
    pos_cycle_error_th, neg_cycle_error_th = kw.get("pos_cycle_error_th"), kw.get("neg_cycle_error_th")
    at_taps = bool(kw.get("add_cycle_error", False)) and (cycle_error0 is None or cycle_error1 is None)
    if warp0 is None or warp1 is None or certainty0 is None or certainty1 is None:
        raise ValueError("gt_matches_from_roma requires warp0/1 and certainty0/1 dense tensors.")
    if pos_th is None or neg_th is None:
        raise ValueError("gt_matches_from_roma requires pos_th and neg_th.")
    if (pos_cycle_error_th is not None or neg_cycle_error_th is not None) and not at_taps \
            and (cycle_error0 is None or cycle_error1 is None):
        raise ValueError("gt_matches_from_roma requires cycle_error0/1 when cycle thresholds are set.")
    nat.require_cuda(kp0, "keypoints0")
    nat.require_cuda(kp1, "keypoints1")
    if at_taps or cycle_error0 is None or cycle_error1 is None:  # the reference samples them only when BOTH are given
        cycle_error0 = cycle_error1 = None
    img0_hw = data["view0"]["image"].shape[-2:]
    img1_hw = data["view1"]["image"].shape[-2:]
    p01, c0, e0 = sample_dense_warp(k0, warp0, certainty0, img0_hw, img1_hw, cycle_error0, warp1 if at_taps else None)
    p10, c1, e1 = sample_dense_warp(k1, warp1, certainty1, img1_hw, img0_hw, cycle_error1, warp0 if at_taps else None)
    out = roma_labels(k0, k1, p01, p10, c0, c1, e0, e1, valid0, valid1, pos_th, neg_th, kw.get("pos_cert_th"),
                      pos_cycle_error_th, kw.get("neg_cert_th"), neg_cycle_error_th, dense=dense)
    out.update({"proj_0to1": p01, "proj_1to0": p10, "certainty_kp0": c0, "certainty_kp1": c1, "cycle_error_kp0": e0,
                "cycle_error_kp1": e1})
    return out
