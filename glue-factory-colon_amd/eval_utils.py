"""HPatches match metrics on the GPU -- counterpart of `gluefactory.eval.utils.eval_matches_homography`
(reference gluefactory/eval/utils.py:141-185).  Same arguments, same result keys; the arithmetic runs in
`gfc_eval_matches_homography` (one workgroup per pair) instead of materialising the M x N distance matrix
with torch ops.  `homography_dlt` / `eval_homography_dlt` are the weighted DLT; `homography_ransac` /
`eval_homography_robust` the robust estimator ("gfc_amd": RANSAC with MSAC scoring and a DLT local optimisation,
all thresholds of the reference's sweep in one kernel call).  The reference's own robust estimators (OpenCV /
PoseLib) are randomised CPU libraries that this package does not use: parity with them is unpinned.
"""
import ctypes

import numpy as np
import torch

from . import _native as nat

RESULT_KEYS = ("prec@1px", "prec@3px", "num_matches", "num_keypoints", "gt_match_recall@3px",
               "gt_match_precision@3px")


def match_metrics(H_0to1, kp0, kp1, matches0, pos_th=3.0, neg_th=3.0, return_gt=False):
    """Batched tensors on the device: H [B,3,3], kp0 [B,M,2], kp1 [B,N,2], matches0 [B,M] -> [B,6]
    (RESULT_KEYS order) and optionally the ground-truth matches [B,M] (-1 unmatched, -2 ignore)."""
    nat.require_cuda(kp0, "keypoints0")
    lib = nat.lib()
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    H = H_0to1.to(device=dev, dtype=torch.float32).reshape(b, 3, 3).contiguous()
    Hinv = torch.linalg.inv(H.double()).float().contiguous()  # 3x3 plumbing
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(torch.long).contiguous()
    out = torch.empty((b, 6), device=dev, dtype=torch.float32)
    gt = torch.empty((b, m), device=dev, dtype=torch.long) if return_gt else None
    nat.check(lib.gfc_eval_matches_homography(nat.ptr(k0), nat.ptr(k1), nat.ptr(m0), nat.ptr(H), nat.ptr(Hinv), b, m,
                                              n, float(pos_th), float(neg_th), nat.ptr(out), nat.ptr(gt),
                                              nat.stream_ptr(dev)), "gfc_eval_matches_homography")
    return (out, gt) if return_gt else out


def eval_matches_homography(data: dict, pred: dict) -> dict:
    """Drop-in for gluefactory.eval.utils.eval_matches_homography: un-batched inputs give floats,
    batched inputs (H_0to1.ndim > 2) lists per item (eval_per_batch_item, eval/utils.py:35-50)."""
    for key in ("H_0to1",):
        assert key in data, f"Missing key {key} in data"
    for key in ("keypoints0", "keypoints1", "matches0", "matching_scores0"):
        assert key in pred, f"Missing key {key} in data"
    H = data["H_0to1"]
    batched = H.ndim > 2
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    if not batched:
        H, kp0, kp1, m0 = H[None], kp0[None], kp1[None], m0[None]
    res = match_metrics(H, kp0, kp1, m0).cpu()
    out = {}
    for i, key in enumerate(RESULT_KEYS):
        col = res[:, i]
        vals = [int(v) if key == "num_matches" else float(v) for v in col.tolist()]
        out[key] = vals if batched else vals[0]
    return out


def homography_dlt(H_0to1, kp0, kp1, matches0, scores0, image_size0):
    """Batched device tensors -> (H_dlt [B,3,3], corner error [B]); +inf where a pair has < 4 matches."""
    nat.require_cuda(kp0, "keypoints0")
    lib = nat.lib()
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    H = H_0to1.to(device=dev, dtype=torch.float32).reshape(b, 9).contiguous()
    size = image_size0.to(device=dev, dtype=torch.float32).reshape(b, 2).contiguous()
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(torch.long).contiguous()
    sc = scores0.to(device=dev, dtype=torch.float32).contiguous()
    Hout = torch.empty((b, 3, 3), device=dev, dtype=torch.float32)
    err = torch.empty((b,), device=dev, dtype=torch.float32)
    nat.check(lib.gfc_eval_homography_dlt(nat.ptr(k0), nat.ptr(k1), nat.ptr(m0), nat.ptr(sc), nat.ptr(H), nat.ptr(size),
                                          b, m, n, nat.ptr(Hout), nat.ptr(err), nat.stream_ptr(dev)),
              "gfc_eval_homography_dlt")
    return Hout, err


def eval_homography_dlt(data: dict, pred: dict) -> dict:
    """Drop-in for gluefactory.eval.utils.eval_homography_dlt (eval/utils.py:276-302): {"H_error_dlt": float}
    (a list per item for batched input).  The weights are the matching scores, as in the reference."""
    assert "H_0to1" in data, "Missing key H_0to1 in data"
    for key in ("keypoints0", "keypoints1", "matches0", "matching_scores0"):
        assert key in pred, f"Missing key {key} in data"
    H = data["H_0to1"]
    batched = H.ndim > 2
    kp0, kp1, m0, s0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"], pred["matching_scores0"]
    size = data["view0"]["image_size"]
    if not batched:
        H, kp0, kp1, m0, s0, size = H[None], kp0[None], kp1[None], m0[None], s0[None], size[None]
    _, err = homography_dlt(H, kp0, kp1, m0, s0, size)
    vals = [float(v) for v in err.cpu().tolist()]
    return {"H_error_dlt": vals if batched else vals[0]}


# ---- robust homography (RANSAC) on the GPU ----------------------------------------------------------------
RANSAC_MAX_THRESHOLDS = 8
RANSAC_ESTIMATORS = ("gfc_amd",)
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_ransac_ws = nat.Workspace()


def _mix64(z):
    """splitmix64 finaliser on numpy uint64 (wrapping arithmetic)."""
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ransac_sample_indices(seed, stream_id, n, num_hypotheses):
    """The minimal samples of the GPU estimator, index for index (csrc/ransac.hip: rs_sample; DESIGN.md "Robust
    homography"): int64 [num_hypotheses, 4], four distinct indices in [0, n) per hypothesis.  Pure integer arithmetic:
    draw j of hypothesis h is u = mix64(key + GOLDEN * (4 h + j + 1)), key = mix64(mix64(seed + GOLDEN) ^ stream_id),
    r_j = ((u >> 32) * (n - j)) >> 32, and the r_j index a partial Fisher-Yates over the virtual array a[p] = p
    (take a[r_j], then move the last live element a[n - 1 - j] into the hole)."""
    n = int(n)
    if n < 4:
        raise ValueError("a minimal sample needs n >= 4 correspondences")
    with np.errstate(over="ignore"):
        key = _mix64(_mix64(np.uint64((int(seed) + _GOLDEN) & _M64)) ^ np.uint64(int(stream_id) & _M64))
        h = np.arange(int(num_hypotheses), dtype=np.uint64)
        r = []
        for j in range(4):
            u = _mix64(key + np.uint64(_GOLDEN) * (np.uint64(4) * h + np.uint64(j + 1)))
            r.append((((u >> np.uint64(32)) * np.uint64(n - j)) >> np.uint64(32)).astype(np.int64))
    r0, r1, r2, r3 = r
    i0 = r0
    p0, v0 = r0, n - 1
    i1 = np.where(r1 == p0, v0, r1)
    l1 = n - 2
    p1, v1 = r1, np.where(l1 == p0, v0, l1)
    i2 = np.where(r2 == p1, v1, np.where(r2 == p0, v0, r2))
    l2 = n - 3
    p2, v2 = r2, np.where(l2 == p1, v1, np.where(l2 == p0, v0, l2))
    i3 = np.where(r3 == p2, v2, np.where(r3 == p1, v1, np.where(r3 == p0, v0, r3)))
    return np.stack([i0, i1, i2, i3], axis=1).astype(np.int64)


def ransac_thresholds(ransac_th):
    """The thresholds the reference's evaluation tries (eval/hpatches.py:118-122): a positive number -> that one,
    a non-positive one -> the sweep, a sequence -> the sequence."""
    if isinstance(ransac_th, (list, tuple, np.ndarray, torch.Tensor)):
        ths = [float(t) for t in ransac_th]
    else:
        ths = [float(ransac_th)] if float(ransac_th) > 0 else [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    if not 1 <= len(ths) <= RANSAC_MAX_THRESHOLDS or not all(0 < t < float("inf") for t in ths):
        raise ValueError(f"ransac thresholds {ths}: 1 to {RANSAC_MAX_THRESHOLDS} positive finite values per call")
    return ths


def homography_ransac(H_0to1, kp0, kp1, matches0, image_size0, ransac_th, *, num_hypotheses=2048, lo_iters=3, seed=0,
                      stream_id=None):
    """RANSAC homography for B pairs x T thresholds in one call of `gfc_eval_homography_ransac`.  Batched device
    tensors: kp0 [B,M,2], kp1 [B,N,2], matches0 [B,M]; H_0to1 [B,3,3] and image_size0 [B,2] together or both None
    (no error computed); ransac_th a float or a sequence of at most 8; stream_id None (0..B-1), an int or [B] ints:
    the random stream of each pair.  Returns a dict of device tensors: H [B,T,3,3] float64, inliers [B,T,M] bool (key-point-0
    indexing), num_inliers [B,T] int32, success [B,T] bool, best_hypothesis [B,T] int32, H_minimal [B,T,3,3] float64,
    thresholds [T], and error [B,T] when H_0to1 is given."""
    nat.require_cuda(kp0, "keypoints0")
    nat.require_cuda(kp1, "keypoints1")
    nat.require_cuda(matches0, "matches0")
    lib = nat.lib()
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    ths = [float(t) for t in ransac_th] if isinstance(ransac_th, (list, tuple, np.ndarray, torch.Tensor)) else [float(ransac_th)]
    t = len(ths)
    if (H_0to1 is None) != (image_size0 is None):
        raise ValueError("H_0to1 and image_size0 are given together or not at all")
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(torch.long).contiguous()
    if stream_id is None:
        sid = None
    elif isinstance(stream_id, torch.Tensor):
        sid = stream_id.to(device=dev, dtype=torch.long).reshape(b).contiguous()
    else:
        sid = torch.as_tensor(np.broadcast_to(np.asarray(stream_id, dtype=np.int64), (b,)).copy(), device=dev)
    H = size = err = None
    if H_0to1 is not None:
        H = H_0to1.to(device=dev, dtype=torch.float32).reshape(b, 9).contiguous()
        size = image_size0.to(device=dev, dtype=torch.float32).reshape(b, 2).contiguous()
        err = torch.empty((b, t), device=dev, dtype=torch.float32)
    Hout = torch.empty((b, t, 3, 3), device=dev, dtype=torch.float64)
    Hmin = torch.empty((b, t, 3, 3), device=dev, dtype=torch.float64)
    inl = torch.empty((b, t, m), device=dev, dtype=torch.uint8)
    ninl = torch.empty((b, t), device=dev, dtype=torch.int32)
    succ = torch.empty((b, t), device=dev, dtype=torch.uint8)
    besth = torch.empty((b, t), device=dev, dtype=torch.int32)
    th_host = (ctypes.c_float * max(t, 1))(*ths)
    nbytes = lib.gfc_eval_homography_ransac_workspace_bytes(b, m, t, int(num_hypotheses))
    ws = _ransac_ws.get(max(nbytes, 256), dev)
    nat.check(lib.gfc_eval_homography_ransac(nat.ptr(k0), nat.ptr(k1), nat.ptr(m0), nat.ptr(sid), nat.ptr(H),
                                             nat.ptr(size), b, m, n, th_host, t, int(num_hypotheses), int(lo_iters),
                                             int(seed) & _M64, nat.ptr(Hout), nat.ptr(inl), nat.ptr(ninl),
                                             nat.ptr(succ), nat.ptr(besth), nat.ptr(Hmin), nat.ptr(err), nat.ptr(ws),
                                             ws.numel(), nat.stream_ptr(dev)), "gfc_eval_homography_ransac")
    out = {"H": Hout, "inliers": inl.bool(), "num_inliers": ninl, "success": succ.bool(), "best_hypothesis": besth,
           "H_minimal": Hmin, "thresholds": torch.tensor(ths, dtype=torch.float32, device=dev)}
    if err is not None:
        out["error"] = err
    return out


def eval_homography_robust(data: dict, pred: dict, conf: dict) -> dict:
    """Drop-in for gluefactory.eval.utils.eval_homography_robust (eval/utils.py:225-273) for key points, with the GPU
    estimator: conf = {"estimator": "gfc_amd", "ransac_th": th} (+ optional num_hypotheses, lo_iters, seed, stream_id:
    an int, or one per item for batched input) -> {"H_error_ransac", "ransac_inl", "ransac_inl%"}; floats for
    un-batched input, lists per item for batched.  There is no CPU estimator here: any other name raises."""
    name = conf.get("estimator")
    if name not in RANSAC_ESTIMATORS:
        raise ValueError(f"unknown homography estimator {name!r}: available here: {list(RANSAC_ESTIMATORS)} "
                         "(the OpenCV / PoseLib estimators of the reference are CPU libraries this package does not use)")
    if "lines0" in pred or "keypoints0" not in pred:
        raise NotImplementedError("the gfc_amd homography estimator takes key-point matches only (no line features)")
    assert "H_0to1" in data, "Missing key H_0to1 in data"
    for key in ("keypoints0", "keypoints1", "matches0"):
        assert key in pred, f"Missing key {key} in data"
    H = data["H_0to1"]
    batched = H.ndim > 2
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    size = data["view0"]["image_size"]
    if not batched:
        H, kp0, kp1, m0, size = H[None], kp0[None], kp1[None], m0[None], size[None]
    res = homography_ransac(H, kp0, kp1, m0, size, float(conf["ransac_th"]),
                            num_hypotheses=conf.get("num_hypotheses", 2048), lo_iters=conf.get("lo_iters", 3),
                            seed=conf.get("seed", 0), stream_id=conf.get("stream_id"))
    err = [float(v) for v in res["error"][:, 0].cpu().tolist()]
    ninl = [float(v) for v in res["num_inliers"][:, 0].cpu().tolist()]
    nmatch = [int(v) for v in ((m0 > -1) & (m0 < kp1.shape[1])).sum(1).cpu().tolist()]
    frac = [a / max(c, 1) for a, c in zip(ninl, nmatch)]
    out = {"H_error_ransac": err, "ransac_inl": ninl, "ransac_inl%": frac}
    return out if batched else {k: v[0] for k, v in out.items()}
