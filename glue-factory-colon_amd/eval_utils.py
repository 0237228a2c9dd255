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
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    H = H_0to1.to(device=dev, dtype=torch.float32).reshape(b, 3, 3).contiguous()
    Hinv = torch.linalg.inv(H.double()).float().contiguous()  # 3x3 plumbing
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(torch.long).contiguous()
    out = torch.empty((b, 6), device=dev, dtype=torch.float32)
    gt = torch.empty((b, m), device=dev, dtype=torch.long) if return_gt else None
    nat.call("gfc_eval_matches_homography", k0, k1, m0, H, Hinv, b, m, n, float(pos_th), float(neg_th), out, gt)
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
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    H = H_0to1.to(device=dev, dtype=torch.float32).reshape(b, 9).contiguous()
    size = image_size0.to(device=dev, dtype=torch.float32).reshape(b, 2).contiguous()
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(torch.long).contiguous()
    sc = scores0.to(device=dev, dtype=torch.float32).contiguous()
    Hout = torch.empty((b, 3, 3), device=dev, dtype=torch.float32)
    err = torch.empty((b,), device=dev, dtype=torch.float32)
    nat.call("gfc_eval_homography_dlt", k0, k1, m0, sc, H, size, b, m, n, Hout, err)
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


def ransac_sample_indices(seed, stream_id, n, num_hypotheses, sample_size=4):
    """The minimal samples of the GPU estimators, index for index (csrc/ransac_common.h: rs_sample_k; DESIGN.md "Robust
    homography"): int64 [num_hypotheses, sample_size], distinct indices in [0, n) per hypothesis; sample_size 4 for the
    homography estimator, 5 for the relative-pose one.  Pure integer arithmetic: draw j of hypothesis h is
    u = mix64(key + GOLDEN * (sample_size h + j + 1)), key = mix64(mix64(seed + GOLDEN) ^ stream_id),
    r_j = ((u >> 32) * (n - j)) >> 32, and the r_j index a partial Fisher-Yates over the virtual array a[p] = p
    (take a[r_j], then move the last live element a[n - 1 - j] into the hole)."""
    n, k = int(n), int(sample_size)
    if k < 1:
        raise ValueError("sample_size >= 1")
    if n < k:
        raise ValueError(f"a minimal sample needs n >= {k} correspondences")
    with np.errstate(over="ignore"):
        key = _mix64(_mix64(np.uint64((int(seed) + _GOLDEN) & _M64)) ^ np.uint64(int(stream_id) & _M64))
        h = np.arange(int(num_hypotheses), dtype=np.uint64)
        r = []
        for j in range(k):
            u = _mix64(key + np.uint64(_GOLDEN) * (np.uint64(k) * h + np.uint64(j + 1)))
            r.append((((u >> np.uint64(32)) * np.uint64(n - j)) >> np.uint64(32)).astype(np.int64))
    holes, vals, out = [], [], []  # hole positions p_q and what was moved into them v_q, looked up latest first
    for j in range(k):
        idx, val = r[j], np.full_like(r[j], n - 1 - j)
        for p, v in zip(holes, vals):  # oldest first: a later hole overrides
            idx = np.where(r[j] == p, v, idx)
            val = np.where((n - 1 - j) == p, v, val)
        out.append(idx)
        holes.append(r[j])
        vals.append(val)
    return np.stack(out, axis=1).astype(np.int64)


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


class _RansacCall:
    """What `homography_ransac` and `relative_pose_ransac` share: the checked and cast inputs (k0, k1, m0), the threshold
    list, the stream ids as a [B] long tensor (or None), and the four outputs both estimators have."""

    def __init__(self, kp0, kp1, matches0, ransac_th, stream_id):
        nat.require_cuda(kp0, "keypoints0")
        nat.require_cuda(kp1, "keypoints1")
        nat.require_cuda(matches0, "matches0")
        self.dev = dev = kp0.device
        self.b, self.m, self.n = b, m, _ = kp0.shape[0], kp0.shape[1], kp1.shape[1]
        self.ths = [float(t) for t in ransac_th] if isinstance(ransac_th, (list, tuple, np.ndarray, torch.Tensor)) else [float(ransac_th)]
        self.t = t = len(self.ths)
        self.k0, self.k1 = kp0.float().contiguous(), kp1.float().contiguous()
        self.m0 = matches0.to(torch.long).contiguous()
        if stream_id is None:
            self.sid = None
        elif isinstance(stream_id, torch.Tensor):
            self.sid = stream_id.to(device=dev, dtype=torch.long).reshape(b).contiguous()
        else:
            self.sid = torch.as_tensor(np.broadcast_to(np.asarray(stream_id, dtype=np.int64), (b,)).copy(), device=dev)
        self.inl = torch.empty((b, t, m), device=dev, dtype=torch.uint8)
        self.succ = torch.empty((b, t), device=dev, dtype=torch.uint8)
        self.ninl, self.besth = self.empty(torch.int32), self.empty(torch.int32)
        self.th_host = (ctypes.c_float * max(t, 1))(*self.ths)

    def empty(self, dtype, *tail):
        """An output of shape [B, T, *tail]."""
        return torch.empty((self.b, self.t, *tail), device=self.dev, dtype=dtype)

    def workspace(self, holder, nbytes):
        return holder.get(max(nbytes, 256), self.dev)

    def common(self):
        """The result entries both estimators have, in the order they have them."""
        return {"inliers": self.inl.bool(), "num_inliers": self.ninl, "success": self.succ.bool(),
                "best_hypothesis": self.besth}

    def thresholds(self):
        return torch.tensor(self.ths, dtype=torch.float32, device=self.dev)


def homography_ransac(H_0to1, kp0, kp1, matches0, image_size0, ransac_th, *, num_hypotheses=2048, lo_iters=3, seed=0,
                      stream_id=None):
    """RANSAC homography for B pairs x T thresholds in one call of `gfc_eval_homography_ransac`.  Batched device
    tensors: kp0 [B,M,2], kp1 [B,N,2], matches0 [B,M]; H_0to1 [B,3,3] and image_size0 [B,2] together or both None
    (no error computed); ransac_th a float or a sequence of at most 8; stream_id None (0..B-1), an int or [B] ints:
    the random stream of each pair.  Returns a dict of device tensors: H [B,T,3,3] float64, inliers [B,T,M] bool (key-point-0
    indexing), num_inliers [B,T] int32, success [B,T] bool, best_hypothesis [B,T] int32, H_minimal [B,T,3,3] float64,
    thresholds [T], and error [B,T] when H_0to1 is given."""
    if (H_0to1 is None) != (image_size0 is None):
        raise ValueError("H_0to1 and image_size0 are given together or not at all")
    c = _RansacCall(kp0, kp1, matches0, ransac_th, stream_id)
    dev, b, t = c.dev, c.b, c.t
    H = size = err = None
    if H_0to1 is not None:
        H = H_0to1.to(device=dev, dtype=torch.float32).reshape(b, 9).contiguous()
        size = image_size0.to(device=dev, dtype=torch.float32).reshape(b, 2).contiguous()
        err = c.empty(torch.float32)
    Hout, Hmin = c.empty(torch.float64, 3, 3), c.empty(torch.float64, 3, 3)
    ws = c.workspace(_ransac_ws, nat.call("gfc_eval_homography_ransac_workspace_bytes", b, c.m, t, int(num_hypotheses)))
    nat.call("gfc_eval_homography_ransac", c.k0, c.k1, c.m0, c.sid, H, size, b, c.m, c.n, c.th_host, t,
             int(num_hypotheses), int(lo_iters), int(seed) & _M64, Hout, c.inl, c.ninl, c.succ, c.besth, Hmin, err, ws,
             ws.numel())
    out = {"H": Hout, **c.common(), "H_minimal": Hmin, "thresholds": c.thresholds()}
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


# ---- pose / depth match metrics (csrc/eval_pose.hip) -------------------------------------------------------------------
DEPTH_RESULT_KEYS = ("reproj_prec@1px", "reproj_prec@3px", "reproj_prec@5px", "covisible", "covisible_percent",
                     "gt_match_recall@3px", "gt_match_precision@3px")
EPIPOLAR_RESULT_KEYS = ("epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3", "num_matches", "num_keypoints")
POSE_RESULT_KEYS = ("rel_pose_error", "ransac_inl", "ransac_inl%")


def _pair_geometry(camera0, camera1, T_0to1, batch, device):
    from . import geometry

    cam0, model0 = geometry.camera_args(camera0, batch, device)
    cam1, model1 = geometry.camera_args(camera1, batch, device)
    T01, T10 = geometry.pose_args(T_0to1, batch, device)
    return cam0, model0, cam1, model1, T01, T10


def _depth_arg(depth, batch, device):
    d = depth.to(device=device, dtype=torch.float32)
    d = d.reshape((-1,) + tuple(d.shape[-2:])).contiguous()
    assert d.shape[0] == batch, f"{d.shape[0]} depth maps for {batch} pairs"
    return d


def pose_project(kp, depth_i, camera_i, camera_j, T_itoj):
    """`sample_depth` + `project(ccth=None)` of the reference (geometry/depth.py) for batched device tensors: kp [B,K,2],
    depth_i [B,H,W], cameras / pose as holders of B items (geometry.Camera / Pose or the reference's wrappers) ->
    (depth_kp [B,K], valid [B,K] bool, proj [B,K,2], visible [B,K] bool)."""
    from . import geometry

    nat.require_cuda(kp, "keypoints")
    dev, (b, k) = kp.device, kp.shape[:2]
    cam_i, model_i = geometry.camera_args(camera_i, b, dev)
    cam_j, model_j = geometry.camera_args(camera_j, b, dev)
    T, _ = geometry.pose_args(T_itoj, b, dev)
    depth = _depth_arg(depth_i, b, dev)
    pts = kp.float().contiguous()
    d = torch.empty((b, k), device=dev, dtype=torch.float32)
    proj = torch.empty((b, k, 2), device=dev, dtype=torch.float32)
    valid = torch.empty((b, k), device=dev, dtype=torch.uint8)
    visible = torch.empty((b, k), device=dev, dtype=torch.uint8)
    nat.call("gfc_eval_pose_project", pts, depth, cam_i, model_i, cam_j, model_j, T, b, k, depth.shape[1], depth.shape[2],
             d, valid, proj, visible)
    return d, valid.bool(), proj, visible.bool()


def pose_depth_metrics(kp0, kp1, matches0, depth0, depth1, camera0, camera1, T_0to1, pos_th=3.0, neg_th=5.0,
                       return_gt=False):
    """Batched tensors on the device: kp0 [B,M,2], kp1 [B,N,2], matches0 [B,M], depth0 [B,H0,W0], depth1 [B,H1,W1],
    cameras and pose as holders of B items -> [B,7] (DEPTH_RESULT_KEYS order) and optionally the ground-truth matches
    of both views ([B,M], [B,N]; -1 unmatched, -2 ignore)."""
    nat.require_cuda(kp0, "keypoints0")
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    cam0, model0, cam1, model1, T01, T10 = _pair_geometry(camera0, camera1, T_0to1, b, dev)
    d0, d1 = _depth_arg(depth0, b, dev), _depth_arg(depth1, b, dev)
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(device=dev, dtype=torch.long).contiguous()
    out = torch.empty((b, 7), device=dev, dtype=torch.float32)
    gt0 = torch.empty((b, m), device=dev, dtype=torch.long) if return_gt else None
    gt1 = torch.empty((b, n), device=dev, dtype=torch.long) if return_gt else None
    nat.call("gfc_eval_matches_depth", k0, k1, m0, d0, d1, cam0, model0, cam1, model1, T01, T10, b, m, n, d0.shape[1],
             d0.shape[2], d1.shape[1], d1.shape[2], float(pos_th), float(neg_th), out, gt0, gt1)
    return (out, gt0, gt1) if return_gt else out


def pose_epipolar_metrics(kp0, kp1, matches0, camera0, camera1, T_0to1):
    """Batched tensors on the device -> [B,5] (EPIPOLAR_RESULT_KEYS order)."""
    nat.require_cuda(kp0, "keypoints0")
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    cam0, model0, cam1, model1, T01, _ = _pair_geometry(camera0, camera1, T_0to1, b, dev)
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()
    m0 = matches0.to(device=dev, dtype=torch.long).contiguous()
    out = torch.empty((b, 5), device=dev, dtype=torch.float32)
    nat.call("gfc_eval_matches_epipolar", k0, k1, m0, cam0, model0, cam1, model1, T01, b, m, n, out)
    return out


def _pose_inputs(data, pred, need_depth):
    for key in ("view0", "view1", "T_0to1"):
        assert key in data, f"Missing key {key} in data"
    for key in ("keypoints0", "keypoints1", "matches0", "matching_scores0"):
        assert key in pred, f"Missing key {key} in pred"
    for view in ("view0", "view1"):
        for key in (("depth", "camera") if need_depth else ("camera",)):
            assert key in data[view], f"Missing key {key} in data[{view}]"
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    batched = kp0.ndim > 2
    if not batched:  # the reference's loop: a loader item of batch 1 with an un-batched cached record
        kp0, kp1, m0 = kp0[None], kp1[None], m0[None]
    return batched, kp0, kp1, m0


def _metric_dict(res, keys, batched, integer=()):
    out = {}
    for i, key in enumerate(keys):
        vals = [int(v) if key in integer else float(v) for v in res[:, i].tolist()]
        out[key] = vals if batched else vals[0]
    return out


def eval_matches_epipolar(data: dict, pred: dict) -> dict:
    """Drop-in for gluefactory.eval.utils.eval_matches_epipolar (eval/utils.py:45-74), same keys: un-batched key
    points give scalars, batched ones lists per item."""
    batched, kp0, kp1, m0 = _pose_inputs(data, pred, need_depth=False)
    res = pose_epipolar_metrics(kp0, kp1, m0, data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]).cpu()
    return _metric_dict(res, EPIPOLAR_RESULT_KEYS, batched, integer=("num_matches",))


def eval_matches_depth(data: dict, pred: dict) -> dict:
    """Drop-in for gluefactory.eval.utils.eval_matches_depth (eval/utils.py:77-138), same keys: un-batched key points
    give scalars, batched ones lists per item."""
    batched, kp0, kp1, m0 = _pose_inputs(data, pred, need_depth=True)
    res = pose_depth_metrics(kp0, kp1, m0, data["view0"]["depth"], data["view1"]["depth"], data["view0"]["camera"],
                             data["view1"]["camera"], data["T_0to1"]).cpu()
    return _metric_dict(res, DEPTH_RESULT_KEYS, batched)


def gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3, neg_th=5, epi_th=None, cc_th=None):
    """Counterpart of gluefactory.geometry.gt_generation.gt_matches_from_pose_depth (gt_generation.py:594-727) for
    batched device key points kp0 [B,M,2], kp1 [B,N,2] and the reference's data dict (`view0/1` = {camera, depth},
    `T_0to1`): `matches0/1`, `matching_scores0/1`, `depth_keypoints0/1`, `proj_0to1/1to0`, `visible0/1`.
    `assignment` and `reward` are NOT returned: they are the M x N matrices this path exists to avoid.  `epi_th` and
    `cc_th` (None wherever the evaluation calls this) are not built."""
    if epi_th is not None or cc_th is not None:
        raise NotImplementedError("gt_matches_from_pose_depth: epi_th / cc_th are not built (the evaluation passes None)")
    cam0, cam1, T = data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]
    depth0, depth1 = data["view0"]["depth"], data["view1"]["depth"]
    b = kp0.shape[0]
    from . import geometry

    T01, T10 = geometry.pose_args(T, b, kp0.device)
    d0, _, p01, vis0 = pose_project(kp0, depth0, cam0, cam1, geometry.Pose(T01))
    d1, _, p10, vis1 = pose_project(kp1, depth1, cam1, cam0, geometry.Pose(T10))
    if kp0.shape[1] == 0 or kp1.shape[1] == 0:  # the reference returns no visibility for an empty side
        vis0, vis1 = torch.zeros_like(vis0), torch.zeros_like(vis1)
    m0 = torch.full(kp0.shape[:2], -1, dtype=torch.long, device=kp0.device)
    _, g0, g1 = pose_depth_metrics(kp0, kp1, m0, depth0, depth1, cam0, cam1, T, pos_th, neg_th, return_gt=True)
    return {"matches0": g0, "matches1": g1, "matching_scores0": (g0 > -1).float(), "matching_scores1": (g1 > -1).float(),
            "depth_keypoints0": d0, "depth_keypoints1": d1, "proj_0to1": p01, "proj_1to0": p10, "visible0": vis0,
            "visible1": vis1}


def relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0):
    """gluefactory.geometry.epipolar.relative_pose_error (epipolar.py:139-155): (t_err, r_err) in degrees between an
    estimated (R, t) and the true pose (a pose holder of one item, or a [4,4] tensor).  The translation angle is taken
    up to sign (an essential matrix fixes t only up to sign).  3 x 3 host work: torch on the CPU, in float64, and each
    angle as atan2(sine, cosine) -- the reference's float32 acos(cosine) is the same angle with an error of
    6e-8 / sin(angle) radians, which scores a perfect estimate at up to 0.03 degrees."""
    if isinstance(T_0to1, torch.Tensor):
        R_gt, t_gt = T_0to1[:3, :3], T_0to1[:3, 3]
    else:
        flat = T_0to1._data.reshape(-1)
        R_gt, t_gt = flat[:9].reshape(3, 3), flat[9:]
    R_gt, t_gt = R_gt.detach().cpu().double(), t_gt.detach().cpu().double()
    R, t = torch.as_tensor(R).detach().cpu().double(), torch.as_tensor(t).detach().cpu().double().reshape(3)
    t_err = torch.rad2deg(torch.atan2(torch.linalg.cross(t, t_gt).norm(), (t * t_gt).sum()))
    t_err = torch.minimum(t_err, 180 - t_err)
    if t_gt.norm() < ignore_gt_t_thr:  # pure rotation: the direction of t means nothing
        t_err = torch.zeros((), dtype=torch.float64)
    D = R.T @ R_gt  # the rotation between the two: its angle from the antisymmetric part (sine) and the trace (cosine)
    axis = torch.stack([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    r_err = torch.rad2deg(torch.atan2(axis.norm() / 2, (D.trace() - 1) / 2))
    return t_err, r_err


RELATIVE_POSE_ESTIMATORS = ("gfc_amd",)
_relpose_ws = nat.Workspace()


def pose_image2cam(kp, camera):
    """`Camera.image2cam` of the reference for batched device key points kp [B,K,2] (pixels) and a holder of B cameras
    -> [B,K,2] float32 points on the z = 1 plane (only OPENCV_FISHEYE removes its distortion): the bearings the
    relative-pose estimator works on, from the same device function."""
    from . import geometry

    nat.require_cuda(kp, "keypoints")
    dev, (b, k) = kp.device, kp.shape[:2]
    cam, model = geometry.camera_args(camera, b, dev)
    pts = kp.float().contiguous()
    out = torch.empty((b, k, 2), device=dev, dtype=torch.float32)
    nat.call("gfc_eval_pose_image2cam", pts, cam, model, b, k, out)
    return out


def relative_pose_ransac(kp0, kp1, matches0, camera0, camera1, ransac_th, T_0to1=None, *, num_hypotheses=2048,
                         lo_iters=3, seed=0, stream_id=None, ignore_gt_t_thr=0.0):
    """Five-point RANSAC relative pose for B pairs x T thresholds in one call of `gfc_eval_relative_pose_ransac`
    (csrc/relpose.hip; DESIGN.md "Robust relative pose").  Batched device tensors: kp0 [B,M,2], kp1 [B,N,2] in pixels,
    matches0 [B,M]; cameras (and the optional true pose T_0to1) as holders of B items (geometry.Camera / Pose or the
    reference's wrappers); ransac_th in pixels, a float or a sequence of at most 8 (a pair uses th / mean(fx0, fy0, fx1,
    fy1)); stream_id None (0..B-1), an int or [B] ints: the random stream of each pair.  Returns a dict of device
    tensors: R [B,T,3,3], t [B,T,3] (unit), E [B,T,3,3] = [t]x R, E_minimal [B,T,3,3] float64; inliers [B,T,M] bool
    (key-point-0 indexing); num_inliers, best_hypothesis, best_solution [B,T] int32; success [B,T] bool; thresholds [T];
    with T_0to1 also r_err, t_err [B,T] float64 degrees (t up to sign).  Convention X1 = R X0 + t."""
    from . import geometry

    c = _RansacCall(kp0, kp1, matches0, ransac_th, stream_id)
    dev, b, t = c.dev, c.b, c.t
    cam0, model0 = geometry.camera_args(camera0, b, dev)
    cam1, model1 = geometry.camera_args(camera1, b, dev)
    T01 = rerr = terr = None
    if T_0to1 is not None:
        T01, _ = geometry.pose_args(T_0to1, b, dev)
        rerr, terr = c.empty(torch.float64), c.empty(torch.float64)
    R, tv = c.empty(torch.float64, 3, 3), c.empty(torch.float64, 3)
    E, Emin = c.empty(torch.float64, 3, 3), c.empty(torch.float64, 3, 3)
    bestk = c.empty(torch.int32)
    ws = c.workspace(_relpose_ws,
                     nat.call("gfc_eval_relative_pose_ransac_workspace_bytes", b, c.m, t, int(num_hypotheses)))
    nat.call("gfc_eval_relative_pose_ransac", c.k0, c.k1, c.m0, c.sid, cam0, model0, cam1, model1, T01, b, c.m, c.n,
             c.th_host, t, int(num_hypotheses), int(lo_iters), int(seed) & _M64, float(ignore_gt_t_thr), R, tv, E, Emin,
             c.inl, c.ninl, c.succ, c.besth, bestk, rerr, terr, ws, ws.numel())
    out = {"R": R, "t": tv, "E": E, "E_minimal": Emin, **c.common(), "best_solution": bestk,
           "thresholds": c.thresholds()}
    if rerr is not None:
        out["r_err"], out["t_err"] = rerr, terr
    return out


def relative_pose_estimator_from_conf(conf):
    """The estimator object a conf names: {"estimator": "gfc_amd", "ransac_th": th [, num_hypotheses, lo_iters, seed,
    stream_id]} -> relative_pose_estimator.GpuRelativePoseEstimator.  Any other name: NotImplementedError."""
    name = conf.get("estimator")
    if name not in RELATIVE_POSE_ESTIMATORS:
        raise NotImplementedError(
            f"no relative-pose estimator {name!r} here: the five-point RANSAC estimator of this package is 'gfc_amd' "
            "(the reference delegates to OpenCV / PoseLib / pycolmap, CPU libraries this package does not use); "
            "pass an estimator object")
    from .relative_pose_estimator import GpuRelativePoseEstimator

    options = {k: conf[k] for k in ("num_hypotheses", "lo_iters", "seed", "stream_id") if conf.get(k) is not None}
    return GpuRelativePoseEstimator({"ransac_th": float(conf["ransac_th"]), "options": options})


def eval_relative_pose_robust(data: dict, pred: dict, conf: dict, estimator=None) -> dict:
    """gluefactory.eval.utils.eval_relative_pose_robust (eval/utils.py:188-222): `rel_pose_error` (the larger of the
    rotation and translation angles, degrees), `ransac_inl`, `ransac_inl%` of one pair.  The estimator is an OBJECT of
    the reference's interface -- estimator({"m_kpts0", "m_kpts1", "camera0", "camera1"}) -> {"success", "M_0to1" (a
    pose holder), "inliers"} -- or, without one, what conf names: {"estimator": "gfc_amd", "ransac_th": th} is this
    package's GPU five-point RANSAC (relative_pose_estimator.GpuRelativePoseEstimator); any other name raises
    NotImplementedError."""
    if estimator is None:
        estimator = relative_pose_estimator_from_conf(conf)
    batched, kp0, kp1, m0 = _pose_inputs(data, pred, need_depth=False)
    if batched:
        raise ValueError("eval_relative_pose_robust takes one pair (un-batched key points), as the reference")
    sel = m0[0] > -1
    cam0, cam1 = data["view0"]["camera"], data["view1"]["camera"]
    est = estimator({"m_kpts0": kp0[0][sel], "m_kpts1": kp1[0][m0[0][sel]],
                     "camera0": cam0[0] if cam0._data.ndim > 1 else cam0,
                     "camera1": cam1[0] if cam1._data.ndim > 1 else cam1})
    if not est["success"]:
        return {"rel_pose_error": float("inf"), "ransac_inl": 0, "ransac_inl%": 0}
    M = est["M_0to1"]
    inl = np.asarray(torch.as_tensor(est["inliers"]).cpu())
    flat = M._data.reshape(-1)
    t_err, r_err = relative_pose_error(data["T_0to1"], flat[:9].reshape(3, 3), flat[9:])
    return {"rel_pose_error": float(max(r_err, t_err)), "ransac_inl": float(np.sum(inl)),
            "ransac_inl%": 0 if inl.size == 0 else float(np.mean(inl))}


def eval_poses(pose_results, auc_ths, key, unit="°"):
    """gluefactory.eval.utils.eval_poses (eval/utils.py:305-331): {threshold: {key: per-pair list, ...}} ->
    (summaries, best threshold).  The threshold reported is the one with the highest mean AUC of `key` (the first on
    a tie); summaries hold `<key>@<t><unit>`, `<key>_mAA` and med_ / mean_ of its numeric lists."""
    from .eval_hpatches import cal_error_auc

    aucs = {th: cal_error_auc(lists[key], list(auc_ths)) for th, lists in pose_results.items()}
    maas = {th: float(np.mean(a)) for th, a in aucs.items()}
    best_th = max(maas, key=maas.get)
    summaries = {f"{key}@{t}{unit}": float(a) for t, a in zip(auc_ths, aucs[best_th])}
    summaries[f"{key}_mAA"] = maas[best_th]
    for k, v in pose_results[best_th].items():
        arr = np.array(v)
        if np.issubdtype(arr.dtype, np.number):
            summaries[f"med_{k}"] = round(float(np.median(arr)), 3)
            summaries[f"mean_{k}"] = round(float(np.mean(arr)), 3)
    return summaries, best_th
