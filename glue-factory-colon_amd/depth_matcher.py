"""Ground-truth matches from pose and depth -- counterpart of gluefactory/models/matchers/depth_matcher.py, the
`ground_truth` component of the MegaDepth / posed-image training and validation configurations.

`gt_matches_from_pose_depth` (geometry/gt_generation.py:594-727) with `th_epi`: the projections come from
`gfc_eval_pose_project` (depth sampled from the maps) or `gfc_gt_project_depth` (cached `depth_keypoints0/1`), the
matching, the epi_th rule and the dense `assignment` / `reward` from `gfc_gt_matches_depth` (csrc/gt_matches.hip): one
workgroup per pair, no M x N matrix for the sparse outputs.  MI355X addition: `dense_outputs: False` omits `assignment`
and `reward` and never allocates them (refused when th_positive > th_negative, as in homography_matcher).
`eval_utils.gt_matches_from_pose_depth` (the evaluation's form, no epi_th) is unchanged.
"""
import torch

from . import _native as nat
from . import eval_utils, geometry
from .base_model import BaseModel


def fundamental_matrix(cam0, cam1, T01):
    """F = K1^-T [t]x R K0^-1 (gt_generation.py:697-701, epipolar.py:7-9) in float32 from the packed arguments of the
    library: cameras [B,10] = w, h, fx, fy, cx, cy, ..., pose [B,12] = R row-major, t.  3 x 3 plumbing."""
    def K(cam):
        k = torch.zeros((cam.shape[0], 3, 3), dtype=torch.float32, device=cam.device)
        k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = cam[:, 2], cam[:, 3], cam[:, 4], cam[:, 5], 1.0
        return k

    R, t = T01[:, :9].reshape(-1, 3, 3), T01[:, 9:]
    z = torch.zeros_like(t[:, 0])
    skew = torch.stack([z, -t[:, 2], t[:, 1], t[:, 2], z, -t[:, 0], -t[:, 1], t[:, 0], z], -1).reshape(-1, 3, 3)
    return (K(cam1).inverse().transpose(-1, -2) @ (skew @ R) @ K(cam0).inverse()).contiguous()


def mask(v, b, k, dev):
    """Any mask of a side as contiguous bool [B,K] on the device."""
    return v.to(device=dev).reshape(b, k).ne(0).contiguous()


def project_given_depth(k, d, valid, ci, mi, cj, mj, T, project=True):
    """Key points k [B,K,2] of view i whose depth d is GIVEN (cached, or from a sparse map) into view j: (depth float32
    [B,K], valid bool, the projection, visible = valid depth and a valid projection).  project False is the reference's
    early return for an empty side: nothing is projected and nothing is visible."""
    dev, (b, cnt) = k.device, k.shape[:2]
    d, valid = d.to(device=dev, dtype=torch.float32).reshape(b, cnt).contiguous(), mask(valid, b, cnt, dev)
    proj = torch.empty((b, cnt, 2), dtype=torch.float32, device=dev)
    vis = torch.zeros((b, cnt), dtype=torch.bool, device=dev)
    if project:
        nat.call("gfc_gt_project_depth", k, d, valid, ci, mi, cj, mj, T, b, cnt, proj, vis, device=dev)
    return d, valid, proj, vis


def gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3, neg_th=5, epi_th=None, cc_th=None, dense=True, **kw):
    """The reference's function for batched device key points kp0 [B,M,2], kp1 [B,N,2] and its data dict (`view0/1` =
    {camera, depth}, `T_0to1`); kw: `depth_keypoints0/1` + `valid_depth_keypoints0/1` (cached depth), or
    `valid_depth_keypoints0/1` alone (ANDed with the sampled validity).  Its twelve keys, ten without dense."""
    if cc_th is not None:
        raise NotImplementedError("gt_matches_from_pose_depth: cc_th (th_consistency) is not built")
    nat.require_cuda(kp0, "keypoints0")
    nat.require_cuda(kp1, "keypoints1")
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    cam0, model0 = geometry.camera_args(data["view0"]["camera"], b, dev)
    cam1, model1 = geometry.camera_args(data["view1"]["camera"], b, dev)
    T01, T10 = geometry.pose_args(data["T_0to1"], b, dev)
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()

    if "depth_keypoints0" in kw and "depth_keypoints1" in kw:
        both = m > 0 and n > 0
        d0, valid0, p01, vis0 = project_given_depth(k0, kw["depth_keypoints0"], kw["valid_depth_keypoints0"], cam0,
                                                    model0, cam1, model1, T01, both)
        d1, valid1, p10, vis1 = project_given_depth(k1, kw["depth_keypoints1"], kw["valid_depth_keypoints1"], cam1,
                                                    model1, cam0, model0, T10, both)
    else:
        depth0, depth1 = data["view0"].get("depth"), data["view1"].get("depth")
        assert depth0 is not None and depth1 is not None
        d0, valid0, p01, vis0 = eval_utils.pose_project(k0, depth0, data["view0"]["camera"], data["view1"]["camera"],
                                                        geometry.Pose(T01))
        d1, valid1, p10, vis1 = eval_utils.pose_project(k1, depth1, data["view1"]["camera"], data["view0"]["camera"],
                                                        geometry.Pose(T10))
        if "valid_depth_keypoints0" in kw:  # visible = valid & a valid projection: the AND carries over
            g0, g1 = mask(kw["valid_depth_keypoints0"], b, m, dev), mask(kw["valid_depth_keypoints1"], b, n, dev)
            valid0, valid1, vis0, vis1 = valid0 & g0, valid1 & g1, vis0 & g0, vis1 & g1
    m0 = torch.empty((b, m), dtype=torch.long, device=dev)
    m1 = torch.empty((b, n), dtype=torch.long, device=dev)
    pos0 = assignment = reward = None
    if dense:
        pos0 = torch.empty((b, m), dtype=torch.int32, device=dev)
        assignment = torch.empty((b, m, n), dtype=torch.bool, device=dev)
        reward = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    if m == 0 or n == 0:  # gt_generation.py:598-634: no projection, nothing visible
        p01, p10 = torch.empty_like(k0), torch.empty_like(k1)
        vis0, vis1 = torch.zeros((b, m), dtype=torch.bool, device=dev), torch.zeros((b, n), dtype=torch.bool, device=dev)
    F = fundamental_matrix(cam0, cam1, T01) if (dense or epi_th is not None) else None
    nat.call("gfc_gt_matches_depth", k0, k1, p01, p10, vis0.contiguous(), vis1.contiguous(), valid0.contiguous(),
             valid1.contiguous(), F, b, m, n, float(pos_th), float(neg_th), -1.0 if epi_th is None else float(epi_th),
             m0, m1, pos0, assignment, reward, device=dev)
    out = {"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(), "matching_scores1": (m1 > -1).float(),
           "depth_keypoints0": d0, "depth_keypoints1": d1, "proj_0to1": p01, "proj_1to0": p10, "visible0": vis0,
           "visible1": vis1}
    if dense:
        out["assignment"], out["reward"] = assignment, reward
    return out


class DepthMatcher(BaseModel):
    default_conf = {
        # GT parameters for points
        "use_points": True,
        "th_positive": 3.0,
        "th_negative": 5.0,
        "th_epi": None,  # add some more epi outliers
        "th_consistency": None,  # check for projection consistency in px
        # GT parameters for lines
        "use_lines": False,
        "n_line_sampled_pts": 50,
        "line_perp_dist_th": 5,
        "overlap_th": 0.2,
        "min_visibility_th": 0.5,
        # MI355X addition: False leaves `assignment` and `reward` ([B,M,N]) out of the result and never allocates them
        "dense_outputs": True,
    }
    required_data_keys = ["view0", "view1", "T_0to1"]

    def _init(self, conf):
        if conf.use_lines:
            raise NotImplementedError("depth_matcher: use_lines (line ground truth) is not built")
        if conf.th_consistency is not None:
            raise NotImplementedError("depth_matcher: th_consistency is not built (no configuration sets it)")
        if conf.th_epi is not None and conf.th_epi < 0:
            raise ValueError("depth_matcher: th_epi must not be negative")
        if not conf.dense_outputs and conf.th_positive > conf.th_negative:
            raise NotImplementedError(
                "depth_matcher: dense_outputs False needs th_positive <= th_negative (a point could otherwise be both "
                "positive in `assignment` and unmatched in `matches0`, and the sparse labels would lose it)")
        if conf.use_points:
            self.required_data_keys += ["keypoints0", "keypoints1"]

    def _forward(self, data):
        if not self.conf.use_points:
            return {}
        if "depth_keypoints0" in data:
            keys = ["depth_keypoints0", "valid_depth_keypoints0", "depth_keypoints1", "valid_depth_keypoints1"]
        elif "valid_depth_keypoints0" in data:
            keys = ["valid_depth_keypoints0", "valid_depth_keypoints1"]
        else:
            keys = []
        return gt_matches_from_pose_depth(
            data["keypoints0"], data["keypoints1"], data, pos_th=self.conf.th_positive, neg_th=self.conf.th_negative,
            epi_th=self.conf.th_epi, cc_th=self.conf.th_consistency, dense=bool(self.conf.dense_outputs),
            **{k: data[k] for k in keys})

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = DepthMatcher
