"""Ground-truth matches from a homography -- counterpart of gluefactory/models/matchers/homography_matcher.py, the
`ground_truth` component of the homography training / validation configurations.

`gt_matches_from_homography` (geometry/gt_generation.py:730-801) runs in `gfc_gt_matches_homography`
(csrc/gt_matches.hip): one workgroup per pair, no M x N matrix for `matches0/1` and the projections; the dense
`assignment` / `reward` are a second launch.  MI355X addition: `dense_outputs: False` omits those two keys and never
allocates them (the validation loss then reads its positives from `matches0`, the same set whenever
th_positive <= th_negative -- anything else is refused here).
"""
import torch

from . import _native as nat
from .base_model import BaseModel


def gt_matches_from_homography(kp0, kp1, H, pos_th=3, neg_th=6, valid_mask0=None, valid_mask1=None, dense=True):
    """The reference's function for batched device tensors kp0 [B,M,2], kp1 [B,N,2], H [B,3,3] (masks [B,M], [B,N] bool
    or None): its eight keys, or six without `assignment` / `reward` when dense is False."""
    nat.require_cuda(kp0, "keypoints0")
    nat.require_cuda(kp1, "keypoints1")
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    # (an empty side, gt_generation.py:735-753: the entry launches nothing and sets the other side's matches to -1; the
    # projections stay unwritten like the reference's torch.empty_like, the dense outputs have no element)
    Hm = H.to(device=dev, dtype=torch.float32).reshape(b, 3, 3).contiguous()
    Hinv = torch.linalg.inv(Hm.double()).float().contiguous()  # 3x3 plumbing, as eval_utils.match_metrics
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()

    def mask(v, k):
        return None if v is None else v.to(device=dev).reshape(b, k).ne(0).contiguous()

    v0, v1 = mask(valid_mask0, m), mask(valid_mask1, n)
    m0 = torch.empty((b, m), dtype=torch.long, device=dev)
    m1 = torch.empty((b, n), dtype=torch.long, device=dev)
    p01, p10 = torch.empty_like(k0), torch.empty_like(k1)
    pos0 = assignment = reward = None
    if dense:
        pos0 = torch.empty((b, m), dtype=torch.int32, device=dev)
        assignment = torch.empty((b, m, n), dtype=torch.bool, device=dev)
        reward = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    nat.call("gfc_gt_matches_homography", k0, k1, Hm, Hinv, v0, v1, b, m, n, float(pos_th), float(neg_th), m0, m1, p01,
             p10, pos0, assignment, reward)
    out = {"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(),
           "matching_scores1": (m1 > -1).float(), "proj_0to1": p01, "proj_1to0": p10}
    if dense:
        out["assignment"], out["reward"] = assignment, reward
    return out


class HomographyMatcher(BaseModel):
    default_conf = {
        # GT parameters for points
        "use_points": True,
        "th_positive": 3.0,
        "th_negative": 3.0,
        # GT parameters for lines
        "use_lines": False,
        "n_line_sampled_pts": 50,
        "line_perp_dist_th": 5,
        "overlap_th": 0.2,
        "min_visibility_th": 0.5,
        # MI355X addition: False leaves `assignment` and `reward` ([B,M,N]) out of the result and never allocates them
        "dense_outputs": True,
    }
    required_data_keys = ["H_0to1"]

    def _init(self, conf):
        if conf.use_lines:
            raise NotImplementedError("homography_matcher: use_lines (line ground truth) is not built")
        if not conf.dense_outputs and conf.th_positive > conf.th_negative:
            raise NotImplementedError(
                "homography_matcher: dense_outputs False needs th_positive <= th_negative (a point could otherwise be "
                "both positive in `assignment` and unmatched in `matches0`, and the sparse labels would lose it)")
        if conf.use_points:
            self.required_data_keys += ["keypoints0", "keypoints1"]

    def _forward(self, data):
        if not self.conf.use_points:
            return {}
        return gt_matches_from_homography(
            data["keypoints0"], data["keypoints1"], data["H_0to1"], pos_th=self.conf.th_positive,
            neg_th=self.conf.th_negative, valid_mask0=data.get("valid_depth_keypoints0", None),
            valid_mask1=data.get("valid_depth_keypoints1", None), dense=bool(self.conf.dense_outputs))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = HomographyMatcher
