"""Ground-truth matches from an Endomapper sparse map -- counterpart of gluefactory/models/matchers/
sparse_depth_matcher.py, the `ground_truth` component of CudaSift+lightglue_endomapper.yaml.

`gt_matches_from_pose_sparse_map` (geometry/gt_generation.py:441-591): labels seeded by 3D-point identity (`use_gt_pos`),
then mutual nearest neighbours of the reprojection, negatives and the th_epi rule, none of which overrides an earlier
decision; th_positive, th_negative and th_epi may each be None.  The projections come from `gfc_gt_project_depth` (the
sparse depth per key point), everything else from `gfc_gt_matches_sparse_map` (csrc/gt_sparse_map.hip), which splits a
pair over workgroups.  Its twenty keys are returned, the eight `mask_*` as bool.
MI355X addition: `dense_outputs: False` omits `assignment` and `reward`, never allocates them and returns
`extra_positives` [B] int32 instead: the number of positives of `assignment` that `matches0` does not name (duplicate
ids, or a distance positive beside a seed), which a loss that sees only `matches0` loses.  Positives keep precedence over
negatives here, so th_positive > th_negative needs no refusal.
`save_fig_when_debug` is accepted and ignored with one warning: this package draws nothing.
An empty side follows the dict of the sparse-dense function (:282-314); the early return of the sparse-map function
(:453-461) is a tuple its caller cannot use.
"""
import logging

import torch

from . import _native as nat
from . import geometry
from .base_model import BaseModel
from .depth_matcher import fundamental_matrix, mask, project_given_depth

logger = logging.getLogger(__name__)
MASK_KEYS = ("mask_pos_3d_map", "mask_pos_reproj", "mask_neg_reproj", "mask_neg_epi")  # the rows of masks0 / masks1
_workspace = nat.Workspace()


def gt_matches_from_sparse_map(kp0, kp1, data, depth0, valid0, depth1, valid1, ids0=None, ids1=None, valid3d0=None,
                               valid3d1=None, pos_th=3.0, neg_th=5.0, epi_th=None, cc_th=None, dense=True):
    """Both reference functions for batched device key points kp0 [B,M,2], kp1 [B,N,2], the depth per key point and its
    validity, and the data dict (`view0/1` = {camera}, `T_0to1`).  ids0/ids1 (with valid3d0/1) seed the labels; None:
    no seeding (use_gt_pos False, or the sparse-dense function)."""
    if cc_th is not None:
        raise NotImplementedError("sparse-map ground truth: cc_th (th_consistency) is not built")
    nat.require_cuda(kp0, "keypoints0")
    nat.require_cuda(kp1, "keypoints1")
    dev = kp0.device
    b, m, n = kp0.shape[0], kp0.shape[1], kp1.shape[1]
    cam0, model0 = geometry.camera_args(data["view0"]["camera"], b, dev)
    cam1, model1 = geometry.camera_args(data["view1"]["camera"], b, dev)
    T01, T10 = geometry.pose_args(data["T_0to1"], b, dev)
    k0, k1 = kp0.float().contiguous(), kp1.float().contiguous()

    both = m > 0 and n > 0  # the early return projects nothing: nothing visible
    _, valid0, p01, vis0 = project_given_depth(k0, depth0, valid0, cam0, model0, cam1, model1, T01, both)
    _, valid1, p10, vis1 = project_given_depth(k1, depth1, valid1, cam1, model1, cam0, model0, T10, both)
    seeded = ids0 is not None
    if seeded:
        ids0 = ids0.to(device=dev, dtype=torch.long).reshape(b, m).contiguous()
        ids1 = ids1.to(device=dev, dtype=torch.long).reshape(b, n).contiguous()
        valid3d0, valid3d1 = mask(valid3d0, b, m, dev), mask(valid3d1, b, n, dev)
    else:
        valid3d0 = valid3d1 = None
    m0 = torch.empty((b, m), dtype=torch.long, device=dev)
    m1 = torch.empty((b, n), dtype=torch.long, device=dev)
    masks0 = torch.empty((b, 4, m), dtype=torch.bool, device=dev)
    masks1 = torch.empty((b, 4, n), dtype=torch.bool, device=dev)
    assignment = reward = extra = None
    if dense:
        assignment = torch.empty((b, m, n), dtype=torch.bool, device=dev)
        reward = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    else:
        extra = torch.empty((b,), dtype=torch.int32, device=dev)
    need_f = epi_th is not None or (dense and neg_th is not None)
    F = fundamental_matrix(cam0, cam1, T01) if need_f else None
    nbytes = nat.call("gfc_gt_matches_sparse_map_workspace_bytes", b, m, n)
    ws = _workspace.get(max(nbytes, 1), dev)
    none = lambda v: -1.0 if v is None else float(v)  # noqa: E731
    nat.call("gfc_gt_matches_sparse_map", k0, k1, p01, p10, vis0, vis1, valid0, valid1, ids0, ids1, valid3d0, valid3d1,
             F, b, m, n, none(pos_th), none(neg_th), none(epi_th), m0, m1, masks0, masks1, None, extra, assignment,
             reward, ws, nbytes, device=dev)
    out = {"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(), "matching_scores1": (m1 > -1).float(),
           "depth_keypoints0": depth0, "depth_keypoints1": depth1, "proj_0to1": p01, "proj_1to0": p10,
           "visible0": vis0, "visible1": vis1}
    for r, key in enumerate(MASK_KEYS):
        out[key + "0"], out[key + "1"] = masks0[:, r], masks1[:, r]
    if dense:
        out["assignment"], out["reward"] = assignment, reward
    else:
        out["extra_positives"] = extra
    return out


def check_conf(name, conf):
    """The refusals the two sparse-map matchers share."""
    if conf.th_consistency is not None:
        raise NotImplementedError(f"{name}: th_consistency is not built (no configuration sets it)")
    for key in ("th_positive", "th_negative", "th_epi"):
        if conf[key] is not None and conf[key] < 0:
            raise ValueError(f"{name}: {key} must not be negative")
    if conf.save_fig_when_debug:
        logger.warning("%s: save_fig_when_debug is ignored, this package draws no figures", name)


class SparseDepthMatcher(BaseModel):
    default_conf = {
        "use_gt_pos": False,
        "th_positive": 3.0,
        "th_negative": 5.0,
        "th_epi": None,  # add some more epi outliers
        "th_consistency": None,  # check for projection consistency in px
        "save_fig_when_debug": False,
        # MI355X addition: False leaves `assignment` and `reward` ([B,M,N]) out, adds `extra_positives` [B]
        "dense_outputs": True,
    }

    required_data_keys = ["view0", "view1", "T_0to1", "keypoints0", "keypoints1", "sparse_depth0", "sparse_depth1",
                          "valid_3D_mask0", "valid_3D_mask1", "point3D_ids0", "point3D_ids1"]

    def _init(self, conf):
        check_conf("sparse_depth_matcher", conf)

    def _forward(self, data):
        seed = bool(self.conf.use_gt_pos)
        return gt_matches_from_sparse_map(
            data["keypoints0"], data["keypoints1"], data, data["sparse_depth0"], data["valid_depth_mask0"],
            data["sparse_depth1"], data["valid_depth_mask1"], data["point3D_ids0"] if seed else None,
            data["point3D_ids1"] if seed else None, data["valid_3D_mask0"] if seed else None,
            data["valid_3D_mask1"] if seed else None, pos_th=self.conf.th_positive, neg_th=self.conf.th_negative,
            epi_th=self.conf.th_epi, cc_th=self.conf.th_consistency, dense=bool(self.conf.dense_outputs))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = SparseDepthMatcher
