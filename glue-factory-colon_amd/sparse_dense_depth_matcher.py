"""Ground-truth matches from cached per-key-point depth -- counterpart of gluefactory/models/matchers/
sparse_dense_depth_matcher.py, the `ground_truth` component of py_cudasift+lightglue_endomapper_dense.yaml.

`gt_matches_from_pose_sparse_dense_map` (geometry/gt_generation.py:271-438): the order of decisions of the sparse-map
function without id seeding, on `depth_keypoints0/1` + `valid_depth_keypoints0/1`; a missing key raises the reference's
ValueError.  `use_gt_pos` and `use_gt_pos_for_plot` only select plots in the reference and do nothing here.  Same entry
(`gfc_gt_matches_sparse_map`), same twenty keys (`mask_pos_3d_map0/1` all False) and the same `dense_outputs` addition
as sparse_depth_matcher.
"""
from .base_model import BaseModel
from .sparse_depth_matcher import check_conf, gt_matches_from_sparse_map


class SparseDenseDepthMatcher(BaseModel):
    default_conf = {
        "use_gt_pos_for_plot": False,
        "use_gt_pos": False,  # legacy alias, plotting-only
        "th_positive": 3.0,
        "th_negative": 5.0,
        "th_epi": None,  # add some more epi outliers
        "th_consistency": None,  # check for projection consistency in px
        "save_fig_when_debug": False,
        # MI355X addition: False leaves `assignment` and `reward` ([B,M,N]) out, adds `extra_positives` [B]
        "dense_outputs": True,
    }

    def _init(self, conf):
        check_conf("sparse_dense_depth_matcher", conf)

    def _forward(self, data):
        if data.get("depth_keypoints0") is None or data.get("depth_keypoints1") is None:
            raise ValueError("Only working with cached features: missing depth_keypoints0/1 in cache output.")
        if data.get("valid_depth_keypoints0") is None or data.get("valid_depth_keypoints1") is None:
            raise ValueError("Only working with cached features: missing valid_depth_keypoints0/1 in cache output.")
        return gt_matches_from_sparse_map(
            data["keypoints0"], data["keypoints1"], data, data["depth_keypoints0"], data["valid_depth_keypoints0"],
            data["depth_keypoints1"], data["valid_depth_keypoints1"], pos_th=self.conf.th_positive,
            neg_th=self.conf.th_negative, epi_th=self.conf.th_epi, cc_th=self.conf.th_consistency,
            dense=bool(self.conf.dense_outputs))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = SparseDenseDepthMatcher
