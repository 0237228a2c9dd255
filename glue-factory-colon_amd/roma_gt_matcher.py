"""Ground-truth matches from RoMa's dense warps -- counterpart of gluefactory/models/matchers/roma_gt_matcher.py, the
`ground_truth` component of configs/train_endomapper_roma.yaml.

The reference runs the RoMa network inside this module and labels the key points with `gt_matches_from_roma`.  The
network (DINOv2 ViT-L plus a decoder) is NOT part of this package: its output keys are read from `data` -- `warp0/1`
[B,H,W,2] (normalised coordinates), `certainty0/1` [B,H,W] and optionally `cycle_error0/1` [B,H,W] --, which
`TwoViewPipeline` fills from `{**data, **pred}`.  Everything after the network runs through dense_warp.py
(csrc/gt_dense_warp.hip); the fields are cast to float32 on entry, as the reference's `custom_fwd(cast_inputs=float32)`
does to RoMa's half-precision output.  `keypoint_scores0/1 > 0` are the validity masks.
With `roma.add_cycle_error: true` and no `cycle_error0/1` in `data` the cycle error is computed at the four tap pixels
of every key point only (bit-equal to the dense fields sampled afterwards): no dense cycle field is allocated.
MI355X addition: `dense_outputs: False` omits `assignment` and `reward` and never allocates them.
`save_fig_when_debug` is accepted and ignored with one warning: this package draws nothing and writes no reports.
"""
import logging

from . import dense_warp
from .base_model import BaseModel

logger = logging.getLogger(__name__)
DENSE_KEYS = ("warp0", "warp1", "certainty0", "certainty1")


class RomaGTMatcher(BaseModel):
    default_conf = {
        "save_fig_when_debug": False,
        "th_positive": None,
        "th_negative": None,
        "roma": {
            "name": "matchers.roma",
            "weights": "indoor",
            "upsample_preds": True,
            "symmetric": True,
            "internal_hw": (560, 560),
            "output_hw": None,
            "sample": False,
            "mixed_precision": True,
            "add_cycle_error": False,
            "pos_cert_th": None,
            "pos_cycle_error_th": None,
            "neg_cert_th": None,
            "neg_cycle_error_th": None,
        },
        # MI355X addition: False leaves `assignment` and `reward` ([B,M,N]) out
        "dense_outputs": True,
    }
    required_data_keys = ["view0", "view1", "keypoints0", "keypoints1"]

    def _init(self, conf):
        if conf.save_fig_when_debug:
            logger.warning("roma_gt_matcher: save_fig_when_debug is ignored, this package draws no figures")

    def _forward(self, data):
        missing = [k for k in DENSE_KEYS if data.get(k) is None]
        if missing:
            raise NotImplementedError(
                "roma_gt_matcher: the RoMa network is not part of this package; supply its output in the data: warp0/1 "
                "[B,H,W,2] (normalised coordinates), certainty0/1 [B,H,W] and optionally cycle_error0/1 [B,H,W] "
                f"(missing: {', '.join(missing)})")
        valid0 = data.get("keypoint_scores0")
        valid1 = data.get("keypoint_scores1")
        if valid0 is None or valid1 is None:
            raise ValueError("RomaGTMatcher requires keypoint_scores0/1 to mask padded features.")
        roma = self.conf.roma
        f32 = lambda v: None if v is None else v.float()  # noqa: E731
        return dense_warp.gt_matches_from_roma(
            data["keypoints0"], data["keypoints1"], data, valid0=valid0 > 0, valid1=valid1 > 0,
            warp0=f32(data["warp0"]), warp1=f32(data["warp1"]), certainty0=f32(data["certainty0"]),
            certainty1=f32(data["certainty1"]), cycle_error0=f32(data.get("cycle_error0")),
            cycle_error1=f32(data.get("cycle_error1")), pos_th=self.conf.th_positive, neg_th=self.conf.th_negative,
            pos_cert_th=roma.pos_cert_th, pos_cycle_error_th=roma.pos_cycle_error_th, neg_cert_th=roma.neg_cert_th,
            neg_cycle_error_th=roma.neg_cycle_error_th, add_cycle_error=bool(roma.add_cycle_error),
            dense=bool(self.conf.dense_outputs))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = RomaGTMatcher
