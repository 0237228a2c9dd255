"""The GPU five-point RANSAC relative-pose estimator behind the reference's estimator contract
(gluefactory/robust_estimators/base_estimator.py, relative_pose/opencv.py): configured with a dict, called with the
matched points and the two cameras, returns {"success", "M_0to1", "inliers"}.  The arithmetic is
`gfc_eval_relative_pose_ransac` (csrc/relpose.hip) through `eval_utils.relative_pose_ransac`; there is no CPU
implementation."""
import torch

from . import _native as nat
from . import eval_utils, geometry
from .base_model import Conf, merge


class GpuRelativePoseEstimator:
    base_default_conf = {"name": "gfc_amd"}
    default_conf = {"ransac_th": 1.0, "options": {"num_hypotheses": 2048, "lo_iters": 3, "seed": 0}}
    required_data_keys = ["m_kpts0", "m_kpts1", "camera0", "camera1"]

    def __init__(self, conf=None):
        self.conf = Conf(merge(merge(self.base_default_conf, self.default_conf), conf or {}))
        self.required_data_keys = list(self.required_data_keys)
        unknown = set(self.conf.options) - {"num_hypotheses", "lo_iters", "seed", "stream_id"}
        if unknown:
            raise ValueError(f"unknown options {sorted(unknown)}: the estimator takes num_hypotheses, lo_iters, seed, stream_id")

    def __call__(self, data):
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        pts0, pts1 = data["m_kpts0"], data["m_kpts1"]
        nat.require_cuda(pts0, "m_kpts0")
        nat.require_cuda(pts1, "m_kpts1")
        assert pts0.ndim == 2 and pts0.shape == pts1.shape, "m_kpts0 / m_kpts1: [n, 2] matched points of one pair"
        n = pts0.shape[0]
        m0 = torch.arange(n, device=pts0.device)[None]
        opt = self.conf.options
        res = eval_utils.relative_pose_ransac(pts0[None], pts1[None], m0, data["camera0"], data["camera1"],
                                              float(self.conf.ransac_th), num_hypotheses=opt.get("num_hypotheses", 2048),
                                              lo_iters=opt.get("lo_iters", 3), seed=opt.get("seed", 0),
                                              stream_id=opt.get("stream_id", 0))
        # float64, as computed: the pose error is an fp64 expression of it
        return {"success": bool(res["success"][0, 0]), "M_0to1": geometry.Pose.from_Rt(res["R"][0, 0], res["t"][0, 0]),
                "inliers": res["inliers"][0, 0]}
