"""The GPU RANSAC homography estimator behind the reference's estimator contract
(gluefactory/robust_estimators/base_estimator.py, homography/poselib.py): configured with a dict, called with the
matched points, returns {"success", "M_0to1", "inliers"}.  The arithmetic is `gfc_eval_homography_ransac`
(csrc/ransac.hip) through `eval_utils.homography_ransac`; there is no CPU implementation."""
import torch

from . import _native as nat
from . import eval_utils
from .base_model import Conf, merge


class GpuHomographyEstimator:
    base_default_conf = {"name": "gfc_amd"}
    default_conf = {"ransac_th": 2.0, "options": {"num_hypotheses": 2048, "lo_iters": 3, "seed": 0}}
    required_data_keys = ["m_kpts0", "m_kpts1"]

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
        res = eval_utils.homography_ransac(None, pts0[None], pts1[None], m0, None, float(self.conf.ransac_th),
                                           num_hypotheses=opt.get("num_hypotheses", 2048),
                                           lo_iters=opt.get("lo_iters", 3), seed=opt.get("seed", 0),
                                           stream_id=opt.get("stream_id", 0))
        return {"success": bool(res["success"][0, 0]), "M_0to1": res["H"][0, 0].to(pts0.dtype),
                "inliers": res["inliers"][0, 0]}
