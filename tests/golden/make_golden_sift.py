"""Generate tests/golden/sift_post.npz by running the REFERENCE's own SIFT post-processing functions
(gluefactory/models/extractors/sift.py: filter_dog_point, sift_to_rootsift; extractors/utils.py:
filter_keypoints_by_specular_mask; the top-k and pad_to_length branch of extract_single_image, restated here call for
call with the reference's own torch.topk / pad_to_length) on planted inputs.

Runs only where a checkout of the reference exists (its path in GFC_REFERENCE); the tests read the committed .npz,
never the reference.  `cv2`, `kornia.color`, `pycolmap` and `packaging` (imported by sift.py, untouched by the called
functions) are empty modules put into sys.modules here; `omegaconf` comes from tests/golden/_standins.

    GFC_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sift.py

Planted (data only, one image of 24 x 32, all float32 as the reference's backends deliver):
  * three points rounding to pixel (5, 7) with distinct scores; two at (9, 20) with equal scores and distinct |angle|;
    two at (9, 21) with equal score and angles +a / -a (both survive); a cluster within 3 pixels around (15, 10) with
    distinct scores (nms_radius 3 keeps one, 0 keeps all); isolated points; points on and across the edge of the
    specular mask (a rectangle of False) and on the image border;
  * 40 descriptors (non-negative, some all-zero rows) for sift_to_rootsift;
  * top-k with k = 12 of the points kept at nms_radius 0, by score and by score x scale: no tie at the boundary;
    pad_to_length of scales / oris / scores / descriptors / valid mask to 48.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GFC_REFERENCE")
if not REF:
    raise SystemExit("set GFC_REFERENCE to a checkout of the reference")
sys.dont_write_bytecode = True
for _name in ("cv2", "kornia", "kornia.color", "pycolmap", "packaging", "packaging.version"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["kornia.color"].rgb_to_grayscale = None  # a name to import, never called
sys.modules["cv2"].Feature2D = None  # a name in an annotation
sys.modules["kornia"].color = sys.modules["kornia.color"]
sys.modules["packaging"].version = sys.modules["packaging.version"]
sys.modules["pycolmap"].__version__ = "0"
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)

import torch  # noqa: E402
from gluefactory.models.extractors.sift import filter_dog_point, sift_to_rootsift  # noqa: E402
from gluefactory.models.extractors.utils import filter_keypoints_by_specular_mask  # noqa: E402
from gluefactory.models.utils.misc import pad_to_length  # noqa: E402

H, W, K, PAD = 24, 32, 12, 48


def planted():
    g = np.random.RandomState(0)
    pts, sc, scale, ang = [], [], [], []

    def add(x, y, s, sig, a):
        pts.append([x, y]); sc.append(s); scale.append(sig); ang.append(a)

    add(7.3, 5.4, 0.030, 1.8, 0.4); add(7.6, 5.7, 0.050, 2.2, -1.0); add(7.45, 5.2, 0.041, 3.0, 2.0)  # pixel (5, 7)
    add(20.5, 9.5, 0.033, 2.0, 1.2); add(20.6, 9.3, 0.033, 2.0, -0.3)  # equal scores, distinct |angle|
    add(21.5, 9.5, 0.027, 2.0, 0.9); add(21.4, 9.6, 0.027, 2.0, -0.9)  # equal scores, equal |angle|
    for dx, dy, s in ((0, 0, 0.060), (2, 1, 0.052), (-1, 2, 0.047), (3, -2, 0.071), (-3, 3, 0.0405)):  # NMS cluster
        add(10.5 + dx, 15.5 + dy, s, 1.7 + 0.1 * dx, 0.1 * dy + 0.05)
    for x, y in ((25.5, 3.5), (26.0, 4.0), (26.49, 4.49), (24.9, 3.2), (28.5, 8.5), (27.51, 6.5), (29.5, 2.5)):  # mask edge
        add(x, y, 0.02 + 0.001 * len(pts), 2.5, 0.3)
    add(0.5, 0.5, 0.045, 1.6, 0.0); add(31.4, 23.4, 0.046, 1.6, 3.1); add(31.5, 12.5, 0.039, 1.6, -3.1)  # borders
    while len(pts) < 40:  # isolated points on distinct pixels, distinct scores
        x, y = g.randint(1, W - 1), g.randint(12, H - 1)
        if any(abs(x - int(p[0])) < 1 and abs(y - int(p[1])) < 1 for p in pts):
            continue
        add(x + g.uniform(0.1, 0.9), y + g.uniform(0.1, 0.9), 0.01 + 0.0007 * len(pts) + g.uniform(0, 0.0003),
            g.uniform(1.6, 6.0), g.uniform(-3.1, 3.1))
    mask = np.ones((H, W), bool)
    mask[2:6, 26:29] = False
    desc = np.abs(g.randn(40, 128)).astype(np.float32) * (g.rand(40, 128) > 0.4)
    desc[3] = 0
    desc[17] = 0
    return (np.array(pts, np.float32), np.array(sc, np.float32), np.array(scale, np.float32), np.array(ang, np.float32),
            mask, desc.astype(np.float32))


def main():
    pts, sc, scale, ang, mask, desc = planted()
    out = dict(points=pts, scores=sc, scales=scale, angles=ang, mask=mask, desc=desc, shape=np.array([H, W]),
               k=np.array(K), pad=np.array(PAD))
    for r in (0, 3):
        out[f"keep_r{r}"] = np.sort(filter_dog_point(pts, scale, ang, (H, W), r, sc))
        out[f"keep_r{r}_noscores"] = np.sort(filter_dog_point(pts, scale, ang, (H, W), r, None))
    out["rootsift"] = sift_to_rootsift(torch.from_numpy(desc.copy())).numpy()
    t = [torch.from_numpy(a) for a in (pts, scale, ang, desc, sc)]
    kept = filter_keypoints_by_specular_mask(t[0], torch.from_numpy(mask)[None], *t[1:], keypoint_offset=0.5)
    out["specular_points"] = kept[0].numpy()
    out["specular_keep"] = np.array([i for i, p in enumerate(pts) if any((p == q).all() for q in kept[0].numpy())])
    # the top-k branch of extract_single_image (sift.py:362-380) on the points kept at nms_radius 0
    keep = out["keep_r0"]
    ksc, kscale = torch.from_numpy(sc[keep]), torch.from_numpy(scale[keep])
    out["topk_score"] = keep[np.sort(torch.topk(ksc, K).indices.numpy())]
    out["topk_score_order"] = keep[torch.topk(ksc, K).indices.numpy()]
    out["topk_score_scale"] = keep[np.sort(torch.topk(ksc * kscale, K).indices.numpy())]
    sel = out["topk_score_order"]
    out["padded_scales"] = pad_to_length(torch.from_numpy(scale[sel]), PAD, -1, mode="zeros").numpy()
    out["padded_oris"] = pad_to_length(torch.from_numpy(ang[sel]), PAD, -1, mode="zeros").numpy()
    out["padded_scores"] = pad_to_length(torch.from_numpy(sc[sel]), PAD, -1, mode="zeros").numpy()
    out["padded_desc"] = pad_to_length(torch.from_numpy(desc[sel]), PAD, -2, mode="zeros").numpy()
    out["padded_valid"] = pad_to_length(torch.ones(K, dtype=torch.bool), PAD, -1, mode="zeros").numpy()
    out["padded_rootsift"] = sift_to_rootsift(torch.from_numpy(out["padded_desc"].copy())).numpy()
    np.savez_compressed(os.path.join(HERE, "sift_post.npz"), **out)
    for k_, v in out.items():
        print(k_, v.shape, v.dtype)


if __name__ == "__main__":
    main()
