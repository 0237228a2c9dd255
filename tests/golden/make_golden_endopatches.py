"""Generate tests/golden/endopatches_homographies.npz by running the REFERENCE's own homography sampler
(gluefactory/geometry/homography.py: sample_homography_corners, compute_homography) under numpy's global generator,
which is what the reference's `fork_rng(seed)` seeds.

Runs only where a checkout of the reference exists (its path in GFC_REFERENCE); the tests read the committed .npz,
never the reference.  `omegaconf` comes from tests/golden/_standins; `kornia` and `cv2` (imported by the geometry
package, unused on this path) are empty modules put into sys.modules here.

    GFC_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_endopatches.py

Stored (data only):
  * EndoPatches geometry: image (582, 429) -- the vignette crop [81, 663, 55, 484] of a 720 x 540 frame --, patch
    (580, 426), max_angle 45, translation 1.0, n_angles 10; for every level in LEVELS and seed s in SEEDS, after
    np.random.seed(s): `H_<l>_<s>` (float64) and `corners_<l>_<s>` (the image's corners through H, float64);
    `H0to1_<l>_<s>`: compute_homography(coords0, coords1, [1, 1]).astype(float32) of the (level 0, level l) view pair
    drawn under the seeds 2 s and 2 s + 1, the corners cast to float32 first, as the dataset's `sample_homography` does;
  * one revisitop-style configuration (the dataset's defaults): image (1024, 768), patch (640, 480), max_angle 60,
    difficulty 0.8, translation 1.0: `rH_<s>`, `rcorners_<s>`.
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
for _name in ("kornia", "cv2"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)

from gluefactory.geometry.homography import compute_homography, sample_homography_corners  # noqa: E402

SIZE, PATCH = (582, 429), (580, 426)
LEVELS = (0.0, 0.3, 0.5, 0.7)
SEEDS = tuple(range(6))
ENDO = {"patch_shape": list(PATCH), "max_angle": 45, "translation": 1.0, "n_angles": 10, "min_convexity": 0.05}
RSIZE = (1024, 768)
REVISITOP = {"patch_shape": [640, 480], "max_angle": 60, "translation": 1.0, "n_angles": 10, "min_convexity": 0.05,
             "difficulty": 0.8}


def draw(seed, size, conf):
    np.random.seed(seed)
    H, _, coords, _ = sample_homography_corners(size, **conf)
    return H, coords


def main():
    out = {"size": np.array(SIZE), "patch": np.array(PATCH), "levels": np.array(LEVELS), "seeds": np.array(SEEDS),
           "rsize": np.array(RSIZE)}
    for li, level in enumerate(LEVELS):
        for s in SEEDS:
            H, coords = draw(s, SIZE, {**ENDO, "difficulty": level})
            out[f"H_{li}_{s}"], out[f"corners_{li}_{s}"] = H, coords
            _, c0 = draw(2 * s, SIZE, {**ENDO, "difficulty": 0.0})
            _, c1 = draw(2 * s + 1, SIZE, {**ENDO, "difficulty": level})
            out[f"H0to1_{li}_{s}"] = compute_homography(c0.astype(np.float32), c1.astype(np.float32), [1, 1]).astype(np.float32)
    for s in SEEDS:
        out[f"rH_{s}"], out[f"rcorners_{s}"] = draw(s, RSIZE, REVISITOP)
    path = os.path.join(HERE, "endopatches_homographies.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
