"""Measured distances between the SIFT kernels and the float64 restatement (tests/sift_reference.py), on the fixtures of
tests/test_gpu_sift.py.  UNPINNED against OpenCV, pycolmap and CudaSift: none of them is available.

    python tools/sift_parity.py --out DIR

Writes DIR/sift_parity.json: per stage the figure the test bounds, the bound or allowance, the excused count (counted
in the run: key points whose number of orientations differs), and how the allowance is set -- orientation and
descriptor allowances are 4 x the distance between the restatement run in float32 and in float64.  The comparisons are
those of tests/sift_gpu_cases.py, which the tests assert on.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sift_gpu_cases as gc  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import sift  # noqa: E402


def pyramid_figures():
    out = []
    for case, (h, w, valid) in gc.PYRAMID_CASES.items():
        for fo in (-1, 0):
            imgs = np.stack([gc.image(h, w, 5 + i) for i in range(len(valid))])
            worst_g, worst_d, _ = gc.pyramid_errors(sift, imgs, valid, fo, 3)
            out.append({"case": case, "first_octave": fo, "worst_gauss_error_over_bound": float(worst_g),
                        "worst_dog_error_over_bound": float(worst_d)})
    return out


def stage_figures():
    fig = gc.stage_fixture_figures(sift)
    fig.pop("_ori")
    return fig


def whole_figures():
    return gc.whole_extractor_figures(sift)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sift_parity needs the GPU")
    res = {"what": "SIFT kernels against the float64 restatement of tests/sift_reference.py; UNPINNED against OpenCV, "
                   "pycolmap and CudaSift (absent)",
           "device": torch.cuda.get_device_name(0), "library": nat.lib().gfc_version().decode(),
           "pyramid": pyramid_figures(), "orientation_and_descriptor": stage_figures(), "whole_extractor": whole_figures()}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "sift_parity.json"), "w") as f:
        json.dump(res, f, indent=1, default=float)
    print(json.dumps(res["orientation_and_descriptor"], default=float))
    print(json.dumps(res["whole_extractor"], default=float))


if __name__ == "__main__":
    main()
