"""Generate tests/golden/sparse_map.npz by running the REFERENCE's own sparse-map label functions on CPU.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_golden_hpatches.py, whose
empty `kornia` / `cv2` modules and `_standins` it shares by importing it); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sparse_map.py [--seed S]

What is called: gt_matches_from_pose_sparse_map and gt_matches_from_pose_sparse_dense_map (gluefactory/geometry/
gt_generation.py:441-591, 271-438), each on float32 inputs and on `.double()` inputs.

Cases `c<k>`: the three pairs of tests/golden/pose_depth.npz (PINHOLE, OPENCV, OPENCV_FISHEYE; 257 x 130 key points, the
depth per key point and its validity as stored there), then 65 x 1 and 1 x 65 cut from pair 0 around one correspondence.
Every seed moves the key points by up to 0.05 px (`jitter`); the depths per key point are inputs and stay.
Planted ids (`plant_ids`): ids on part of the true correspondences; a triple of duplicate ids in image 0 with a pair in
image 1; ids whose valid_3D is false; an id pair that contradicts the distance match; a seeded point without valid depth.
Settings `s<k>` = (pos_th, neg_th, epi_th, use_gt_pos): SETTINGS below; the last has pos_th > neg_th and separates
"negative overrides positive" from the fork's rule.  The sparse-dense function runs with the same thresholds (`d<k>`).
The script walks seeds until float32 and float64 agree on every integer, mask, `assignment` and `reward`, and
tests/sparse_map_reference.py flags NOTHING undecided.  `reward` is stored as int8, `assignment` with numpy.packbits.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden_hpatches as mh  # noqa: E402,F401  (sets up sys.modules / sys.path for the reference)

sys.path.insert(0, ROOT)
from gluefactory.geometry.gt_generation import (  # noqa: E402
    gt_matches_from_pose_sparse_dense_map,
    gt_matches_from_pose_sparse_map,
)
from gluefactory.geometry.wrappers import Camera, Pose  # noqa: E402

import sparse_map_reference as sr  # noqa: E402

torch.set_grad_enabled(False)
SETTINGS = ((3.0, 5.0, None, False), (None, 10.0, None, True), (3.0, 5.0, 5.0, True), (None, None, None, True),
            (6.0, 5.0, None, True))
INT_KEYS = ("matches0", "matches1", "visible0", "visible1") + tuple(k + s for k in sr.MASK_KEYS for s in "01")


def ref_camera(data, model, dtype):
    cam = Camera(data.to(dtype) if model != "PINHOLE" else data[..., :6].to(dtype))
    cam.model = model
    return cam


def geometry_cases():
    """kp0, kp1, depth per key point, valid depth, cameras, pose, model and the true matches of every case."""
    fx = np.load(os.path.join(HERE, "pose_depth.npz"))
    t = lambda k, c: torch.from_numpy(fx[k][c])  # noqa: E731
    cases = []
    for c, model in enumerate(fx["models"]):
        cases.append({"kp0": t("kp0", c), "kp1": t("kp1", c), "d0": t("depth_kp0", c), "d1": t("depth_kp1", c),
                      "valid0": t("valid0", c), "valid1": t("valid1", c), "cam0": t("cam0", c), "cam1": t("cam1", c),
                      "T": t("T_0to1", c), "model": str(model), "gt0": t("gt_matches0", c)})
    full = cases[0]
    rows = torch.nonzero(full["gt0"][:65] > -1).flatten()
    i = int(rows[0])
    j = int(full["gt0"][i])
    cut = lambda r0, r1: {**full, **{k: full[k][r0] for k in ("kp0", "d0", "valid0")},  # noqa: E731
                          **{k: full[k][r1] for k in ("kp1", "d1", "valid1")}}
    a = cut(slice(0, 65), slice(j, j + 1))
    a["gt0"] = torch.where(full["gt0"][:65] == j, 0, -1)
    lo = max(0, min(j - 30, full["kp1"].shape[0] - 65))
    b = cut(slice(i, i + 1), slice(lo, lo + 65))
    b["gt0"] = torch.tensor([j - lo])
    return cases + [a, b]


def jitter(case, seed):
    """The key points moved by up to 0.05 px (their depth and its validity are inputs of these functions and stay): what
    a new seed changes about the geometry, so that walking seeds can leave every threshold."""
    g = torch.Generator().manual_seed(seed + 17)
    return {**case, "kp0": case["kp0"] + 0.1 * (torch.rand(case["kp0"].shape, generator=g) - 0.5),
            "kp1": case["kp1"] + 0.1 * (torch.rand(case["kp1"].shape, generator=g) - 0.5)}


def plant_ids(case, seed):
    g = torch.Generator().manual_seed(seed)
    m, n = case["kp0"].shape[0], case["kp1"].shape[0]
    ids0, ids1 = torch.arange(m) + 1_000_000, torch.arange(n) + 2_000_000
    v3d0, v3d1 = torch.rand(m, generator=g) > 0.1, torch.rand(n, generator=g) > 0.1
    rows = torch.nonzero(case["gt0"] > -1).flatten()
    keep = rows[torch.rand(rows.shape[0], generator=g) > 0.4]
    ids1[case["gt0"][keep]] = ids0[keep]  # ids on true correspondences (some with valid_3D false)
    if m >= 65 and n >= 65:
        free0 = torch.nonzero(case["gt0"] == -1).flatten()
        pick0 = free0[torch.randperm(free0.shape[0], generator=g)[:4]]
        cols = torch.randperm(n, generator=g)[:3]
        ids0[pick0[:3]], ids1[cols[:2]] = 77, 77        # a triple in image 0, a pair in image 1
        v3d0[pick0[:3]], v3d1[cols[:2]] = True, True
        contra = keep[0]                                 # an id pair that contradicts the distance match
        other = int((case["gt0"][contra] + 1 + int(torch.randint(n - 1, (1,), generator=g))) % n)
        ids0[contra] = 88
        ids1[other] = 88
        v3d0[contra], v3d1[other] = True, True
        nodepth = torch.nonzero(~case["valid0"]).flatten()  # a seeded point without valid depth
        if nodepth.numel():
            ids0[nodepth[0]] = ids1[cols[2]]
            v3d0[nodepth[0]], v3d1[cols[2]] = True, True
    return ids0, ids1, v3d0, v3d1


def run(case, ids, setting, dtype, dense_fn):
    pos, neg, epi, use = setting
    f = lambda v: v[None].to(dtype)  # noqa: E731
    data = {"view0": {"camera": ref_camera(case["cam0"][None], case["model"], dtype)},
            "view1": {"camera": ref_camera(case["cam1"][None], case["model"], dtype)}, "T_0to1": Pose(f(case["T"]))}
    if dense_fn:
        r = gt_matches_from_pose_sparse_dense_map(
            f(case["kp0"]), f(case["kp1"]), data, pos_th=pos, neg_th=neg, epi_th=epi, depth_keypoints0=f(case["d0"]),
            depth_keypoints1=f(case["d1"]), valid_depth_keypoints0=case["valid0"][None],
            valid_depth_keypoints1=case["valid1"][None])
    else:
        ids0, ids1, v3d0, v3d1 = ids
        r = gt_matches_from_pose_sparse_map(
            f(case["kp0"]), f(case["kp1"]), data, pos_th=pos, neg_th=neg, epi_th=epi, use_gt_pos=use,
            sparse_depth0=f(case["d0"]), sparse_depth1=f(case["d1"]), valid_depth_mask0=case["valid0"][None],
            valid_depth_mask1=case["valid1"][None], point3D_ids0=ids0[None], point3D_ids1=ids1[None],
            valid_3D_mask0=v3d0[None], valid_3D_mask1=v3d1[None])
    assert len(r) == 20
    return {k: v[0] for k, v in r.items()}


def fundamental64(case):
    from gluefactory.geometry.epipolar import T_to_E

    cam0 = ref_camera(case["cam0"][None], case["model"], torch.float64)
    cam1 = ref_camera(case["cam1"][None], case["model"], torch.float64)
    return (cam1.calibration_matrix().inverse().transpose(-1, -2) @ T_to_E(Pose(case["T"][None].double()))
            @ cam0.calibration_matrix().inverse())[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    out = {"settings": np.array([[-1.0 if v is None else float(v) for v in s] for s in SETTINGS])}
    for c, geometry in enumerate(geometry_cases()):
        seed = args.seed
        while True:
            ids = plant_ids(geometry, seed * 100 + c)
            case = jitter(geometry, seed * 100 + c)
            ok, results = True, {}
            for s, setting in enumerate(SETTINGS):
                for dense_fn in (False, True):
                    r64 = run(case, ids, setting, torch.float64, dense_fn)
                    use = setting[3] and not dense_fn
                    chk = sr.sparse_map_labels(
                        case["kp0"].double(), case["kp1"].double(), r64["proj_0to1"], r64["proj_1to0"], r64["visible0"],
                        r64["visible1"], case["valid0"], case["valid1"], *(ids if use else (None,) * 4),
                        F=fundamental64(case), pos_th=setting[0], neg_th=setting[1], epi_th=setting[2])
                    und = int(chk["undecided0"].sum()) + int(chk["undecided1"].sum()) + int(chk["undecided_dense"].sum())
                    if und:  # the next seed: no need for the rest
                        ok = False
                        break
                    r32 = run(case, ids, setting, torch.float32, dense_fn)
                    same = all(torch.equal(r32[k], r64[k]) for k in INT_KEYS + ("assignment",)) and \
                        torch.equal(r32["reward"].double(), r64["reward"])
                    agree = all(torch.equal(chk[k], r64[k]) for k in ("matches0", "matches1", "assignment")) and \
                        torch.equal(chk["reward"], r64["reward"])
                    g0 = r32["matches0"]
                    print(f"c{c} seed {seed} {'d' if dense_fn else 's'}{s}: same {same}, undecided {und}, restatement "
                          f"agrees {agree}, matches0 match/unmatched/ignore {int((g0 > -1).sum())}/"
                          f"{int((g0 == -1).sum())}/{int((g0 == -2).sum())}, assignment {int(r32['assignment'].sum())}, "
                          f"extra {chk['extra_positives']} = {chk['extra_positives_dense']}", flush=True)
                    assert agree, "the restatement differs from the reference"
                    ok = ok and same
                    results[("d" if dense_fn else "s") + str(s)] = (r32, r64)
                if not ok:
                    break
            if ok:
                break
            seed += 1
        pre = f"c{c}_"
        out[pre + "seed"] = np.int64(seed)
        out[pre + "model"] = np.array(case["model"])
        for k in ("kp0", "kp1", "d0", "d1", "valid0", "valid1", "cam0", "cam1", "T"):
            out[pre + k] = case[k].numpy()
        for k, v in zip(("ids0", "ids1", "v3d0", "v3d1"), ids):
            out[pre + k] = v.numpy()
        out[pre + "F_f64"] = fundamental64(case).numpy()
        for tag, (r32, r64) in results.items():
            for k in INT_KEYS:
                out[f"{pre}{tag}_{k}"] = r32[k].numpy()
            out[f"{pre}{tag}_assignment"] = np.packbits(r32["assignment"].numpy())
            out[f"{pre}{tag}_reward"] = r32["reward"].numpy().astype(np.int8)
            if tag == "s0":
                out[pre + "proj_0to1_f64"], out[pre + "proj_1to0_f64"] = r64["proj_0to1"].numpy(), r64["proj_1to0"].numpy()
    path = os.path.join(HERE, "sparse_map.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
