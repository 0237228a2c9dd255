"""Generate tests/golden/pose_depth.npz by running the REFERENCE's own pose / depth evaluation code.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_golden.py); the tests
read the committed .npz, never the reference.  The reference's geometry package imports `kornia` and `cv2` at module
level without using them on this path: two EMPTY modules of those names are put into sys.modules right here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pose.py [--seed S]

Three pairs (PINHOLE, OPENCV with four coefficients, OPENCV_FISHEYE) of synthetic.posed_plane_pairs with 96 x 128 depth
maps, M = 257 and N = 130 key points, plus planted special points (see `plant`).  Outputs are what the reference's
symmetric_reprojection_error, gt_matches_from_pose_depth, generalized_epi_dist, relative_pose_error and
Camera.cam2image / image2cam give in float32, and the same on `.double()` inputs (suffix _f64).  The script walks seeds
from --seed until tests/pose_reference.undecidable_counts finds no reference value within a rounding error of a
decision (threshold, argmin, image bound, depth sign, sampling cell), so that the GPU comparison needs no excuses.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GFC_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for _name in ("kornia", "cv2"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gluefactory.geometry.depth import project, sample_depth, symmetric_reprojection_error  # noqa: E402
from gluefactory.geometry.epipolar import generalized_epi_dist, relative_pose_error  # noqa: E402
from gluefactory.geometry.gt_generation import gt_matches_from_pose_depth  # noqa: E402
from gluefactory.geometry.wrappers import Camera, Pose  # noqa: E402

import pose_reference as pr  # noqa: E402
from glue_factory_colon_amd import synthetic  # noqa: E402

torch.set_grad_enabled(False)
H, W, M, N = 96, 128, 257, 130
CASES = (("PINHOLE", None), ("OPENCV", (-0.5, 0.1, 0.002, -0.001)), ("OPENCV_FISHEYE", None))
N_SPECIAL0 = 14  # rows of kp0 the planted special points take (the last unmatched ones)


def ref_camera(data, model, dtype):
    cam = Camera(data.to(dtype) if model != "PINHOLE" else data[..., :6].to(dtype))
    cam.model = model
    return cam


def ref_project(kp, depth_i, cam_i, cam_j, T):
    d, valid = sample_depth(kp, depth_i)
    proj, visible = project(kp, d, None, cam_i, cam_j, T, valid, ccth=None)
    return d, valid, proj, visible


def plant(rng, item, pred, model):
    """Overwrite the last unmatched key points of view 0 (and two of view 1) with the special cases of the fixture."""
    cam0d, cam1d = item["view0"]["camera"]._data, item["view1"]["camera"]._data
    depth0 = item["view0"]["depth"].clone()
    kp0, kp1, m0 = pred["keypoints0"].clone(), pred["keypoints1"].clone(), pred["matches0"].clone()
    T = item["T_0to1"]._data[0].double()
    R, t = T[:9].reshape(3, 3), T[9:]
    rows = list(range(M - N_SPECIAL0, M))
    m0[rows] = -1
    hole = (depth0[0] <= 0).numpy()
    ys, xs = np.nonzero(hole)
    # 1-4: inside a hole (centre of a hole pixel with hole neighbours), and next to one: 0.7 px outside its left edge
    # (the bilinear footprint touches the hole, the nearest pixel is valid) and 0.3 px inside (nearest is a hole)
    inner = [(y, x) for y, x in zip(ys, xs) if 1 <= y < H - 1 and 1 <= x < W - 1 and hole[y - 1:y + 2, x - 1:x + 2].all()]
    y, x = inner[len(inner) // 2]
    kp0[rows[0]] = torch.tensor([x + 0.3, y + 0.6])
    edge = [(y, x) for y, x in zip(ys, xs) if 2 <= x and 1 <= y < H - 1 and not hole[y - 1:y + 2, x - 2:x].any()
            and hole[y - 1:y + 2, x].all()]
    y, x = edge[len(edge) // 3]
    kp0[rows[1]] = torch.tensor([x - 0.2, y + 0.3])   # 0.2 px left of the hole's first column: nearest pixel valid
    kp0[rows[2]] = torch.tensor([x + 0.3, y + 0.7])   # inside the first hole column: nearest pixel is the hole
    kp0[rows[3]] = torch.tensor([x - 0.7, y + 0.2])   # footprint x-2 / x-1: clear of the hole
    # 5-8: on the image border, over valid depth
    free = [yy for yy in range(4, H - 4) if not hole[yy - 1:yy + 2, :2].any() and not hole[yy - 1:yy + 2, -2:].any()]
    kp0[rows[4]] = torch.tensor([0.0, free[0] + 0.3])
    kp0[rows[5]] = torch.tensor([W - 1.0, free[len(free) // 2] + 0.7])
    kp1[N - 1] = torch.tensor([0.0, free[-1] + 0.3])
    kp1[N - 2] = torch.tensor([W - 1.0, free[1] + 0.7])
    # 9-10: a 3 x 3 patch of small depth puts a point behind camera 1 / beyond the radial validity limit of camera 1
    clear = [(yy, xx) for yy in range(6, H - 6, 5) for xx in range(6, W - 6, 5) if not hole[yy - 3:yy + 4, xx - 3:xx + 4].any()]

    def patch_point(target_row, depth_value, k):
        yy, xx = clear[k]
        depth0[0, yy - 1:yy + 2, xx - 1:xx + 2] = depth_value
        kp0[target_row] = torch.tensor([xx + 0.3, yy + 0.3])

    tz = float(t[2])
    patch_point(rows[6], max(0.4 * -tz, 1e-3) if tz < 0 else 1e-3, len(clear) // 2)  # Z = z + tz < 0
    if model == "OPENCV":  # r^2 a little beyond the limit 2.0 of (k1, k2) = (-0.5, 0.1): lands INSIDE the image
        yy, xx = clear[len(clear) // 3]
        ray = torch.tensor([(xx + 0.3 - float(cam0d[0, 4])) / float(cam0d[0, 2]),
                            (yy + 0.3 - float(cam0d[0, 5])) / float(cam0d[0, 3]), 1.0], dtype=torch.float64)
        best = None
        for z in np.linspace(0.02, 1.0, 4000):
            P = R @ (ray * z) + t
            r2 = float((P[0] / P[2]) ** 2 + (P[1] / P[2]) ** 2) if P[2] > 1e-3 else 0.0
            if 2.1 < r2 < 2.4:
                best = z
                break
        assert best is not None, "no depth puts the point beyond the validity limit"
        patch_point(rows[7], float(best), len(clear) // 3)
    # 11: a point whose projection falls between size - 1 and size of view 1 (inside by `< size`, outside by `<= size - 1`)
    cand = torch.stack(torch.meshgrid(torch.arange(0.3, W - 0.2, 0.37), torch.arange(0.3, H - 0.2, 0.61), indexing="xy"), -1).reshape(-1, 2)
    cam0, cam1 = ref_camera(cam0d, model, torch.float32), ref_camera(cam1d, model, torch.float32)
    _, cvalid, cproj, _ = ref_project(cand[None], depth0, cam0, cam1, Pose(item["T_0to1"]._data))
    sel = cvalid[0] & (((cproj[0, :, 0] > W - 0.9) & (cproj[0, :, 0] < W - 0.1) & (cproj[0, :, 1] > 1) & (cproj[0, :, 1] < H - 2))
                       | ((cproj[0, :, 1] > H - 0.9) & (cproj[0, :, 1] < H - 0.1) & (cproj[0, :, 0] > 1) & (cproj[0, :, 0] < W - 2)))
    assert sel.any(), "no candidate projects into the last pixel row / column"
    kp0[rows[8]] = cand[sel.nonzero()[0, 0]]
    # 12-13: exact duplicates: key point N - 3 of view 1 repeats the partner of planted point 4 (a tie in row 4), key
    # point rows[9] of view 0 repeats planted point 8 (a tie in the column of its partner): the first index must win
    # (4 and 8 stand for the first two planted points that the reference itself matches to their partners)
    pre = gt_matches_from_pose_depth(kp0[None], kp1[None], {"view0": {"camera": cam0, "depth": depth0},
                                                           "view1": {"camera": cam1, "depth": item["view1"]["depth"]},
                                                           "T_0to1": Pose(item["T_0to1"]._data)}, pos_th=3.0, neg_th=5.0)
    good = [i for i in range(M - N_SPECIAL0) if m0[i] > -1 and m0[i] < N - 3 and pre["matches0"][0, i] == m0[i]]
    assert len(good) >= 2, "fewer than two planted matches are ground-truth matches"
    i_row, i_col = good[0], good[1]
    kp1[N - 3] = kp1[m0[i_row]]
    kp0[rows[9]] = kp0[i_col]
    item["view0"]["depth"] = depth0
    # matches pointing at the overwritten points of view 1 are dropped; the special points stay unmatched except two
    for j in (N - 1, N - 2, N - 3):
        m0[m0 == j] = -1
    used = set(m0[m0 > -1].tolist())
    for r_, j in ((rows[1], N - 1), (rows[2], N - 2)):  # hole-adjacent points take part in the reprojection metric
        if j not in used:
            m0[r_] = j
    pred.update(keypoints0=kp0, keypoints1=kp1, matches0=m0)
    return {"dup_row": i_row, "dup_col": int(m0[i_col]), "dup_kp0": (i_col, rows[9]), "dup_kp1": (int(m0[i_row]), N - 3)}


def evaluate(item, pred, model, dtype):
    """Everything the fixture stores for one pair, from the reference's functions in `dtype`."""
    cam0 = ref_camera(item["view0"]["camera"]._data, model, dtype)
    cam1 = ref_camera(item["view1"]["camera"]._data, model, dtype)
    T = Pose(item["T_0to1"]._data.to(dtype))
    d0, d1 = item["view0"]["depth"].to(dtype), item["view1"]["depth"].to(dtype)
    kp0, kp1, m0 = pred["keypoints0"][None].to(dtype), pred["keypoints1"][None].to(dtype), pred["matches0"]
    data = {"view0": {"camera": cam0, "depth": d0}, "view1": {"camera": cam1, "depth": d1}, "T_0to1": T}
    gt = gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3.0, neg_th=5.0)
    _, valid0 = sample_depth(kp0, d0)
    _, valid1 = sample_depth(kp1, d1)
    sel = m0 > -1
    pts0, pts1 = kp0[0][sel], kp1[0][m0[sel]]
    err, valid = symmetric_reprojection_error(pts0[None], pts1[None], cam0, cam1, T, d0, d1)
    err, valid = err[0], valid[0]
    e = err[valid].nan_to_num(nan=float("inf"))
    gm = gt["matches0"]
    mask_r = (gm > -1).float()
    mask_p = ((m0[None] > -1) & (gm >= -1)).float()
    metrics7 = [(e < 1).float().mean().nan_to_num().item(), (e < 3).float().mean().nan_to_num().item(),
                (e < 5).float().mean().nan_to_num().item(), valid.float().sum().item(),
                valid.float().mean().nan_to_num().item() * 100.0,
                (((m0[None] == gm) * mask_r).sum(1) / (1e-8 + mask_r.sum(1)))[0].item(),
                (((m0[None] == gm) * mask_p).sum(1) / (1e-8 + mask_p.sum(1)))[0].item()]
    epi = generalized_epi_dist(pts0[None], pts1[None], cam0, cam1, T, False, essential=True)[0]
    metrics5 = [(epi < 1e-4).float().mean().nan_to_num().item(), (epi < 5e-4).float().mean().nan_to_num().item(),
                (epi < 1e-3).float().mean().nan_to_num().item(), float(pts0.shape[0]), (M + N) / 2.0]
    # the camera functions on their own: all key points through image2cam, their 3-D points through cam2image
    ray0 = cam0.image2cam(kp0)
    p3d = T.transform(ray0 * gt["depth_keypoints0"][..., None].nan_to_num(nan=1.0))
    c2i, c2i_valid = cam1.cam2image(p3d)
    p3d_back = T.inv().transform(cam1.image2cam(kp1) * gt["depth_keypoints1"][..., None].nan_to_num(nan=1.0))
    pad = torch.full((M,), float("nan"), dtype=dtype)
    err_pad, epi_pad = pad.clone(), pad.clone()
    err_pad[: len(err)], epi_pad[: len(epi)] = err, epi
    valid_pad = torch.zeros(M, dtype=torch.bool)
    valid_pad[: len(valid)] = valid
    return {"depth_kp0": gt["depth_keypoints0"][0], "depth_kp1": gt["depth_keypoints1"][0], "valid0": valid0[0],
            "valid1": valid1[0], "proj_0to1": gt["proj_0to1"][0], "proj_1to0": gt["proj_1to0"][0],
            "visible0": gt["visible0"][0], "visible1": gt["visible1"][0], "gt_matches0": gt["matches0"][0],
            "gt_matches1": gt["matches1"][0], "reproj_err": err_pad, "reproj_valid": valid_pad, "epi_err": epi_pad,
            "metrics7": torch.tensor(metrics7, dtype=torch.float64), "metrics5": torch.tensor(metrics5, dtype=torch.float64),
            "ray0": ray0[0], "p3d_1": p3d[0], "p3d_0": p3d_back[0], "c2i": c2i[0], "c2i_valid": c2i_valid[0], "T_1to0": T.inv()._data[0]}


def pose_error_cases(rng, T_gt):
    """A few estimated poses per pair and the reference's relative_pose_error of each, in float32 as the evaluation
    runs it.  Both angles of every case are kept above 3 degrees: the reference forms them as acos(c) in float32,
    whose error is ulp(1) / sin(angle) = 6e-8 / sin(angle); below 3 degrees that alone exceeds the 1e-4 degrees the
    tests compare to (at 0.7 degrees the reference's float32 and float64 results differ by 2.4e-4 degrees)."""
    Rs, ts, errs = [], [], []
    gt = Pose(T_gt[None].float())
    for k in range(4):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad([5.0, 12.0, 25.0, 60.0][k])
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        dR = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        R = torch.from_numpy(dR).float() @ T_gt[:9].reshape(3, 3).float()
        tn = float(T_gt[9:].norm())
        side = rng.normal(size=3)
        t = T_gt[9:].float() * [1.0, -2.0, 0.5, 1.0][k] + torch.from_numpy(side / np.linalg.norm(side) * tn * [0.2, 0.5, 0.3, 2.0][k]).float()
        t_err, r_err = relative_pose_error(gt, R, t)
        assert 3.0 < float(t_err) <= 90.0 and 3.0 < float(r_err) < 177.0, (float(t_err), float(r_err))
        Rs.append(R)
        ts.append(t)
        errs.append(torch.stack([torch.as_tensor(t_err).float().reshape(()), r_err.float().reshape(())]))
    return torch.stack(Rs), torch.stack(ts), torch.stack(errs)


def build(seed):
    rng = np.random.default_rng(seed)
    out = {}
    per_case = []
    for c, (model, coeffs) in enumerate(CASES):
        items, preds = synthetic.posed_plane_pairs(1, H, W, seed=1000 * seed + c, model=model, num_keypoints=(M, N), coeffs=coeffs)
        item, pred = items[0], preds[0]
        info = plant(rng, item, pred, model)
        f32 = evaluate(item, pred, model, torch.float32)
        f64 = evaluate(item, pred, model, torch.float64)
        R_est, t_est, pose_err = pose_error_cases(rng, item["T_0to1"]._data[0])
        rec = {"kp0": pred["keypoints0"], "kp1": pred["keypoints1"], "matches0": pred["matches0"],
               "depth0": item["view0"]["depth"][0], "depth1": item["view1"]["depth"][0],
               "cam0": item["view0"]["camera"]._data[0], "cam1": item["view1"]["camera"]._data[0],
               "T_0to1": item["T_0to1"]._data[0], "R_est": R_est, "t_est": t_est, "pose_err": pose_err,
               "dup_row": torch.tensor(info["dup_row"]), "dup_col": torch.tensor(info["dup_col"]),
               "dup_kp0": torch.tensor(info["dup_kp0"]), "dup_kp1": torch.tensor(info["dup_kp1"]), **f32,
               **{k + "_f64": v for k, v in f64.items() if v.dtype == torch.float64 and k not in ("metrics7", "metrics5")}}
        per_case.append(rec)
    for k in per_case[0]:
        out[k] = np.stack([r[k].numpy() for r in per_case])
    out["models"] = np.array([m for m, _ in CASES])
    return out


def main():
    seed = int(sys.argv[sys.argv.index("--seed") + 1]) if "--seed" in sys.argv else 0
    for s in range(seed, seed + 200):
        try:
            fx = build(s)
        except AssertionError as e:
            print(f"seed {s}: {e}")
            continue
        counts = pr.undecidable_counts(fx)
        cover = pr.coverage(fx)
        print(f"seed {s}: undecidable {counts}\n  coverage {cover}")
        ties = cover["tie_row"] == len(CASES) and cover["tie_col"] == len(CASES)  # every pair holds both planted ties
        if not any(counts.values()) and all(v > 0 for v in cover.values()) and ties:
            fx["seed"] = np.array(s)
            path = os.path.join(HERE, "pose_depth.npz")
            np.savez_compressed(path, **fx)
            print(f"pose_depth: {os.path.getsize(path) / 1024:.0f} KB, seed {s}, keys={sorted(fx)}")
            return 0
    raise SystemExit("no decidable seed found")


if __name__ == "__main__":
    raise SystemExit(main())
