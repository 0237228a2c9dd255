"""tests/pose_reference.py (the torch checker of the pose / depth kernels) against vectors the reference project
produced (tests/golden/pose_depth.npz, written by tests/golden/make_golden_pose.py), on the CPU.

1. The restatement equals the fixture: integers and masks exactly, floats to 1e-5 relative to 1 + |value| in float32
   (pixel coordinates reach 128: one float32 ulp there is 7.6e-6) and to 1e-9 against the reference's float64 run.
2. The fixture is decidable: ZERO reference values lie within a rounding error of a decision (threshold, argmin,
   image bound, depth sign, sampling cell), so the GPU comparison (test_gpu_eval_pose.py) excuses nothing; and it
   covers every special case it was built for.
3. Each deliberately wrong rule (pose_reference.WRONG_RULES) is rejected by the fixture.
4. The host pieces that need no GPU: geometry holders, relative_pose_error, eval_poses, the missing estimator,
   synthetic.posed_plane_pairs.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_reference as pr  # noqa: E402

from glue_factory_colon_amd import eval_utils, geometry, synthetic  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_depth.npz")
CASES = (0, 1, 2)


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case_args(fx, c, dtype=torch.float32):
    t = lambda k: torch.from_numpy(fx[k][c])  # noqa: E731
    model = str(fx["models"][c])
    return dict(kp0=t("kp0").to(dtype), kp1=t("kp1").to(dtype), depth0=t("depth0").to(dtype), depth1=t("depth1").to(dtype),
                cam0=t("cam0").to(dtype), model0=model, cam1=t("cam1").to(dtype), model1=model, T_0to1=t("T_0to1").to(dtype))


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    same_inf = np.isinf(a) & (a == b)
    diff = np.where(both_nan | same_inf, 0.0, np.abs(a - b))
    worst = float(np.nanmax(diff / (1 + np.abs(np.where(np.isfinite(b), b, 0)))) if diff.size else 0.0)
    assert not np.isnan(diff).any() and worst <= tol, worst


@pytest.mark.parametrize("c", CASES)
@pytest.mark.parametrize("dtype,suffix,tol", [(torch.float32, "", 1e-5), (torch.float64, "_f64", 1e-9)])
def test_restatement_equals_the_reference(fx, c, dtype, suffix, tol):
    a = case_args(fx, c, dtype)
    m0 = torch.from_numpy(fx["matches0"][c])
    gt = pr.gt_matches(**a)
    for mine, key in (("depth_keypoints0", "depth_kp0"), ("depth_keypoints1", "depth_kp1"), ("proj_0to1", "proj_0to1"),
                      ("proj_1to0", "proj_1to0")):
        close(gt[mine].numpy(), fx[key + suffix][c], tol)
    for key in ("valid0", "valid1", "visible0", "visible1"):
        assert np.array_equal(gt[key].numpy(), fx[key][c]), key
    assert np.array_equal(gt["matches0"].numpy(), fx["gt_matches0"][c])
    assert np.array_equal(gt["matches1"].numpy(), fx["gt_matches1"][c])
    if dtype == torch.float32:
        close(pr.invert_pose(a["T_0to1"]).numpy(), fx["T_1to0"][c], tol)
    nm = int((m0 > -1).sum())
    err, valid = pr.reprojection_errors(a["kp0"], a["kp1"], m0, a["depth0"], a["depth1"], a["cam0"], a["model0"],
                                        a["cam1"], a["model1"], a["T_0to1"])
    assert np.array_equal(valid.numpy(), fx["reproj_valid"][c][:nm])
    close(err.numpy(), fx["reproj_err" + suffix][c][:nm], tol)
    sel = m0 > -1
    epi = pr.epipolar_errors(a["kp0"][sel], a["kp1"][m0[sel]], a["cam0"], a["model0"], a["cam1"], a["model1"], a["T_0to1"])
    close(epi.numpy(), fx["epi_err" + suffix][c][:nm], tol)
    # the camera functions on their own
    nx, ny = pr.pixel_to_ray(a["cam0"], a["model0"], a["kp0"][:, 0], a["kp0"][:, 1])
    close(torch.stack([nx, ny, torch.ones_like(nx)], -1).numpy(), fx["ray0" + suffix][c], tol)
    P = torch.from_numpy(fx["p3d_1" + suffix][c])
    px, py, ok = pr.ray_to_pixel(a["cam1"], a["model1"], P[:, 0], P[:, 1], P[:, 2])
    close(torch.stack([px, py], -1).numpy(), fx["c2i" + suffix][c], tol)
    assert np.array_equal(ok.numpy(), fx["c2i_valid"][c])


def test_metrics_equal_the_reference(fx):
    b = {k: torch.stack([case_args(fx, c)[k] for c in CASES]) for k in ("kp0", "kp1", "depth0", "depth1", "cam0", "cam1", "T_0to1")}
    m0 = torch.from_numpy(fx["matches0"])
    for c in CASES:  # the model is one argument of a call: one case per call
        s = slice(c, c + 1)
        model = str(fx["models"][c])
        m7, g0, g1 = pr.depth_metrics(b["kp0"][s], b["kp1"][s], m0[s], b["depth0"][s], b["depth1"][s], b["cam0"][s], model,
                                      b["cam1"][s], model, b["T_0to1"][s])
        m5 = pr.epipolar_metrics(b["kp0"][s], b["kp1"][s], m0[s], b["cam0"][s], model, b["cam1"][s], model, b["T_0to1"][s])
        assert m7[0, 3] == fx["metrics7"][c][3] and tuple(m5[0, 3:]) == tuple(fx["metrics5"][c][3:])  # counts: exactly
        close(m7[0].numpy(), fx["metrics7"][c], 1e-6)
        close(m5[0].numpy(), fx["metrics5"][c], 1e-6)
        assert np.array_equal(g0[0].numpy(), fx["gt_matches0"][c]) and np.array_equal(g1[0].numpy(), fx["gt_matches1"][c])


def test_fixture_is_decidable_and_covers_its_cases(fx):
    counts = pr.undecidable_counts(fx)
    assert counts == {k: 0 for k in counts}, counts
    cover = pr.coverage(fx)
    assert all(v > 0 for v in cover.values()), cover
    assert cover["tie_row"] == len(CASES) and cover["tie_col"] == len(CASES), cover  # both planted ties in every pair
    assert fx["kp0"].shape[1:] == (257, 2) and fx["kp1"].shape[1:] == (130, 2) and fx["depth0"].shape[1:] == (96, 128)
    assert list(fx["models"]) == ["PINHOLE", "OPENCV", "OPENCV_FISHEYE"]
    assert np.count_nonzero(fx["cam0"][1][6:10]) == 4  # OPENCV with all four coefficients


@pytest.mark.parametrize("rule", pr.WRONG_RULES)
def test_fixture_rejects_wrong_rule(fx, rule):
    """last_index_ties: ties go to the last index; masked_d0_negatives: the negative rule reads the visibility-masked
    distances; in_image_lt_size: a projection counts as inside up to `< size` instead of `<= size - 1`."""
    rejected = 0
    for c in CASES:
        gt = pr.gt_matches(**case_args(fx, c), rule=rule)
        same = all(np.array_equal(gt[mine].numpy(), fx[key][c]) for mine, key in
                   (("matches0", "gt_matches0"), ("matches1", "gt_matches1"), ("visible0", "visible0"), ("visible1", "visible1")))
        rejected += not same
    assert rejected == len(CASES), f"{rule}: only {rejected} of {len(CASES)} fixture pairs tell it from the right rule"


def test_relative_pose_error_equals_the_reference(fx):
    for c in CASES:
        T = torch.from_numpy(fx["T_0to1"][c])
        for R, t, want in zip(fx["R_est"][c], fx["t_est"][c], fx["pose_err"][c]):
            for fn, gt in ((pr.relative_pose_error, T), (eval_utils.relative_pose_error, geometry.Pose(T[None]))):
                t_err, r_err = fn(gt, torch.from_numpy(R), torch.from_numpy(t))
                assert abs(float(t_err) - want[0]) < 1e-4 and abs(float(r_err) - want[1]) < 1e-4, (c, t_err, r_err, want)
    T4 = torch.eye(4)
    T4[:3, 3] = torch.tensor([1e-3, 0.0, 0.0])
    t_err, r_err = eval_utils.relative_pose_error(T4, torch.eye(3), torch.tensor([0.0, 1.0, 0.0]), ignore_gt_t_thr=0.01)
    assert float(t_err) == 0.0 and float(r_err) == 0.0


def test_geometry_holders():
    K = torch.tensor([[100.0, 0, 64], [0, 110, 48], [0, 0, 1]])
    cam = geometry.Camera.from_calibration_matrix(K)
    assert cam.model == "PINHOLE" and cam._data.tolist() == [128, 96, 100, 110, 64, 48]
    col = geometry.Camera.from_colmap({"model": "SIMPLE_RADIAL", "width": 128, "height": 96, "params": [100.0, 64, 48, -0.1]})
    assert col._data.tolist() == [128, 96, 100, 100, 64, 48, -0.1, 0.0] and geometry.model_id(col) == geometry.GFC_CAM_RADIAL
    col = geometry.Camera.from_colmap({"model": "OPENCV", "width": 128, "height": 96, "params": [100.0, 101, 64, 48, 1, 2, 3, 4]})
    assert col._data.tolist() == [128, 96, 100, 101, 64, 48, 1, 2, 3, 4] and geometry.model_id(col) == geometry.GFC_CAM_OPENCV
    fish = geometry.Camera.from_npz({"model": "OPENCV_FISHEYE", "width": 128, "height": 96,
                                     "params": np.array([70.0, 71, 64, 48, 0.1, 0.2, 0.3, 0.4])})
    assert fish.model == "OPENCV_FISHEYE" and fish._data.dtype == torch.float32 and fish._data.shape == (10,)
    assert geometry.model_id(fish) == geometry.GFC_CAM_OPENCV_FISHEYE
    with pytest.raises(NotImplementedError):
        geometry.Camera.from_npz({"model": "PINHOLE", "width": 1, "height": 1, "params": np.zeros(4)})
    s = fish.scale(torch.tensor([0.5, 0.25]))
    assert s.model == "OPENCV_FISHEYE" and s._data.tolist()[:6] == [64, 24, 35, 17.75, 32, 12]
    assert torch.equal(s.dist, fish.dist)
    cr = fish.crop((10, 20), (50, 40))
    assert cr._data.tolist()[:6] == [50, 40, 70, 71, 54, 28] and cr.model == "OPENCV_FISHEYE"
    stacked = geometry.Camera.stack([fish, fish])
    assert stacked._data.shape == (2, 10) and stacked[1].model == "OPENCV_FISHEYE"
    arr, mid = geometry.camera_args(cam, 1, "cpu")
    assert arr.shape == (1, 10) and mid == geometry.GFC_CAM_PINHOLE and arr[0, 6:].tolist() == [0, 0, 0, 0]
    R = torch.tensor([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    P = geometry.Pose.from_Rt(R, torch.tensor([1.0, 2, 3]))
    T4 = torch.eye(4)
    T4[:3, :3], T4[:3, 3] = R, torch.tensor([1.0, 2, 3])
    assert torch.equal(geometry.Pose.from_4x4mat(T4)._data, P._data)
    assert torch.equal(P.inv().R, R.T) and torch.allclose(P.inv().t, -(R.T @ P.t))
    assert torch.equal(P.inv()._data, pr.invert_pose(P._data))
    fwd, inv = geometry.pose_args(T4, 1, "cpu")
    assert torch.equal(fwd[0], P._data) and torch.equal(inv[0], P.inv()._data)


def test_eval_poses_and_the_missing_estimator():
    pose_results = {0.5: {"rel_pose_error": [1.0, 30.0, 2.0], "ransac_inl": [10, 0, 12], "names": ["a", "b", "c"]},
                    1.0: {"rel_pose_error": [0.5, 4.0, 2.0], "ransac_inl": [11, 5, 12], "names": ["a", "b", "c"]}}
    summaries, best = eval_utils.eval_poses(pose_results, [5, 10, 20], "rel_pose_error")
    assert best == 1.0
    from glue_factory_colon_amd.eval_hpatches import cal_error_auc
    want = cal_error_auc([0.5, 4.0, 2.0], [5, 10, 20])
    assert [summaries[f"rel_pose_error@{t}°"] for t in (5, 10, 20)] == [float(a) for a in want]
    assert summaries["rel_pose_error_mAA"] == float(np.mean(want))
    assert summaries["med_rel_pose_error"] == 2.0 and summaries["mean_ransac_inl"] == round(28 / 3, 3)
    assert "med_names" not in summaries
    with pytest.raises(NotImplementedError, match="five-point"):
        eval_utils.eval_relative_pose_robust({}, {}, {"estimator": "poselib", "ransac_th": 1.0})
    with pytest.raises(NotImplementedError):
        eval_utils.gt_matches_from_pose_depth(torch.zeros(1, 1, 2), torch.zeros(1, 1, 2), {}, epi_th=1.0)


@pytest.mark.parametrize("model", pr.MODELS)
def test_posed_plane_pairs(model):
    items, preds = synthetic.posed_plane_pairs(2, 48, 64, seed=5, model=model, num_keypoints=(70, 45))
    again, preds2 = synthetic.posed_plane_pairs(2, 48, 64, seed=5, model=model, num_keypoints=(70, 45))
    assert all(torch.equal(p[k], q[k]) for p, q in zip(preds, preds2) for k in p)
    assert torch.equal(items[1]["view1"]["depth"], again[1]["view1"]["depth"])
    it, p = items[1], preds[1]
    assert it["view0"]["depth"].shape == (1, 48, 64) and it["view0"]["camera"].model == model
    assert (it["view0"]["depth"] == 0).any() and (it["view0"]["depth"] > 0).any()
    assert p["keypoints0"].shape == (70, 2) and p["keypoints1"].shape == (45, 2)
    m0 = p["matches0"]
    assert len(set(m0[m0 > -1].tolist())) == int((m0 > -1).sum())  # one-to-one
    # the planted matches carry the four noise levels: the reprojection error of a planted match is its noise level
    # up to the interpolation of the depth map and, for the distorting models, the asymmetry of the two directions
    err, valid = pr.reprojection_errors(p["keypoints0"], p["keypoints1"], m0, it["view0"]["depth"][0], it["view1"]["depth"][0],
                                        it["view0"]["camera"]._data[0], model, it["view1"]["camera"]._data[0], model,
                                        it["T_0to1"]._data[0])
    e = err[valid]
    for lo, hi in ((0.0, 1.0), (1.0, 3.0), (3.0, 5.0), (5.0, 1e9)):
        assert ((e >= lo) & (e < hi)).any(), (lo, hi)
