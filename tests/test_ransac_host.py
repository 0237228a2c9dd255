"""The parts of the GPU RANSAC homography estimator that need no GPU: the sampler's definition
(`eval_utils.ransac_sample_indices`, pure-integer numpy, which the kernel must match index for index), the float64
restatement of the algorithm (tests/ransac_reference.py) on the seeded regimes the GPU tests compare against, the
argument checks of the C entry point (they return before anything is launched) and the Python-side refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_reference as rr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import eval_hpatches, eval_utils  # noqa: E402
from glue_factory_colon_amd.homography_estimator import GpuHomographyEstimator  # noqa: E402


def test_sample_indices_are_distinct_in_range_and_a_function_of_their_arguments():
    for n in (4, 5, 6, 7, 8, 9, 13, 64, 257, 1000, 4999, 5000):
        s = eval_utils.ransac_sample_indices(3, 17, n, 4096)
        assert s.shape == (4096, 4) and s.dtype == np.int64
        assert s.min() >= 0 and s.max() < n
        srt = np.sort(s, axis=1)
        assert (srt[:, 1:] != srt[:, :-1]).all(), n
    with pytest.raises(ValueError):
        eval_utils.ransac_sample_indices(0, 0, 3, 8)
    # no state and no dependence on how many hypotheses are asked for: hypothesis h is a function of (seed, stream, n, h)
    a = eval_utils.ransac_sample_indices(5, 123456789012, 300, 2048)
    assert np.array_equal(a, eval_utils.ransac_sample_indices(5, 123456789012, 300, 2048))
    assert np.array_equal(a[:100], eval_utils.ransac_sample_indices(5, 123456789012, 300, 100))
    # ... and another stream, seed or n gives other samples
    for other in (eval_utils.ransac_sample_indices(6, 123456789012, 300, 2048),
                  eval_utils.ransac_sample_indices(5, 123456789013, 300, 2048),
                  eval_utils.ransac_sample_indices(5, 123456789012, 301, 2048)):
        assert (other != a).any(axis=1).mean() > 0.9


def test_sample_indices_are_uniform():
    k = 1 << 16
    for n in (4, 5, 7, 12, 60, 1000):
        s = eval_utils.ransac_sample_indices(11, 2, n, k)
        p = 4.0 / n  # a hypothesis holds index i with probability 4 / n
        counts = np.bincount(s.ravel(), minlength=n)
        sd = np.sqrt(k * p * (1 - p))
        assert np.abs(counts - k * p).max() <= 5 * sd + 1e-9, (n, np.abs(counts - k * p).max() / max(sd, 1e-9))
        # every position of the sample is uniform too
        for j in range(4):
            cj = np.bincount(s[:, j], minlength=n)
            assert np.abs(cj - k / n).max() <= 5 * np.sqrt(k / n * (1 - 1 / n)), (n, j)


def test_sample_indices_literal():
    """The definition, pinned: DESIGN.md writes the function down, the kernel and numpy implement it."""
    assert eval_utils.ransac_sample_indices(0, 0, 12, 4).tolist() == [[4, 2, 10, 11], [7, 4, 0, 1], [5, 3, 7, 8], [3, 4, 2, 1]]
    assert eval_utils.ransac_sample_indices(7, 123456789, 5000, 3).tolist() == [
        [4997, 1566, 4313, 852], [1758, 4828, 4673, 2261], [916, 2307, 1439, 2634]]


def test_four_point_solve_and_its_degeneracies():
    rng = np.random.default_rng(0)
    H = np.array([[1.1, 0.05, 12.0], [-0.04, 0.95, -7.0], [1e-4, -5e-5, 1.0]])
    p = rng.uniform(0, 500, (64, 4, 2))
    ph = np.concatenate([p, np.ones((64, 4, 1))], -1) @ H.T
    q = ph[..., :2] / ph[..., 2:]
    est, ok = rr.homography_4pt(p[..., 0], p[..., 1], q[..., 0], q[..., 1])
    assert ok.all() and np.abs(est - H.reshape(1, 9)).max() < 1e-7
    # three collinear points in either image, or coincident points: skipped
    col = p.copy()
    col[:, 2] = 0.5 * (col[:, 0] + col[:, 1])
    assert not rr.homography_4pt(col[..., 0], col[..., 1], q[..., 0], q[..., 1])[1].any()
    assert not rr.homography_4pt(p[..., 0], p[..., 1], col[..., 0], col[..., 1])[1].any()
    same = np.full((1, 4), 3.0)
    assert not rr.homography_4pt(same, same, same, same)[1].any()


def test_restatement_on_the_table():
    worst = {"free": 0.0, "t05": 0.0, "noisy": 0.0}
    for ths in ([0.5, 1.0, 3.0], rr.SWEEP):
        for r, k, c, hyp in rr.table_cases():
            n, share, sigma, _ = rr.TABLE[r]
            res = rr.ransac(c["kp0"], c["kp1"], c["m0"], ths, hyp, 3, 0, 100 * r + k, c["H_gt"], c["size"])
            assert len(res) == len(ths)
            for t, x in zip(ths, res):
                assert x["success"] and 0 <= x["best_hypothesis"] < hyp
                key = "free" if sigma == 0 else ("t05" if t < 1 else "noisy")
                worst[key] = max(worst[key], x["error"])
                assert x["error"] <= rr.error_bound(sigma, t), (r, k, t, x["error"])
                # local optimisation never raises the MSAC score: every accepted score is strictly lower
                assert all(b < a for a, b in zip(x["lo_scores"], x["lo_scores"][1:])), x["lo_scores"]
                corr, idx = rr.correspondences(c["kp0"], c["kp1"], c["m0"])
                t2 = float(np.float32(t)) ** 2
                assert rr.msac(rr.residual2(x["H"], corr), t2)[0] <= rr.msac(rr.residual2(x["H_minimal"], corr), t2)[0]
                assert x["num_inliers"] == int(x["inliers"].sum()) and not x["inliers"][c["m0"] < 0].any()
                if sigma == 0:  # every clean match is an inlier, no outlier is
                    assert np.array_equal(x["inliers"], c["clean"]), (r, k, t)
    print("largest restatement errors:", worst)
    assert worst["free"] <= rr.MEASURED_MAX_NOISE_FREE * 1.01 and worst["t05"] <= rr.MEASURED_MAX_NOISY_T05 * 1.01
    assert worst["noisy"] <= rr.MEASURED_MAX_NOISY * 1.01


def test_restatement_failure_cases():
    c = rr.make_case(12, 0.0, 0.0, seed=5)
    three = c["m0"].copy()
    three[np.nonzero(three >= 0)[0][3:]] = -1
    none = np.full_like(c["m0"], -1)
    same0, same1 = np.tile(c["kp0"][:1], (12, 1)), np.tile(c["kp1"][:1], (12, 1))
    for kp0, kp1, m0 in ((c["kp0"], c["kp1"], three), (c["kp0"], c["kp1"], none), (same0, same1, c["m0"]),
                         (c["kp0"][:0], c["kp1"][:0], c["m0"][:0])):
        for x in rr.ransac(kp0, kp1, m0, [0.5, 1.0, 3.0], 256, 3, 0, 0, c["H_gt"], c["size"]):
            assert not x["success"] and x["best_hypothesis"] == -1 and x["error"] == float("inf")
            assert np.array_equal(x["H"], np.eye(3).reshape(9)) and x["num_inliers"] == 0 and not x["inliers"].any()


def test_thresholds_and_best_threshold_selection():
    assert eval_utils.ransac_thresholds(2.0) == [2.0]
    assert eval_utils.ransac_thresholds(-1) == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    assert eval_utils.ransac_thresholds([1.0, 4]) == [1.0, 4.0]
    for bad in ([], [1.0] * 9, [1.0, 0.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="thresholds"):
            eval_utils.ransac_thresholds(bad)
    pose = {0.5: {"H_error_ransac": [0.4, 6.0, float("inf")], "ransac_inl": [10.0, 4.0, 0.0], "ransac_inl%": [0.5, 0.1, 0.0]},
            2.0: {"H_error_ransac": [0.6, 0.9, 2.0], "ransac_inl": [12.0, 9.0, 5.0], "ransac_inl%": [0.6, 0.3, 0.2]}}
    summ, best = eval_hpatches.robust_summaries(pose)
    assert best == 2.0
    want = eval_hpatches.cal_error_auc(pose[2.0]["H_error_ransac"], [1, 3, 5])
    assert [summ[f"H_error_ransac@{t}px"] for t in (1, 3, 5)] == [float(v) for v in want]
    assert summ["H_error_ransac_mAA"] == pytest.approx(float(np.mean(want)))
    assert summ["mean_ransac_inl"] == round(26 / 3, 3) and summ["med_ransac_inl%"] == 0.3
    assert summ["med_H_error_ransac"] == 0.9


def test_python_refusals_need_no_gpu():
    cpu = torch.zeros(1, 8, 2)
    with pytest.raises(nat.NativeError, match="cuda"):
        eval_utils.homography_ransac(None, cpu, cpu, torch.zeros(1, 8, dtype=torch.long), None, 1.0)
    est = GpuHomographyEstimator({"ransac_th": 1.5})
    assert est.conf.ransac_th == 1.5 and est.conf.options.num_hypotheses == 2048 and est.conf.options.lo_iters == 3
    assert est.required_data_keys == ["m_kpts0", "m_kpts1"] and GpuHomographyEstimator().conf.ransac_th == 2.0
    with pytest.raises(nat.NativeError, match="cuda"):
        est({"m_kpts0": cpu[0], "m_kpts1": cpu[0]})
    with pytest.raises(ValueError, match="unknown options"):
        GpuHomographyEstimator({"options": {"confidence": 0.99}})
    data = {"H_0to1": torch.eye(3), "view0": {"image_size": torch.tensor([640.0, 480.0])}}
    pred = {"keypoints0": cpu[0], "keypoints1": cpu[0], "matches0": torch.zeros(8, dtype=torch.long)}
    for name in ("poselib", "opencv", None):
        with pytest.raises(ValueError, match="gfc_amd"):
            eval_utils.eval_homography_robust(data, pred, {"estimator": name, "ransac_th": 1.0})
    with pytest.raises(NotImplementedError, match="line"):
        eval_utils.eval_homography_robust(data, {**pred, "lines0": cpu[0]}, {"estimator": "gfc_amd", "ransac_th": 1.0})


def test_c_entry_point_refuses_bad_arguments_before_any_launch():
    """GFC_ERR_INVALID comes from the host-side checks: nothing is launched and no pointer is followed, so dummy
    non-null addresses do and the test runs without a GPU."""
    lib = nat.lib()
    d = ctypes.c_void_p(0x1000)  # never dereferenced

    def call(B=2, M=16, N=16, ths=(1.0,), T=None, nh=64, lo=3, kp0=d, m0=d, out=d, ws=d, H_gt=None, size=None, err=None):
        arr = (ctypes.c_float * max(len(ths), 1))(*ths)
        return lib.gfc_eval_homography_ransac(kp0, d, m0, None, H_gt, size, B, M, N, arr if ths is not None else None,
                                              len(ths) if T is None else T, nh, lo, 0, out, d, d, d, d, d, err, ws, 1 << 30,
                                              None)

    invalid = 1
    assert call(B=0) == invalid and call(B=-1) == invalid and call(M=-1) == invalid and call(N=-1) == invalid
    assert call(T=0) == invalid and call(ths=(1.0,) * 9) == invalid  # the cap is 8 thresholds
    assert call(nh=0) == invalid and call(nh=-5) == invalid and call(lo=-1) == invalid
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(ths=(1.0, bad)) == invalid, bad
    assert call(kp0=None) == invalid and call(m0=None) == invalid and call(out=None) == invalid and call(ws=None) == invalid
    assert call(H_gt=d) == invalid and call(H_gt=d, size=d) == invalid  # H_gt, image_size0, err_out: all or none
    assert lib.gfc_eval_homography_ransac_workspace_bytes(0, 16, 1, 64) == 0
    assert lib.gfc_eval_homography_ransac_workspace_bytes(2, 16, 9, 64) == 0
    small = lib.gfc_eval_homography_ransac_workspace_bytes(2, 16, 1, 64)
    assert 0 < small <= lib.gfc_eval_homography_ransac_workspace_bytes(540, 1024, 6, 2048)


def test_ransac_kernels_compile_without_scratch():
    """hipcc's resource report for csrc/ransac.hip (the library's own flags): every kernel of the unit, the scoring
    kernel for each threshold count included, uses 0 bytes of scratch and spills no register."""
    import importlib.util
    import re
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gfc_build_for_test", os.path.join(root, "glue-factory-colon_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = os.path.join(mod.HERE, "ransac.hip")
    r = subprocess.run([mod._hipcc(), *mod.FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    report = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and name:
            report[name][m.group(1)] = int(m.group(2))
    scoring = [k for k in report if "ransac_score_kernel" in k]
    assert len(scoring) == 8 and any("ransac_lo_kernel" in k for k in report) and any("ransac_compact_kernel" in k for k in report)
    for k, v in report.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, (k, v)
