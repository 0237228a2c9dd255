"""The GPU five-point RANSAC relative-pose estimator (csrc/relpose.hip through eval_utils.relative_pose_ransac) against
the float64 restatement of its algorithm (tests/relpose_reference.py) and against properties that need no reference.
Parity with OpenCV's / PoseLib's / pycolmap's estimators is NOT tested: randomised CPU libraries that are not available
here.

Inputs: the seeded scenes of relpose_reference.table_cases(), the six-threshold sweep.  All scenes of one shape (M,
camera model) go through ONE batched call.  Identity-camera rows hand both sides the same fp32 bearings (delta = 1e-9:
fp64 on both sides); the PINHOLE and OPENCV_FISHEYE rows go through ep_image2cam in fp32 (delta = 2e-3 px / f).  The
bounds on E_minimal and on (R, t) are constants the restatement measured on itself (relpose_reference.MEASURED_*,
guarded by test_relpose_reference_host.py), times 100.  The (R, t) bound is about reduction orders, so it needs the same
inputs on both sides: for the two camera rows the restatement is also run on the kernel's own fp32 bearings
(eval_utils.pose_image2cam), and its mirror of ep_image2cam is checked against them separately."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relpose_reference as rr  # noqa: E402

from glue_factory_colon_amd import eval_utils, geometry, synthetic  # noqa: E402
from glue_factory_colon_amd.eval_pose_pairs import PosePairsPipeline  # noqa: E402
from glue_factory_colon_amd.export_predictions import _write  # noqa: E402
from glue_factory_colon_amd.relative_pose_estimator import GpuRelativePoseEstimator  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_KEYS = ("R", "t", "E", "E_minimal", "inliers", "num_inliers", "success", "best_hypothesis", "best_solution", "r_err",
            "t_err")


def camera_of(cams, model):
    data = torch.from_numpy(np.stack(cams)).float()
    if model == "OPENCV_FISHEYE":
        return geometry.Camera(data, model=model)
    return geometry.Camera(data[:, :6].contiguous())


def gpu_run(cases, ths, hyp, sids, seed=0, lo_iters=3, with_gt=True):
    st = lambda key, dtype: torch.from_numpy(np.stack([c[key] for c in cases])).to(device="cuda", dtype=dtype)  # noqa: E731
    model = cases[0]["model"]
    T = geometry.Pose(st("T_gt", torch.float32)) if with_gt else None
    out = eval_utils.relative_pose_ransac(st("kp0", torch.float32), st("kp1", torch.float32), st("m0", torch.long),
                                          camera_of([c["cam0"] for c in cases], model),
                                          camera_of([c["cam1"] for c in cases], model), ths, T, num_hypotheses=hyp,
                                          lo_iters=lo_iters, seed=seed, stream_id=sids)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b, keys=OUT_KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys if k in a)


@pytest.fixture(scope="module")
def records():
    """One record per scene: the GPU's outputs [T, ...] and the restatement's list over the thresholds."""
    groups = {}
    for e in rr.table_cases():
        groups.setdefault((len(e["case"]["kp0"]), e["camera"], e["hypotheses"]), []).append(e)
    recs = []
    for (n, cam, hyp), members in groups.items():
        ths = rr.thresholds_for(members[0])
        out = gpu_run([e["case"] for e in members], ths, hyp, [e["stream_id"] for e in members])
        for j, e in enumerate(members):
            rec, idx = rr.records(e["case"])
            one = {"entry": e, "ths": ths, "gpu": {k: out[k][j] for k in OUT_KEYS}, "rec": rec, "idx": idx,
                   "ref": rr.ransac(e["case"], ths, hyp, 3, 0, e["stream_id"])}
            one["ref_same"], one["rec_same"] = one["ref"], rec
            if cam is not None:
                # the same scene with the kernel's own fp32 bearings handed to the restatement: identical inputs on
                # both sides, which is what the bound on (R, t) presupposes (the identity-camera rows have it by
                # construction; tanf of the fisheye model is not the same function bit for bit on the two sides)
                c = e["case"]
                bear = [eval_utils.pose_image2cam(torch.from_numpy(c[k])[None].cuda(), camera_of([c[q]], c["model"]))[0].cpu().numpy()
                        for k, q in (("kp0", "cam0"), ("kp1", "cam1"))]
                same_case = {**c, "bearings": bear}
                one["rec_same"], _ = rr.records(same_case)
                one["ref_same"] = rr.ransac(same_case, ths, hyp, 3, 0, e["stream_id"])
            recs.append(one)
    return recs


def test_bearings_of_the_camera_rows(records):
    """The restatement's fp32 mirror of ep_image2cam is within delta of the kernel's bearings (equal for PINHOLE)."""
    seen = 0
    for r in records:
        if r["entry"]["camera"] is None:
            continue
        d = np.abs(r["rec"] - r["rec_same"]).max()
        print(r["entry"]["camera"], "largest bearing difference:", d)
        assert d <= rr.delta_for(r["entry"])
        if r["entry"]["camera"] == "PINHOLE":
            assert d == 0
        seen += 1
    assert seen == 4


def angle(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return 2.0 * np.arcsin(min(1.0, 0.5 * min(np.linalg.norm(a - b), np.linalg.norm(a + b))))


def outlier_free(e):
    _, share, sigma, _ = rr.REGIMES[e["regime"]]
    return share == 0 and sigma == 0


def test_sampler_through_the_kernel(records):
    """1. E_minimal is, up to sign, one of the restatement's models of ransac_sample_indices(...)[best_hypothesis]."""
    worst, checked = 0.0, 0
    for r in records:
        e = r["entry"]
        if not outlier_free(e):
            continue
        samples = eval_utils.ransac_sample_indices(0, e["stream_id"], len(r["rec"]), e["hypotheses"], sample_size=5)
        for t in range(len(r["ths"])):
            h, k = int(r["gpu"]["best_hypothesis"][t]), int(r["gpu"]["best_solution"][t])
            assert 0 <= h < e["hypotheses"] and 0 <= k < 10
            E, ok = rr.five_point(r["rec"][samples[h]][None])
            assert ok[0].any()
            d = min(angle(r["gpu"]["E_minimal"][t], E[0, q]) for q in np.nonzero(ok[0])[0])
            assert ok[0, k] and angle(r["gpu"]["E_minimal"][t], E[0, k]) == d
            worst = max(worst, d)
            checked += 1
    print("largest angle between E_minimal and the restatement's model (rad):", worst, "over", checked)
    assert checked >= 36 and worst <= 100 * rr.MEASURED_ROUTE_SPREAD


def test_winner(records):
    """2. The float64 score of the GPU's (h, k) is within 2 t delta n of the restatement's best."""
    other, total = 0, 0
    for r in records:
        delta = rr.delta_for(r["entry"])
        for t, ref in enumerate(r["ref"]):
            h, k = int(r["gpu"]["best_hypothesis"][t]), int(r["gpu"]["best_solution"][t])
            assert r["gpu"]["success"][t] and ref["success"]
            gap = ref["scores"][h, k] - ref["scores"][ref["best_hypothesis"], ref["best_solution"]]
            bound = 2 * np.sqrt(ref["t2"]) * delta * len(r["rec"])
            if (h, k) != (ref["best_hypothesis"], ref["best_solution"]):
                other += 1
                print("another winner:", r["entry"]["row"], r["entry"]["scene"], t, (h, k), "gap", gap, "bound", bound)
            assert 0 <= gap <= bound, (r["entry"]["row"], r["entry"]["scene"], t, gap, bound)
            total += 1
    print(other, "of", total, "(scene, threshold) cases pick another hypothesis")
    assert other <= 0.1 * total


def test_same_winner_same_result(records):
    """3. inliers outside the delta band, counts, (R, t) and the pose errors."""
    worst_rt, worst_err, worst_band, compared = 0.0, 0.0, 0.0, 0
    for r in records:
        e, g = r["entry"], r["gpu"]
        delta = rr.delta_for(e)
        Tgt = torch.from_numpy(e["case"]["T_gt"])
        rec = r["rec_same"]
        for t, ref in enumerate(r["ref_same"]):
            assert int(g["num_inliers"][t]) == int(g["inliers"][t].sum())
            t_err, r_err = eval_utils.relative_pose_error(geometry.Pose(Tgt), g["R"][t], g["t"][t])
            worst_err = max(worst_err, abs(float(r_err) - g["r_err"][t]), abs(float(t_err) - g["t_err"][t]))
            if (int(g["best_hypothesis"][t]), int(g["best_solution"][t])) != (ref["best_hypothesis"], ref["best_solution"]):
                continue
            d = np.sqrt(rr.sampson2(ref["E"], rec))
            band = np.zeros(len(e["case"]["kp0"]), bool)
            band[r["idx"]] = np.abs(d - np.sqrt(ref["t2"])) < delta
            worst_band = max(worst_band, band.sum() / len(rec))
            assert (g["inliers"][t] == ref["inliers"])[~band].all(), (e["row"], e["scene"], t)
            rt = max(np.abs(g["R"][t] - ref["R"]).max(), np.abs(g["t"][t] - ref["t"]).max())
            if rt > worst_rt:
                print("(R, t) difference", rt, "row", e["row"], e["camera"], "scene", e["scene"], "threshold", t)
            worst_rt = max(worst_rt, rt)
            compared += 1
    print("largest |R, t difference|:", worst_rt, "pose-error difference (deg):", worst_err, "band share:", worst_band,
          "compared:", compared)
    assert compared >= 0.9 * 6 * len(records)
    assert worst_band <= 0.01
    assert worst_rt <= 100 * rr.MEASURED_REDUCTION_SPREAD
    assert worst_err <= 1e-9


def test_properties(records):
    """4. errors against the true pose, R in SO(3), |t| = 1, E = [t]x R."""
    for r in records:
        e, g = r["entry"], r["gpu"]
        limit = 2 * (rr.MEASURED_MAX_POSE_ERROR[e["regime"]] if e["camera"] is None else rr.MEASURED_MAX_POSE_ERROR_CAMERA[e["camera"]])
        for t in range(len(r["ths"])):
            R, tv, E = g["R"][t], g["t"][t], g["E"][t]
            assert max(g["r_err"][t], g["t_err"][t]) <= limit, (e["row"], e["scene"], t)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
            assert abs(np.linalg.norm(tv) - 1) < 1e-12
            tx = np.array([[0, -tv[2], tv[1]], [tv[2], 0, -tv[0]], [-tv[1], tv[0], 0]])
            assert angle(E / np.linalg.norm(E), (tx @ R) / np.linalg.norm(tx @ R)) < 1e-12
            assert abs(np.linalg.norm(g["E_minimal"][t]) - 1) < 1e-12
            if outlier_free(e):
                assert (g["inliers"][t] == (e["case"]["m0"] > -1)).all()


def test_independent_of_batch_and_threshold_count(records):
    """5. bit-equal across the batch size (S = 8, 8, 4, 3, 1 ranges), alone vs in a batch, T = 6 vs six calls of T = 1."""
    pool = [e for e in rr.table_cases() if e["camera"] is None and e["regime"] == 3]
    cases, sids = [e["case"] for e in pool], [e["stream_id"] for e in pool]
    ths = rr.thresholds_for(pool[0])[1:3]
    ref = None
    for B in (1, 64, 128, 171, 512):
        pick = [j % len(pool) for j in range(B)]
        out = gpu_run([cases[j] for j in pick], ths, 2048, [sids[j] for j in pick])
        assert out["success"].all()
        first = {k: out[k][:len(pool)] for k in OUT_KEYS}
        if ref is None:
            alone = [gpu_run([cases[j]], ths, 2048, [sids[j]]) for j in range(len(pool))]
            ref = {k: np.concatenate([a[k] for a in alone]) for k in OUT_KEYS}
        assert same({k: v[:B] for k, v in ref.items()}, {k: v[:B] for k, v in first.items()}), B
        for j in range(B):  # every copy of a scene equals its first
            assert all(np.array_equal(out[k][j], out[k][pick[j]]) for k in OUT_KEYS), (B, j)
    ths6 = rr.thresholds_for(pool[0])
    all6 = gpu_run(cases, ths6, 512, sids)
    for t, th in enumerate(ths6):
        one = gpu_run(cases, [th], 512, sids)
        assert all(np.array_equal(one[k][:, 0], all6[k][:, t]) for k in OUT_KEYS), t


def test_records_beyond_the_lds_staging_limit():
    """5. M = 8200 (records read through L2) against the same matches in an M = 400 array."""
    case = rr.make_case(400, 0.5, 0.5, seed=4242)
    ths = [float(np.float32(t / rr.FOCAL)) for t in (1.0, 2.0)]
    small = gpu_run([case], ths, 256, [7])
    M = 8200
    big = dict(case)
    big["kp0"] = np.concatenate([case["kp0"], np.zeros((M - 400, 2), np.float32)])
    big["m0"] = np.concatenate([case["m0"], np.full(M - 400, -1, np.int64)])
    large = gpu_run([big], ths, 256, [7])
    assert small["success"].all()
    for k in OUT_KEYS:
        if k == "inliers":
            assert np.array_equal(large[k][..., :400], small[k]) and not large[k][..., 400:].any()
        else:
            assert np.array_equal(large[k], small[k]), k


def test_failures():
    """6. n = 0, n = 4, one repeated point, NaN key points fail cleanly; n = 5 succeeds."""
    five = rr.make_case(5, 0.0, 0.0, seed=9)
    M = 8
    pad = lambda a, fill: np.concatenate([a, np.full((M - len(a),) + a.shape[1:], fill, a.dtype)])  # noqa: E731
    base = {**five, "kp0": pad(five["kp0"], 0.25), "kp1": pad(five["kp1"], 0.5), "m0": pad(five["m0"], -1)}
    none = {**base, "m0": np.full(M, -1, np.int64)}
    four = {**base, "m0": base["m0"].copy()}
    four["m0"][np.nonzero(four["m0"] > -1)[0][0]] = -1
    repeated = {**base, "kp0": np.full((M, 2), 0.1, np.float32), "kp1": np.full((M, 2), 0.2, np.float32),
                "m0": np.arange(M, dtype=np.int64)}
    nans = {**base, "kp0": np.full((M, 2), np.nan, np.float32), "m0": np.arange(M, dtype=np.int64)}
    out = gpu_run([none, four, repeated, nans, base], [0.002, 0.004], 256, [0, 1, 2, 3, 4])
    for j in range(4):
        assert not out["success"][j].any(), j
        assert (out["R"][j] == np.eye(3)).all() and not out["t"][j].any() and not out["E"][j].any()
        assert not out["E_minimal"][j].any() and not out["inliers"][j].any() and not out["num_inliers"][j].any()
        assert (out["best_hypothesis"][j] == -1).all() and (out["best_solution"][j] == -1).all()
        assert np.isposinf(out["r_err"][j]).all() and np.isposinf(out["t_err"][j]).all()
    assert out["success"][4].all() and (out["num_inliers"][4] == 5).all()
    assert all(np.isfinite(out[k][4]).all() for k in ("R", "t", "E", "E_minimal", "r_err", "t_err"))
    # an empty key-point set
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    cam = geometry.Camera(torch.tensor([[0.0, 0, 1, 1, 0, 0]]))
    empty = eval_utils.relative_pose_ransac(z(1, 0, 2), z(1, 3, 2), torch.zeros((1, 0), dtype=torch.long, device="cuda"), cam,
                                            cam, [0.002], num_hypotheses=256)
    assert not empty["success"].any() and empty["inliers"].shape == (1, 1, 0) and (empty["best_hypothesis"] == -1).all()
    assert "r_err" not in empty


# ---- 7. interface ------------------------------------------------------------------------------------------------------
H, W = 96, 128


def to_cuda_item(item):
    return {"name": item["name"], "T_0to1": item["T_0to1"].cuda(),
            **{v: {"camera": item[v]["camera"].cuda()} for v in ("view0", "view1")}}


def test_named_estimator_and_estimator_object():
    items, preds = synthetic.posed_relief_pairs(2, H, W, seed=5, model="OPENCV_FISHEYE", num_keypoints=(70, 60))
    for it, p in zip(items, preds):
        item, pred = to_cuda_item(it), {k: v.cuda() for k, v in p.items()}
        named = eval_utils.eval_relative_pose_robust(item, pred, {"estimator": "gfc_amd", "ransac_th": 1.0})
        assert sorted(named) == ["ransac_inl", "ransac_inl%", "rel_pose_error"]
        assert np.isfinite(named["rel_pose_error"]) and 5 <= named["ransac_inl"] <= int((p["matches0"] > -1).sum())
        est = GpuRelativePoseEstimator({"ransac_th": 1.0})
        assert eval_utils.eval_relative_pose_robust(item, pred, {"estimator": "whatever", "ransac_th": 1.0}, estimator=est) == named
        sel = pred["matches0"] > -1
        got = est({"m_kpts0": pred["keypoints0"][sel], "m_kpts1": pred["keypoints1"][pred["matches0"][sel]],
                   "camera0": item["view0"]["camera"], "camera1": item["view1"]["camera"]})
        assert got["success"] and isinstance(got["M_0to1"], geometry.Pose) and got["inliers"].shape == (int(sel.sum()),)
        assert float(got["inliers"].sum()) == named["ransac_inl"]
    with pytest.raises(NotImplementedError, match="five-point"):
        eval_utils.eval_relative_pose_robust(item, pred, {"estimator": "opencv", "ransac_th": 1.0})
    with pytest.raises(ValueError):
        GpuRelativePoseEstimator({"options": {"confidence": 0.99}})


def test_pipeline_with_the_named_estimator(tmp_path):
    # eight pairs: three fisheye ones, then five pinhole ones with other key-point counts -> groups of equal shapes
    items_a, preds_a = synthetic.posed_relief_pairs(3, H, W, seed=11, model="OPENCV_FISHEYE", num_keypoints=(70, 60))
    items_b, preds_b = synthetic.posed_relief_pairs(5, H, W, seed=12, model="PINHOLE", num_keypoints=(52, 45))
    preds_b[4] = {**preds_b[4], "matches0": torch.where(torch.arange(52) < 3, preds_b[4]["matches0"], torch.tensor(-1))}
    items, preds = items_a + items_b, preds_a + preds_b
    pred_file = tmp_path / "predictions.npz"
    _write(pred_file, {it["name"][0]: {k: v.numpy() for k, v in p.items()} for it, p in zip(items, preds)})
    cuda_items = [to_cuda_item(it) for it in items]
    runs = {}
    for g in (2, 64):
        runs[g] = PosePairsPipeline({"estimator": "gfc_amd", "ransac_th": -1}, max_group=g).run_eval(cuda_items, pred_file)
    summaries, results = runs[2]
    assert sorted(results["pose_results"]) == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    for key in ("rel_pose_error@5°", "rel_pose_error@10°", "rel_pose_error@20°", "rel_pose_error_mAA"):
        assert 0.0 <= summaries[key] <= 1.0
    for key in ("rel_pose_error", "ransac_inl", "ransac_inl%"):
        assert len(results[key]) == 8
    assert str(runs[2]) == str(runs[64])  # NaN rows included
    # the pair with three matches gives NaN rows
    assert all(np.isnan(results["pose_results"][th]["rel_pose_error"][7]) for th in results["pose_results"])
    print("rel_pose_error at the best threshold:", results["rel_pose_error"], summaries["rel_pose_error_mAA"])
    # the per-pair object path: one estimator per pair and threshold, stream_id = the pair's position
    for th, lists in results["pose_results"].items():
        for i, (item, p) in enumerate(zip(cuda_items, preds)):
            if int((p["matches0"] > -1).sum()) < 5:
                continue
            est = GpuRelativePoseEstimator({"ransac_th": th, "options": {"stream_id": i}})
            want = eval_utils.eval_relative_pose_robust(item, {k: v.cuda() for k, v in p.items()},
                                                        {"estimator": "gfc_amd", "ransac_th": th}, estimator=est)
            assert {k: lists[k][i] for k in want} == want, (th, i)
    # the default eval_conf computes no pose
    _, plain = PosePairsPipeline({"ransac_th": -1}).run_eval(cuda_items, pred_file)
    assert "rel_pose_error" not in plain and "pose_results" not in plain
