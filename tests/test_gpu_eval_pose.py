"""The pose / depth evaluation kernels (csrc/eval_pose.hip through eval_utils and eval_pose_pairs) on the GPU.

Against the fixture the reference produced (tests/golden/pose_depth.npz; test_pose_reference_host.py shows that no value
in it lies within a rounding error of a decision, so nothing is excused here): masks and ground-truth matches exactly,
counts exactly, ratios to 1e-6 (covisible_percent is a ratio times 100: compared as the ratio), relative_pose_error to
1e-4 degrees.  Against tests/pose_reference.py on the CPU with the same inputs: the edge shapes.

Float tolerance of `proj` and `depth_kp`: not a fixed number.  The fixture holds the reference's float32 result and its
float64 result on the same inputs; per camera model, the largest difference of the two is the reference's own float32
error E, and the kernel may differ from float64 by at most max(4 E, 1e-4) (pixels for `proj`, depth units for
`depth_kp`) -- another, equally valid float32 operation order must pass, the fisheye Newton iteration and tan included.
E is taken over the projections inside a 4096-pixel box: the few beyond it (a point behind the camera divides by the
1e-4 floor) carry float32 errors proportional to their size and are held to 1e-5 of it instead.  The measured figures go
to profiles/pose_eval_parity.json when GFC_WRITE_PROFILES=1.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_reference as pr  # noqa: E402

from glue_factory_colon_amd import eval_utils, geometry, synthetic  # noqa: E402
from glue_factory_colon_amd.eval_pose_pairs import PosePairsPipeline  # noqa: E402
from glue_factory_colon_amd.export_predictions import _write  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_depth.npz")
CASES = (0, 1, 2)
BOX = 4096.0
WIDTH = {"PINHOLE": 6, "RADIAL": 8, "OPENCV": 10, "OPENCV_FISHEYE": 10}
_parity = {}


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def camera(data, model):
    return geometry.Camera(data[..., :WIDTH[model]].contiguous(), model=model)


def case_dev(fx, c):
    t = lambda k, dt=torch.float32: torch.from_numpy(fx[k][c:c + 1]).to(device="cuda", dtype=dt)  # noqa: E731
    model = str(fx["models"][c])
    return dict(kp0=t("kp0"), kp1=t("kp1"), m0=t("matches0", torch.long), depth0=t("depth0"), depth1=t("depth1"),
                cam0=camera(t("cam0"), model), cam1=camera(t("cam1"), model), T=geometry.Pose(t("T_0to1")), model=model)


def deviation(value, f64):
    """(largest |value - f64| inside the box, largest relative one beyond it); the NaN patterns must agree."""
    value, f64 = np.asarray(value, dtype=np.float64), np.asarray(f64, dtype=np.float64)
    assert np.array_equal(np.isnan(value), np.isnan(f64))
    fin = np.isfinite(f64)
    assert np.array_equal(np.isfinite(value), fin)
    inside = fin & (np.abs(f64) <= BOX)
    far = fin & ~inside
    d_in = float(np.abs(value[inside] - f64[inside]).max()) if inside.any() else 0.0
    d_far = float((np.abs(value[far] - f64[far]) / np.abs(f64[far])).max()) if far.any() else 0.0
    return d_in, d_far


@pytest.mark.parametrize("c", CASES)
def test_pose_project_against_the_fixture(fx, c):
    a = case_dev(fx, c)
    T10 = geometry.Pose(torch.from_numpy(fx["T_1to0"][c:c + 1]).cuda())
    record = {}
    for tag, kp, depth, ci, cj, T, side in (("0to1", a["kp0"], a["depth0"], a["cam0"], a["cam1"], a["T"], "0"),
                                            ("1to0", a["kp1"], a["depth1"], a["cam1"], a["cam0"], T10, "1")):
        d, valid, proj, visible = eval_utils.pose_project(kp, depth, ci, cj, T)
        torch.cuda.synchronize()
        assert np.array_equal(valid[0].cpu().numpy(), fx["valid" + side][c])
        assert np.array_equal(visible[0].cpu().numpy(), fx["visible" + side][c])
        for name, mine, key in (("depth_kp", d, "depth_kp" + side), ("proj", proj, "proj_" + tag)):
            ref_in, _ = deviation(fx[key][c], fx[key + "_f64"][c])
            got_in, got_far = deviation(mine[0].cpu().numpy(), fx[key + "_f64"][c])
            bound = max(4 * ref_in, 1e-4)
            record[f"{name}_{tag}"] = {"reference_f32_vs_f64": ref_in, "kernel_vs_f64": got_in, "bound": bound,
                                       "kernel_vs_f64_relative_beyond_4096px": got_far}
            print(a["model"], name, tag, record[f"{name}_{tag}"])
            assert got_in <= bound and got_far <= 1e-5, (name, tag, got_in, bound, got_far)
    _parity[a["model"]] = record
    if os.environ.get("GFC_WRITE_PROFILES") == "1" and len(_parity) == len(CASES):
        with open(os.path.join(ROOT, "profiles", "pose_eval_parity.json"), "w") as f:
            json.dump({"what": "largest absolute difference to the reference's float64 evaluation of the fixture "
                               "(tests/golden/pose_depth.npz), per camera model: the reference's own float32 result and "
                               "gfc_eval_pose_project; pixels for proj, depth units for depth_kp",
                       "device": torch.cuda.get_device_name(0), "models": _parity}, f, indent=1)


def ratios_close(got, want):
    """[.., 7] or [.., 5] rows: every entry is a ratio in [0, 1] or a count except covisible_percent (ratio x 100)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.ones(got.shape[-1])
    if got.shape[-1] == 7:
        scale[4] = 100.0
    return float(np.abs((got - want) / scale).max()) <= 1e-6


@pytest.mark.parametrize("c", CASES)
def test_metrics_and_gt_matches_against_the_fixture(fx, c):
    a = case_dev(fx, c)
    out, g0, g1 = eval_utils.pose_depth_metrics(a["kp0"], a["kp1"], a["m0"], a["depth0"], a["depth1"], a["cam0"], a["cam1"],
                                                a["T"], return_gt=True)
    epi = eval_utils.pose_epipolar_metrics(a["kp0"], a["kp1"], a["m0"], a["cam0"], a["cam1"], a["T"])
    torch.cuda.synchronize()
    assert torch.equal(g0[0].cpu(), torch.from_numpy(fx["gt_matches0"][c]))
    assert torch.equal(g1[0].cpu(), torch.from_numpy(fx["gt_matches1"][c]))
    out, epi = out[0].cpu().numpy(), epi[0].cpu().numpy()
    print(a["model"], out.tolist(), fx["metrics7"][c].tolist(), epi.tolist(), fx["metrics5"][c].tolist())
    assert out[3] == fx["metrics7"][c][3] and epi[3] == fx["metrics5"][c][3] and epi[4] == fx["metrics5"][c][4]
    assert ratios_close(out, fx["metrics7"][c]) and ratios_close(epi, fx["metrics5"][c])
    # the dictionary form of the ground truth: same arrays, and no M x N matrix among them
    gt = eval_utils.gt_matches_from_pose_depth(a["kp0"], a["kp1"], {"view0": {"camera": a["cam0"], "depth": a["depth0"]},
                                                                   "view1": {"camera": a["cam1"], "depth": a["depth1"]},
                                                                   "T_0to1": a["T"]}, pos_th=3, neg_th=5)
    assert sorted(gt) == sorted(["matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0",
                                 "depth_keypoints1", "proj_0to1", "proj_1to0", "visible0", "visible1"])
    assert torch.equal(gt["matches0"], g0) and torch.equal(gt["matches1"], g1)
    assert np.array_equal(gt["visible0"][0].cpu().numpy(), fx["visible0"][c])
    assert torch.equal(gt["matching_scores1"], (g1 > -1).float())


def test_relative_pose_error_against_the_fixture(fx):
    for c in CASES:
        T = geometry.Pose(torch.from_numpy(fx["T_0to1"][c:c + 1]).cuda())
        for R, t, want in zip(fx["R_est"][c], fx["t_est"][c], fx["pose_err"][c]):
            t_err, r_err = eval_utils.relative_pose_error(T, torch.from_numpy(R).cuda(), torch.from_numpy(t).cuda())
            assert abs(float(t_err) - want[0]) < 1e-4 and abs(float(r_err) - want[1]) < 1e-4, (t_err, r_err, want)


# ---- edge shapes against the torch checker on the CPU ---------------------------------------------------------------
H, W, M, N = 48, 64, 70, 45


@pytest.fixture(scope="module")
def scenes():
    """Five pairs per model, 48 x 64 maps, 70 + 45 key points: (items, preds) of synthetic.posed_plane_pairs."""
    return {model: synthetic.posed_plane_pairs(5, H, W, seed=11, model=model, num_keypoints=(M, N)) for model in pr.MODELS}


def batch_of(items, preds, idx):
    model = items[0]["view0"]["camera"].model
    cat = lambda f: torch.cat([f(items[i]) for i in idx])  # noqa: E731
    return dict(kp0=torch.stack([preds[i]["keypoints0"] for i in idx]), kp1=torch.stack([preds[i]["keypoints1"] for i in idx]),
                m0=torch.stack([preds[i]["matches0"] for i in idx]), depth0=cat(lambda it: it["view0"]["depth"]),
                depth1=cat(lambda it: it["view1"]["depth"]), cam0=cat(lambda it: it["view0"]["camera"]._data),
                cam1=cat(lambda it: it["view1"]["camera"]._data), T=cat(lambda it: it["T_0to1"]._data), model=model)


def run_gpu(b):
    cam0, cam1 = camera(b["cam0"].cuda(), b["model"]), camera(b["cam1"].cuda(), b["model"])
    T = geometry.Pose(b["T"].cuda())
    out, g0, g1 = eval_utils.pose_depth_metrics(b["kp0"].cuda(), b["kp1"].cuda(), b["m0"].cuda(), b["depth0"].cuda(),
                                                b["depth1"].cuda(), cam0, cam1, T, return_gt=True)
    epi = eval_utils.pose_epipolar_metrics(b["kp0"].cuda(), b["kp1"].cuda(), b["m0"].cuda(), cam0, cam1, T)
    torch.cuda.synchronize()
    return out.cpu(), g0.cpu(), g1.cpu(), epi.cpu()


def run_cpu(b):
    m7, g0, g1 = pr.depth_metrics(b["kp0"], b["kp1"], b["m0"], b["depth0"], b["depth1"], b["cam0"], b["model"], b["cam1"],
                                  b["model"], b["T"])
    m5 = pr.epipolar_metrics(b["kp0"], b["kp1"], b["m0"], b["cam0"], b["model"], b["cam1"], b["model"], b["T"])
    return m7, g0, g1, m5


def assert_same(gpu, cpu):
    out, g0, g1, epi = gpu
    m7, c0, c1, m5 = cpu
    assert torch.equal(g0, c0) and torch.equal(g1, c1)
    assert torch.equal(out[:, 3].double(), m7[:, 3]) and torch.equal(epi[:, 3:].double(), m5[:, 3:])
    assert ratios_close(out.numpy(), m7.numpy()) and ratios_close(epi.numpy(), m5.numpy()), (out, m7, epi, m5)


@pytest.mark.parametrize("model", pr.MODELS)
def test_every_model_against_the_checker(scenes, model):
    """All four camera models (the fixture has three), B = 5 in one call."""
    b = batch_of(*scenes[model], range(5))
    gpu = run_gpu(b)
    assert_same(gpu, run_cpu(b))
    assert (gpu[1] > -1).any() and (gpu[1] == -1).any() and (gpu[1] == -2).any()


@pytest.mark.parametrize("edge", ["M0", "N0", "no_matches", "depth_invalid"])
def test_edge_shapes(scenes, edge):
    b = batch_of(*scenes["OPENCV_FISHEYE"], range(2))
    if edge == "M0":
        b.update(kp0=b["kp0"][:, :0], m0=b["m0"][:, :0])
    elif edge == "N0":
        b.update(kp1=b["kp1"][:, :0], m0=torch.full_like(b["m0"], -1))
    elif edge == "no_matches":
        b.update(m0=torch.full_like(b["m0"], -1))
    else:
        b.update(depth0=torch.zeros_like(b["depth0"]), depth1=-torch.ones_like(b["depth1"]))
    gpu = run_gpu(b)
    assert_same(gpu, run_cpu(b))
    out, g0, g1, epi = gpu
    if edge in ("M0", "N0"):
        assert (g0 == -1).all() and (g1 == -1).all() and (out == 0).all()
    if edge == "no_matches":
        assert (out[:, :5] == 0).all() and (out[:, 6] == 0).all() and (epi[:, :4] == 0).all()
    if edge == "depth_invalid":
        assert (g0 == -2).all() and (g1 == -2).all() and (out[:, 3] == 0).all()


def test_batch_of_five_equals_five_single_calls(scenes):
    b = batch_of(*scenes["OPENCV"], range(5))
    whole = run_gpu(b)
    d, valid, proj, vis = eval_utils.pose_project(b["kp0"].cuda(), b["depth0"].cuda(), camera(b["cam0"].cuda(), b["model"]),
                                                  camera(b["cam1"].cuda(), b["model"]), geometry.Pose(b["T"].cuda()))
    for i in range(5):
        one_b = batch_of(*scenes["OPENCV"], [i])
        one = run_gpu(one_b)
        for x, y in zip(whole, one):
            assert torch.equal(x[i:i + 1], y)  # bit for bit
        d1, valid1, proj1, vis1 = eval_utils.pose_project(one_b["kp0"].cuda(), one_b["depth0"].cuda(),
                                                          camera(one_b["cam0"].cuda(), b["model"]),
                                                          camera(one_b["cam1"].cuda(), b["model"]), geometry.Pose(one_b["T"].cuda()))
        same = lambda u, v: torch.equal(torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0))  # noqa: E731
        assert same(d[i:i + 1], d1) and same(proj[i:i + 1], proj1) and torch.equal(valid[i:i + 1], valid1) and torch.equal(vis[i:i + 1], vis1)


def to_cuda_item(item):
    return {"name": item["name"], "T_0to1": item["T_0to1"].cuda(),
            **{v: {"camera": item[v]["camera"].cuda(), "depth": item[v]["depth"].cuda()} for v in ("view0", "view1")}}


def test_drop_in_dict_forms(scenes):
    items, preds = scenes["RADIAL"]
    b = batch_of(items, preds, range(3))
    out, _, _, epi = run_gpu(b)
    # un-batched: a loader item of batch 1 and the un-batched cached record -> scalars
    for i in range(3):
        pred = {k: v.cuda() for k, v in preds[i].items()}
        res = {**eval_utils.eval_matches_epipolar(to_cuda_item(items[i]), pred), **eval_utils.eval_matches_depth(to_cuda_item(items[i]), pred)}
        assert list(res) == [*eval_utils.EPIPOLAR_RESULT_KEYS, *eval_utils.DEPTH_RESULT_KEYS]
        assert isinstance(res["num_matches"], int) and isinstance(res["reproj_prec@3px"], float)
        assert [res[k] for k in eval_utils.DEPTH_RESULT_KEYS] == out[i].tolist()
        assert [float(res[k]) for k in eval_utils.EPIPOLAR_RESULT_KEYS] == epi[i].tolist()
    # batched -> lists per item
    data = {"T_0to1": geometry.Pose(b["T"].cuda()),
            "view0": {"camera": camera(b["cam0"].cuda(), "RADIAL"), "depth": b["depth0"].cuda()},
            "view1": {"camera": camera(b["cam1"].cuda(), "RADIAL"), "depth": b["depth1"].cuda()}}
    pred = {"keypoints0": b["kp0"].cuda(), "keypoints1": b["kp1"].cuda(), "matches0": b["m0"].cuda(),
            "matching_scores0": (b["m0"] > -1).float().cuda()}
    res = eval_utils.eval_matches_depth(data, pred)
    assert all(res[k] == out[:, j].tolist() for j, k in enumerate(eval_utils.DEPTH_RESULT_KEYS))
    res = eval_utils.eval_matches_epipolar(data, pred)
    assert res["num_matches"] == [int(v) for v in epi[:, 3].tolist()] and res["epi_prec@1e-3"] == epi[:, 2].tolist()


class TruePose:
    """An estimator object of the reference's interface that answers with the true pose of the pair it is asked about."""

    def __init__(self):
        self.truth, self.calls = None, []

    def __call__(self, data):
        assert sorted(data) == ["camera0", "camera1", "m_kpts0", "m_kpts1"] and data["camera0"]._data.ndim == 1
        assert data["m_kpts0"].shape == data["m_kpts1"].shape and data["m_kpts0"].shape[1] == 2
        self.calls.append(len(data["m_kpts0"]))
        return {"success": True, "M_0to1": self.truth, "inliers": torch.ones(len(data["m_kpts0"]), dtype=torch.bool)}


def test_pipeline_on_eight_pairs(scenes, tmp_path):
    # eight pairs: three fisheye ones, then five pinhole ones with other key-point counts -> groups of equal shapes
    items_a, preds_a = scenes["OPENCV_FISHEYE"]
    items_b, preds_b = synthetic.posed_plane_pairs(5, H, W, seed=12, model="PINHOLE", num_keypoints=(52, 45))
    items, preds = items_a[:3] + items_b, preds_a[:3] + preds_b
    pred_file = tmp_path / "predictions.npz"
    _write(pred_file, {it["name"][0]: {k: v.numpy() for k, v in p.items()} for it, p in zip(items, preds)})
    pipe = PosePairsPipeline({"ransac_th": -1}, max_group=2)
    summaries, results = pipe.run_eval([to_cuda_item(it) for it in items], pred_file)
    assert results["names"] == [it["name"][0] for it in items]
    for i, (it, p) in enumerate(zip(items, preds)):
        pred = {k: v.cuda() for k, v in p.items()}
        want = {**eval_utils.eval_matches_epipolar(to_cuda_item(it), pred), **eval_utils.eval_matches_depth(to_cuda_item(it), pred)}
        for k, v in want.items():
            assert results[k][i] == v, (i, k)
    assert summaries["mean_num_matches"] == round(float(np.mean(results["num_matches"])), 3)
    assert summaries["med_reproj_prec@3px"] == round(float(np.median(results["reproj_prec@3px"])), 3)
    assert "rel_pose_error" not in results
    # without depth the depth metrics are not computed, as in the reference
    bare = [{"name": it["name"], "T_0to1": it["T_0to1"].cuda(), "view0": {"camera": it["view0"]["camera"].cuda()},
             "view1": {"camera": it["view1"]["camera"].cuda()}} for it in items[:2]]
    _, res = pipe.run_eval(bare, pred_file)
    assert "reproj_prec@3px" not in res and len(res["epi_prec@1e-3"]) == 2
    # a stub estimator that returns the true pose
    est = TruePose()

    def with_truth():
        for it in items:
            est.truth = it["T_0to1"]
            yield to_cuda_item(it)

    summaries, results = pipe.run_eval(with_truth(), pred_file, estimator=est)
    assert len(est.calls) == 8 * 6 and len(results["rel_pose_error"]) == 8
    print("rel_pose_error of the true pose:", results["rel_pose_error"])
    assert max(results["rel_pose_error"]) < 1e-3
    assert summaries["rel_pose_error@5°"] > 0.99 and summaries["rel_pose_error_mAA"] > 0.99
    assert results["ransac_inl%"] == [1.0] * 8 and sorted(results["pose_results"]) == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    with pytest.raises(NotImplementedError, match="five-point"):
        eval_utils.eval_relative_pose_robust(to_cuda_item(items[0]), {k: v.cuda() for k, v in preds[0].items()},
                                             {"estimator": "poselib", "ransac_th": 1.0})


# ---- the depth kernel on its large path: above 64 KB of LDS, the evaluation's 2048 x 2048, and the LDS limit -------------
# One workgroup keeps every key point of a pair in LDS: 24 M + 28 N bytes of dynamic arrays beside the kernel's static
# ones.  The fixture and the scenes above stay below 4 KB; these scenes (240 x 320 maps) are the first shape above
# 64 KB, the evaluation's shape, and the largest shape the launcher admits -- the next one up is refused before any launch.
# Checker: pose_reference in float64.  Only what pose_reference.undecided flags is exempt (its own undecidable rules, per
# key point), and every scene asserts on the CPU side, before the kernel's answer is looked at, that at most 1 % of the
# key points of either view and at most 1 % of the matches are flagged.
BIG_H, BIG_W, LDS_LIMIT, CAP = 240, 320, 160 * 1024, 0.01


def largest_admitted_depth(m):
    lds_bytes = eval_utils.nat.lib().gfc_eval_matches_depth_lds_bytes
    n = 0
    while lds_bytes(m, n + 1) <= LDS_LIMIT:
        n += 1
    return n


def check_large(model, m, n, b, seed):
    items, preds = synthetic.posed_plane_pairs(b, BIG_H, BIG_W, seed=seed, model=model, num_keypoints=(m, n))
    bt = batch_of(items, preds, range(b))
    T10 = torch.stack([pr.invert_pose(t.double()) for t in bt["T"]])
    dbl = {k: v.double() for k, v in bt.items() if k not in ("m0", "model")}
    flags = [pr.undecided(bt["kp0"][i], bt["kp1"][i], bt["m0"][i], bt["depth0"][i], bt["depth1"][i], bt["cam0"][i], model,
                          bt["cam1"][i], model, bt["T"][i]) for i in range(b)]
    for f, m0 in zip(flags, bt["m0"]):  # the condition on the input
        shares = (float(f["undecided0"].float().mean()), float(f["undecided1"].float().mean()),
                  float(f["undecided_match"].sum()) / max(int((m0 > -1).sum()), 1))
        print(model, (m, n), "undecided shares", shares)
        assert max(shares) <= CAP, ("bad input: too many undecided", shares)
    m7, c0, c1 = pr.depth_metrics(dbl["kp0"], dbl["kp1"], bt["m0"], dbl["depth0"], dbl["depth1"], dbl["cam0"], model,
                                  dbl["cam1"], model, dbl["T"], T10)
    out, g0, g1, _ = run_gpu(bt)
    out = out.double()
    for i, f in enumerate(flags):
        s0, s1 = ~f["undecided0"], ~f["undecided1"]
        assert torch.equal(g0[i][s0], c0[i][s0]), (i, torch.nonzero((g0[i] != c0[i]) & s0).flatten()[:10])
        assert torch.equal(g1[i][s1], c1[i][s1]), (i, torch.nonzero((g1[i] != c1[i]) & s1).flatten()[:10])
        assert (c0[i] > -1).any() and (c0[i] == -1).any() and (c0[i] == -2).any()
        m0 = bt["m0"][i]
        err, valid = pr.reprojection_errors(dbl["kp0"][i], dbl["kp1"][i], m0, dbl["depth0"][i], dbl["depth1"][i],
                                            dbl["cam0"][i], model, dbl["cam1"][i], model, dbl["T"][i], T10[i])
        und = f["undecided_match"][m0 > -1]
        n_und, nm = int(und.sum()), int((m0 > -1).sum())
        nv = float(out[i, 3])
        sure_valid = int((valid & ~und).sum())
        assert nv == round(nv) and sure_valid <= nv <= sure_valid + n_und, (i, nv, sure_valid, n_und)
        assert abs(float(out[i, 4]) / 100.0 - nv / nm) <= 1e-6
        e = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        for col, th in ((0, 1.0), (1, 3.0), (2, 5.0)):
            sure_true = int((valid & ~und & (e < th)).sum())
            k = round(float(out[i, col]) * nv)
            assert sure_true <= k <= sure_true + n_und, (i, th, k, sure_true, n_und)
            assert abs(float(out[i, col]) - k / nv) <= 1e-6
        # recall and precision from the kernel's OWN ground truth: the reduction, pinned apart from the verdicts
        agree, rec, prec = m0 == g0[i], g0[i] > -1, (m0 > -1) & (g0[i] >= -1)
        assert abs(float(out[i, 5]) - float((agree & rec).sum()) / (1e-8 + float(rec.sum()))) <= 1e-6
        assert abs(float(out[i, 6]) - float((agree & prec).sum()) / (1e-8 + float(prec.sum()))) <= 1e-6


@pytest.mark.parametrize("model,m,n,b,seed", [("PINHOLE", 1300, 1250, 1, 21), ("OPENCV_FISHEYE", 1300, 1250, 1, 21),
                                               ("PINHOLE", 2048, 2048, 2, 22)])
def test_depth_metrics_above_64_kb_of_lds(model, m, n, b, seed):
    lds_bytes = eval_utils.nat.lib().gfc_eval_matches_depth_lds_bytes
    assert lds_bytes(m, n) > 64 * 1024 >= lds_bytes(1250, 1250)  # 1300 x 1250 is just above, 1250 x 1250 below
    check_large(model, m, n, b, seed)


def test_depth_metrics_largest_admitted_shape_and_the_next_one_refused():
    m = 3150
    n = largest_admitted_depth(m)
    lds_bytes = eval_utils.nat.lib().gfc_eval_matches_depth_lds_bytes
    assert n >= 3100 and lds_bytes(m, n) <= LDS_LIMIT < lds_bytes(m, n + 1)
    check_large("PINHOLE", m, n, 1, 23)
    # one more key point: refused by the launcher's own arithmetic, nothing is launched
    items, preds = synthetic.posed_plane_pairs(1, BIG_H, BIG_W, seed=23, model="PINHOLE", num_keypoints=(m, n + 1))
    with pytest.raises(eval_utils.nat.NativeError, match="UNSUPPORTED"):
        run_gpu(batch_of(items, preds, range(1)))
