"""The GPU RANSAC homography estimator (csrc/ransac.hip through eval_utils.homography_ransac) against the float64
restatement of its algorithm (tests/ransac_reference.py) and against properties that need no reference.  Parity with
OpenCV's / PoseLib's estimators is NOT tested: both are randomised CPU libraries that are not available here.

Inputs: the seeded regimes of ransac_reference.TABLE (640 x 480, M = N = n key points, 10 % of the rows unmatched),
two scenes each, thresholds [0.5, 1, 3] and the six-threshold sweep.  All scenes of one (M, N) shape go through ONE
batched call -- except that the two n = 1000 rows ask for different numbers of hypotheses (1024 / 2048), which is one
argument of a call, so they are two calls of two scenes.

delta = 2e-3 px is the bound on an fp32 projection of coordinates below 4096 (a handful of roundings of
2^-24 * 4096 = 2.4e-4 px); the kernel scores in fp64, so it holds with room."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_reference as rr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import eval_utils  # noqa: E402

pytestmark = pytest.mark.gpu
DELTA = 2e-3
THRESHOLD_SETS = {"three": [0.5, 1.0, 3.0], "sweep": rr.SWEEP}
OUT_KEYS = ("H", "inliers", "num_inliers", "success", "best_hypothesis", "H_minimal", "error")


def to_dev(cases):
    def st(key, dtype):
        return torch.from_numpy(np.stack([c[key] for c in cases])).to(device="cuda", dtype=dtype)

    return st("H_gt", torch.float32), st("kp0", torch.float32), st("kp1", torch.float32), st("m0", torch.long), st("size", torch.float32)


def gpu_run(cases, ths, hyp, sids, seed=0, lo_iters=3):
    H, kp0, kp1, m0, size = to_dev(cases)
    out = eval_utils.homography_ransac(H, kp0, kp1, m0, size, ths, num_hypotheses=hyp, lo_iters=lo_iters, seed=seed,
                                       stream_id=sids)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def records():
    """One record per (scene, threshold set): the GPU's outputs for the scene [T, ...] and the restatement's."""
    table = rr.table_cases()
    groups = {}
    for r, k, c, hyp in table:
        groups.setdefault((len(c["kp0"]), hyp), []).append((r, k, c))
    recs = []
    for name, ths in THRESHOLD_SETS.items():
        for (n, hyp), members in groups.items():
            recs += make_records(members, ths, hyp, [100 * r + k for r, k, _ in members])
    return recs


def band(H, corr, t):
    """correspondences whose residual under H is within delta of the threshold"""
    return np.abs(np.sqrt(rr.residual2(H, corr)[0]) - t) < DELTA


def test_sampler_through_the_kernel(records):
    """1. H_minimal is the float64 solve through ransac_sample_indices(...)[best_hypothesis]."""
    checked = 0
    for rec in records:
        if rr.TABLE[rec["row"]][1] == 0:
            continue  # rows with outliers: there the winner says something about the sample
        samples = eval_utils.ransac_sample_indices(0, rec["sid"], len(rec["corr"]), rec["hyp"])
        for t in range(len(rec["ths"])):
            h = int(rec["gpu"]["best_hypothesis"][t])
            assert 0 <= h < rec["hyp"]
            p = rec["corr"][samples[h]][None]
            H64, ok = rr.homography_4pt(p[:, :, 0], p[:, :, 1], p[:, :, 2], p[:, :, 3])
            assert ok[0]
            d = np.abs(rr.corners(rec["gpu"]["H_minimal"][t], rec["case"]["size"]) - rr.corners(H64[0], rec["case"]["size"])).max()
            assert d < 1e-3, (rec["row"], rec["scene"], t, d)
            checked += 1
    assert checked == 8 * 9


def compare_with_restatement(rec, stats):
    """Conditions 2 and 3 for one record (one scene, all its thresholds); returns (cases, flips)."""
    n = len(rec["corr"])
    cases = flips = 0
    for t, th in enumerate(rec["ths"]):
        g, ref = rec["gpu"], rec["ref"][t]
        assert g["success"][t] and ref["success"]
        h = int(g["best_hypothesis"][t])
        assert 0 <= h < rec["hyp"]
        gap = ref["scores"][h] - ref["scores"].min()
        stats["gap"] = max(stats["gap"], gap / (2 * th * DELTA * n))
        assert gap <= 2 * th * DELTA * n, (rec["row"], rec["scene"], th, gap)
        assert int(g["num_inliers"][t]) == int(g["inliers"][t].sum())
        cases += 1
        if h != ref["best_hypothesis"]:
            flips += 1
            continue
        inside = np.zeros(len(rec["case"]["kp0"]), bool)
        inside[rec["idx"]] = band(ref["H"], rec["corr"], th)
        stats["band"] = max(stats["band"], inside.sum() / n)
        assert inside.sum() <= 0.01 * n, (rec["row"], rec["scene"], th, inside.sum())
        assert np.array_equal(g["inliers"][t][~inside], ref["inliers"][~inside]), (rec["row"], rec["scene"], th)
        diff = abs(float(g["error"][t]) - ref["error"])
        stats["err"] = max(stats["err"], diff)
        assert diff <= 2e-2 + 2e-3 * ref["error"], (rec["row"], rec["scene"], th, float(g["error"][t]), ref["error"])
    return cases, flips


def make_records(members, ths, hyp, sids):
    """One batched GPU call for `members` [(row, scene, case)] + the restatement of every scene."""
    out = gpu_run([c for _, _, c in members], ths, hyp, sids)
    out = {key: out[key].cpu().numpy() for key in OUT_KEYS}
    recs = []
    for j, (r, k, c) in enumerate(members):
        ref = rr.ransac(c["kp0"], c["kp1"], c["m0"], ths, hyp, 3, 0, sids[j], c["H_gt"], c["size"])
        corr, idx = rr.correspondences(c["kp0"], c["kp1"], c["m0"])
        recs.append({"row": r, "scene": k, "case": c, "hyp": hyp, "sid": sids[j], "ths": ths,
                     "gpu": {key: v[j] for key, v in out.items()}, "ref": ref, "corr": corr, "idx": idx})
    return recs


def test_selection_and_agreement_with_the_restatement(records):
    """2. the float64 score of the GPU's winner is within 2 t delta n of the best float64 score;  3. flips (another
    winner than the restatement's) in <= 10 % of the cases; elsewhere the same inliers outside the band, a band of
    <= 1 % of the correspondences, and the corner error within 2e-2 + 2e-3 err of the restatement's."""
    cases = flips = 0
    stats = {"gap": 0.0, "band": 0.0, "err": 0.0}
    for rec in records:
        c, f = compare_with_restatement(rec, stats)
        cases, flips = cases + c, flips + f
    print(f"cases {cases}, flips {flips}, worst score gap / bound {stats['gap']:.3g}, worst band share {stats['band']:.3g}, "
          f"worst corner-error difference {stats['err']:.3g} px")
    assert cases == 10 * 9 and flips <= 0.10 * cases, (flips, cases)


def test_hypothesis_counts_that_do_not_fill_the_lanes():
    """Hypothesis counts that are no multiple of the 256 lanes of a workgroup (several passes per lane, the last one
    with idle lanes; ranges of unequal length when a pair's hypotheses are split): conditions 2 and 3 again."""
    members = [(r, k, c) for r, k, c, _ in rr.table_cases() if r == 3]
    cases = flips = 0
    stats = {"gap": 0.0, "band": 0.0, "err": 0.0}
    for hyp in (257, 300, 1000, 2047):
        for rec in make_records(members, [1.0, 3.0], hyp, [41, 42]):
            c, f = compare_with_restatement(rec, stats)
            cases, flips = cases + c, flips + f
    print(f"odd counts: cases {cases}, flips {flips}, worst score gap / bound {stats['gap']:.3g}")
    assert cases == 16 and flips <= 0.10 * cases, (flips, cases)


def test_many_key_points():
    """The two other ways the scoring kernel holds the correspondences: more than 64 KB of LDS (4096 < M <= 8192) and,
    beyond what fits (M > 8192), reads through L2.  30 % outliers, sigma 0.5 px, 512 hypotheses, two scenes each."""
    cases = flips = 0
    stats = {"gap": 0.0, "band": 0.0, "err": 0.0}
    for m in (5000, 9000):
        members = [(m, k, rr.make_case(m, 0.3, 0.5, seed=7000 + m + k)) for k in range(2)]
        for rec in make_records(members, [1.0, 3.0], 512, [m, m + 1]):
            c, f = compare_with_restatement(rec, stats)
            cases, flips = cases + c, flips + f
    print(f"large M: cases {cases}, flips {flips}, worst corner-error difference {stats['err']:.3g} px")
    assert cases == 8 and flips <= 0.10 * cases, (flips, cases)


def test_every_match_valid_around_one_chunk_of_the_compaction():
    """No row unmatched, M one short of, equal to and one over the 256 rows the compaction takes per step: every row is a
    correspondence, in its own order (the inlier masks are compared by row).  30 % outliers, sigma 0.5 px, 512
    hypotheses, two scenes each: conditions 2 and 3 again."""
    cases = flips = 0
    stats = {"gap": 0.0, "band": 0.0, "err": 0.0}
    for m in (255, 256, 257):
        members = [(m, k, rr.make_case(m, 0.3, 0.5, seed=8000 + m + k, unmatched_share=0.0)) for k in range(2)]
        for rec in make_records(members, [1.0, 3.0], 512, [m, m + 1]):
            assert len(rec["corr"]) == m and np.array_equal(rec["idx"], np.arange(m))
            c, f = compare_with_restatement(rec, stats)
            cases, flips = cases + c, flips + f
    print(f"every match valid: cases {cases}, flips {flips}, worst score gap / bound {stats['gap']:.3g}")
    assert cases == 12 and flips <= 0.10 * cases, (flips, cases)


def test_self_consistency(records):
    """4. no reference involved: inliers == {r^2 < t^2} of the returned H outside the band; the returned model's MSAC
    score is not above H_minimal's (both recomputed in float64 from the fp64 models the kernel returns)."""
    for rec in records:
        for t, th in enumerate(rec["ths"]):
            g = rec["gpu"]
            t2 = float(np.float32(th)) ** 2
            r2 = rr.residual2(g["H"][t], rec["corr"])[0]
            keep = ~band(g["H"][t], rec["corr"], th)
            assert np.array_equal(g["inliers"][t][rec["idx"]][keep], (r2 < t2)[keep])
            assert not g["inliers"][t][rec["case"]["m0"] < 0].any()
            s_final = rr.msac(rr.residual2(g["H"][t], rec["corr"]), t2)[0]
            s_min = rr.msac(rr.residual2(g["H_minimal"][t], rec["corr"]), t2)[0]
            assert s_final <= s_min, (rec["row"], rec["scene"], th, s_final, s_min)
            assert abs(g["H"][t][2, 2] - 1.0) < 1e-12 and float(g["error"][t]) <= rr.error_bound(rr.TABLE[rec["row"]][2], th)


def test_determinism_and_invariance():
    """5. two calls are equal bit for bit; a pair alone (B = 1: its hypotheses split over several workgroups) gives what
    it gives inside a batch, given the same stream_id; another seed picks other samples, the error stays bounded."""
    cases = [c for r, _, c, _ in rr.table_cases() if r in (3, 4)]  # the four n = 1000 scenes
    rows = [r for r, _, _, _ in rr.table_cases() if r in (3, 4)]
    sids = [7, 1 << 40, 3, 12345]
    a = gpu_run(cases, rr.SWEEP, 2048, sids)
    b = gpu_run(cases, rr.SWEEP, 2048, sids)
    for key in OUT_KEYS:
        assert torch.equal(a[key], b[key]), key
    for j in (0, 3):
        alone = gpu_run(cases[j:j + 1], rr.SWEEP, 2048, sids[j:j + 1])
        for key in OUT_KEYS:
            assert torch.equal(alone[key][0], a[key][j]), (j, key)
    # batch order does not matter either
    rev = gpu_run(cases[::-1], rr.SWEEP, 2048, sids[::-1])
    for key in OUT_KEYS:
        assert torch.equal(rev[key].flip(0), a[key]), key
    other = gpu_run(cases, rr.SWEEP, 2048, sids, seed=1)
    assert (other["best_hypothesis"] != a["best_hypothesis"]).any()
    for j, r in enumerate(rows):
        for t, th in enumerate(rr.SWEEP):
            assert float(other["error"][j, t]) <= rr.error_bound(rr.TABLE[r][2], th), (j, th, float(other["error"][j, t]))
    # default stream ids are 0..B-1
    d0 = gpu_run(cases, [1.0], 512, None)
    d1 = gpu_run(cases, [1.0], 512, [0, 1, 2, 3])
    assert torch.equal(d0["best_hypothesis"], d1["best_hypothesis"]) and torch.equal(d0["H"], d1["H"])


def test_launch_shapes_pick_the_same_winner():
    """5, the part about the launch shape.  The hypotheses of a pair are split over ceil(512 / B) workgroups (ranges of
    at least 256): alone (B = 1) a pair's 2048 hypotheses are 8 ranges of 256, one per lane; in a batch of 128 they are
    4 ranges of 512, two passes per lane; in a batch of 512 -- the shape of the evaluation -- one workgroup scores all
    2048, eight passes per lane.  Same stream_id -> every output equal bit for bit."""
    cases = [c for r, _, c, _ in rr.table_cases() if r in (3, 4)]
    sids = [7, 1 << 40, 3, 12345]
    alone = [gpu_run(cases[j:j + 1], rr.SWEEP, 2048, sids[j:j + 1]) for j in range(4)]
    for rep in (32, 128):
        big = gpu_run(cases * rep, rr.SWEEP, 2048, sids * rep)
        for key in OUT_KEYS:
            for j in range(4):
                got = big[key][j::4]
                assert got.shape[0] == rep and torch.equal(got, alone[j][key].expand_as(got).contiguous()), (rep, key, j)
    # a count that leaves lanes idle and ranges unequal: 1000 hypotheses are 3 ranges of 334 alone, one range in the batch
    alone = [gpu_run(cases[j:j + 1], [1.0, 2.0], 1000, sids[j:j + 1]) for j in range(4)]
    big = gpu_run(cases * 128, [1.0, 2.0], 1000, sids * 128)
    for key in OUT_KEYS:
        for j in range(4):
            got = big[key][j::4]
            assert torch.equal(got, alone[j][key].expand_as(got).contiguous()), (key, j)


def test_failure_cases_and_bad_arguments():
    """6. n = 3, n = 0, all matches identical points -> success 0, identity, no inliers, +inf; bad arguments ->
    GFC_ERR_INVALID."""
    c = rr.make_case(12, 0.0, 0.0, seed=5)
    three = dict(c, m0=c["m0"].copy())
    three["m0"][np.nonzero(c["m0"] >= 0)[0][3:]] = -1
    none = dict(c, m0=np.full_like(c["m0"], -1))
    same = dict(c, kp0=np.tile(c["kp0"][:1], (12, 1)), kp1=np.tile(c["kp1"][:1], (12, 1)))
    out_of_range = dict(c, m0=np.where(c["m0"] >= 0, c["m0"] + 12, -1))  # indices >= N are not matches
    out = gpu_run([three, none, same, out_of_range, c], [0.5, 1.0, 3.0], 256, None)
    eye = torch.eye(3, dtype=torch.float64, device="cuda").expand(3, 3, 3)
    for j in range(4):
        assert not out["success"][j].any() and (out["best_hypothesis"][j] == -1).all(), j
        assert torch.equal(out["H"][j], eye) and torch.equal(out["H_minimal"][j], eye)
        assert not out["inliers"][j].any() and (out["num_inliers"][j] == 0).all()
        assert torch.isinf(out["error"][j]).all() and (out["error"][j] > 0).all()
    assert out["success"][4].all() and (out["num_inliers"][4] == 11).all()  # the good pair beside them is unharmed
    # shapes with fewer than 4 key points, and none at all
    for m in (3, 0):
        e = gpu_run([dict(c, kp0=c["kp0"][:m], kp1=c["kp1"][:m], m0=np.arange(m))], [1.0], 64, None)
        assert not e["success"].any() and e["inliers"].shape == (1, 1, m) and torch.isinf(e["error"]).all()
    # without a ground truth there is no error
    H, kp0, kp1, m0, size = to_dev([c])
    assert "error" not in eval_utils.homography_ransac(None, kp0, kp1, m0, None, 1.0)
    for bad in ({"ransac_th": 0.0}, {"ransac_th": [1.0] * 9}, {"ransac_th": float("nan")}, {"num_hypotheses": 0},
                {"ransac_th": []}, {"lo_iters": -1}):
        kw = {"ransac_th": 1.0, **bad}
        th = kw.pop("ransac_th")
        with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
            eval_utils.homography_ransac(H, kp0, kp1, m0, size, th, **kw)
    with pytest.raises(ValueError):
        eval_utils.homography_ransac(H, kp0, kp1, m0, None, 1.0)


def test_estimator_and_drop_in_interfaces():
    """7. GpuHomographyEstimator on matched points == homography_ransac on the same pair; eval_homography_robust
    un-batched / batched; an unknown estimator raises."""
    from glue_factory_colon_amd.homography_estimator import GpuHomographyEstimator

    cases = [c for r, _, c, _ in rr.table_cases() if r == 2]
    H, kp0, kp1, m0, size = to_dev(cases)
    full = eval_utils.homography_ransac(H, kp0, kp1, m0, size, 1.5, num_hypotheses=1024, stream_id=[0, 0])
    est = GpuHomographyEstimator({"ransac_th": 1.5, "options": {"num_hypotheses": 1024}})
    for j in range(2):
        valid = m0[j] > -1
        got = est({"m_kpts0": kp0[j][valid], "m_kpts1": kp1[j][m0[j][valid]]})
        assert got["success"] is True and got["M_0to1"].dtype == torch.float32 and got["M_0to1"].shape == (3, 3)
        assert torch.equal(got["M_0to1"], full["H"][j, 0].float())
        assert got["inliers"].dtype == torch.bool and torch.equal(got["inliers"], full["inliers"][j, 0][valid])
    bad = est({"m_kpts0": kp0[0][:3], "m_kpts1": kp1[0][:3]})
    assert bad["success"] is False and torch.equal(bad["M_0to1"], torch.eye(3, device="cuda")) and not bad["inliers"].any()
    conf = {"estimator": "gfc_amd", "ransac_th": 1.5, "num_hypotheses": 1024, "stream_id": 0}
    data = {"H_0to1": H, "view0": {"image_size": size}}
    pred = {"keypoints0": kp0, "keypoints1": kp1, "matches0": m0, "matching_scores0": torch.ones_like(kp0[..., 0])}
    batched = eval_utils.eval_homography_robust(data, pred, conf)
    assert set(batched) == {"H_error_ransac", "ransac_inl", "ransac_inl%"} and all(len(v) == 2 for v in batched.values())
    for j in range(2):
        single = eval_utils.eval_homography_robust({"H_0to1": H[j], "view0": {"image_size": size[j]}},
                                                   {k: v[j] for k, v in pred.items()}, conf)
        assert all(isinstance(v, float) for v in single.values())
        assert single["H_error_ransac"] == batched["H_error_ransac"][j] == float(full["error"][j, 0])
        assert single["ransac_inl"] == batched["ransac_inl"][j] == float(full["num_inliers"][j, 0])
        assert single["ransac_inl%"] == pytest.approx(float(full["num_inliers"][j, 0]) / int((m0[j] > -1).sum()))
    per_item = eval_utils.eval_homography_robust(data, pred, {**conf, "stream_id": [0, 0]})
    assert per_item == batched
    with pytest.raises(ValueError, match="gfc_amd"):
        eval_utils.eval_homography_robust(data, pred, {"estimator": "poselib", "ransac_th": 1.5})


def write_ppm(path, img):
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n" + f"{w} {h}\n255\n".encode() + img.tobytes())


ROBUST_SUMMARY_KEYS = {"H_error_ransac@1px", "H_error_ransac@3px", "H_error_ransac@5px", "H_error_ransac_mAA",
                       "med_H_error_ransac", "mean_H_error_ransac", "med_ransac_inl", "mean_ransac_inl",
                       "med_ransac_inl%", "mean_ransac_inl%"}


def test_hpatches_evaluation_with_the_estimator(tmp_path):
    """8. a ten-pair PPM directory (two sequences, view 1 = the canvas displaced by a known shift, so the written H_1_q
    is the true homography): with the estimator the summaries hold the robust keys, run_eval == run_eval_pairwise pair
    by pair, the robust error does not lose to the DLT on clean pairs, the command line prints the same summaries;
    without it the summaries are the DLT-only ones."""
    from glue_factory_colon_amd import eval_hpatches, synthetic
    from glue_factory_colon_amd.synthetic import HPATCHES_LIKE_ORIGINALS, HPATCHES_LIKE_SHAPES

    raw = synthetic.hpatches_like_host_images(10, seed=5200, pin=False, shared_view0=True)
    root = tmp_path / "hpatches-sequences-release"
    for i, it in enumerate(raw):
        seq = root / ("v_" + it["scene"])
        seq.mkdir(parents=True, exist_ok=True)
        if i % 5 == 0:
            write_ppm(seq / "1.ppm", it["view0"]["image"].numpy())
        write_ppm(seq / f"{i % 5 + 2}.ppm", it["view1"]["image"].numpy())
        j0, j1 = (i // 5) % 5, (i * 2 + 1) % 5
        u0x, u0y = (HPATCHES_LIKE_ORIGINALS[j0][k] / HPATCHES_LIKE_SHAPES[j0][k] for k in (1, 0))
        u1x, u1y = (HPATCHES_LIKE_ORIGINALS[j1][k] / HPATCHES_LIKE_SHAPES[j1][k] for k in (1, 0))
        dx, dy = 24 + 6 * (i % 5), 16 + 4 * (i % 5)
        H = np.array([[u1x / u0x, 0, -dx * u1x], [0, u1y / u0y, -dy * u1y], [0, 0, 1.0]])
        (seq / f"H_1_{i % 5 + 2}").write_text("\n".join(" ".join(f"{v:.10g}" for v in row) for row in H) + "\n")
    eval_conf = {"estimator": "gfc_amd", "ransac_th": -1}
    pipe = eval_hpatches.HPatchesPipeline({"data_dir": str(root)}, pair_batch=8, eval_conf=eval_conf)
    model = eval_hpatches.build_model("synthetic", "synthetic", official=False, max_num_keypoints=512).cuda()
    summaries, results = pipe.run(tmp_path / "exp", model)
    pred_file = tmp_path / "exp" / "predictions.h5"
    assert ROBUST_SUMMARY_KEYS <= set(summaries)
    assert sorted(results["pose_results"]) == rr.SWEEP
    for key in ("H_error_ransac", "ransac_inl", "ransac_inl%"):
        assert len(results[key]) == 10
    best = [th for th, r in results["pose_results"].items() if r["H_error_ransac"] == results["H_error_ransac"]]
    assert best, "the per-pair lists are those of one tested threshold"
    aucs = eval_hpatches.cal_error_auc(results["H_error_ransac"], [1, 3, 5])
    assert [summaries[f"H_error_ransac@{t}px"] for t in (1, 3, 5)] == [float(a) for a in aucs]
    assert summaries["H_error_ransac_mAA"] == pytest.approx(float(np.mean(aucs)))
    assert summaries["H_error_ransac_mAA"] >= max(float(np.mean(eval_hpatches.cal_error_auc(r["H_error_ransac"], [1, 3, 5])))
                                                  for r in results["pose_results"].values())
    # clean pairs: those whose matches follow the written homography (the first of each sequence, ~340 matches each)
    clean = [i for i in range(10) if results["prec@3px"][i] > 0.95 and results["num_matches"][i] >= 4]
    assert {0, 5} <= set(clean)
    for i in clean:
        assert results["H_error_ransac"][i] <= results["H_error_dlt"][i] + 0.1, (i, results["H_error_ransac"][i], results["H_error_dlt"][i])
        assert results["ransac_inl"][i] >= 4 and 0 < results["ransac_inl%"][i] <= 1
    # the reference's loop shape: one pair and one threshold at a time through the drop-in function, stream = pair index
    pairwise = pipe.run_eval_pairwise(pred_file)
    assert sorted(pairwise["pose_results"]) == rr.SWEEP
    for th in rr.SWEEP:
        for key in ("H_error_ransac", "ransac_inl", "ransac_inl%"):
            assert pairwise["pose_results"][th][key] == results["pose_results"][th][key], (th, key)
    # without an estimator: the DLT-only summaries, same values
    plain = eval_hpatches.HPatchesPipeline({"data_dir": str(root)}, pair_batch=8)
    plain_summaries, plain_results = plain.run_eval(pred_file)
    assert set(plain_summaries) == set(summaries) - ROBUST_SUMMARY_KEYS and not any("ransac" in k for k in plain_summaries)
    assert all(plain_summaries[k] == summaries[k] for k in plain_summaries)
    assert "pose_results" not in plain_results and "pose_results" not in plain.run_eval_pairwise(pred_file)
    want_keys = {f"{p}_{k}" for p in ("med", "mean") for k in (*eval_utils.RESULT_KEYS, "H_error_dlt")}
    optional = {f"{p}_{k}" for p in ("med", "mean") for k in eval_hpatches.OPTIONAL_EXPORT_KEYS}  # what the records carry
    assert set(plain_summaries) - optional == want_keys | {f"H_error_dlt@{t}px" for t in (1, 3, 5)}
    with pytest.raises(ValueError, match="gfc_amd"):
        eval_hpatches.HPatchesPipeline({"data_dir": str(root)}, eval_conf={"estimator": "opencv"})
    with pytest.raises(ValueError, match="thresholds"):
        eval_hpatches.HPatchesPipeline({"data_dir": str(root)}, eval_conf={"estimator": "gfc_amd", "ransac_th": [1.0] * 9})
    # the command line, in a child process with its own time limit
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "glue_factory_colon_amd.eval_hpatches", "--data_dir", str(root), "--open",
                        "--pair_batch", "8", "--experiment_dir", str(tmp_path / "cli"), "--estimator", "gfc_amd",
                        "--ransac_th", "-1"], capture_output=True, text=True, cwd=root_dir, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cli = json.loads(r.stdout[r.stdout.index("{"):])
    # the command line builds its model with the default 1024 key points: the same pipeline in this process
    model_1024 = eval_hpatches.build_model("synthetic", "synthetic", official=False).cuda()
    same, _ = eval_hpatches.HPatchesPipeline({"data_dir": str(root)}, pair_batch=8, eval_conf=eval_conf).run(tmp_path / "exp1024", model_1024)
    assert set(cli) == set(same) == set(summaries)
    assert cli == json.loads(json.dumps(same))
