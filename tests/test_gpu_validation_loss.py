"""gfc_lg_validation_metrics (csrc/lg_validation.hip) through losses / metrics / LightGlue.loss / TwoViewPipeline.loss /
validate, against the reference's vectors (tests/golden/validation.npz) and the float64 restatement
(tests/validation_reference.py) on the same log assignment.

Bounds (E = 2^-24, one float32 rounding):
  counts, ratios   num_matchable, num_unmatchable, match_recall, match_precision, accuracy: equal to the reference's float32
                   values -- exact integers and one correctly rounded division.
  nll_pos, nll_neg, assignment_nll
                   the kernel adds float32 values in fp64 (a few thousand terms: error below 1e-12 relative) and rounds
                   the quotient once: |x - x64| <= E |x64| (+ 1e-12).
  row_norm         every term is expf of a float32, documented at 1 ulp = 2 E relative; the terms are positive, so the
                   sum carries at most 2 E, plus the final rounding: |x - x64| <= 3 E |x64|.
  against the reference's float32 values: the same plus the reference's own |float32 - float64| stored in the fixture.
  average_precision within (M + 2) E of the reference's value, which sums M - 1 rounded products.
Measured worst case on an MI355X over all cases here, in units of the float64 bound: 0.60 (`nopos`; the tests print
RATIOS per case).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endopatches_reference as er  # noqa: E402
import hpatches_reference as hr  # noqa: E402
import validation_cases as vc  # noqa: E402
import validation_reference as vr  # noqa: E402

from glue_factory_colon_amd import lightglue, synthetic, weights  # noqa: E402
from glue_factory_colon_amd.homography_matcher import HomographyMatcher  # noqa: E402
from glue_factory_colon_amd.losses import NLLLoss, validation_metrics  # noqa: E402
from glue_factory_colon_amd.metrics import matcher_metrics  # noqa: E402
from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2.0**-24
EXACT = ("num_matchable", "num_unmatchable", "match_recall", "match_precision", "accuracy")
NLL = ("nll_pos", "nll_neg", "assignment_nll")
LA_TOL = 1e-4  # the suite's bound on this matcher's log assignment against the reference (tests/test_gpu_models.py)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "validation.npz"))


def bound(key, x64):
    return (3 * E if key == "row_norm" else E) * abs(x64) + 1e-12


def check_row(name, got, row64, m, ref32=None, ref64=None):
    """got [10] from the kernel against the float64 restatement row64 (and the reference's float32 / float64 rows)."""
    worst = 0.0
    for i, key in enumerate(vr.OUT_KEYS):
        g, x = float(got[i]), float(row64[i])
        if key in NLL or key == "row_norm":
            ratio = abs(g - x) / bound(key, x)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, key, g, x)
            if ref32 is not None:
                assert abs(g - ref32[i]) <= bound(key, x) + abs(ref32[i] - ref64[i]), (name, key, g, ref32[i])
        elif key == "average_precision":
            assert abs(g - (x if ref32 is None else ref32[i])) <= (m + 2) * E, (name, key, g, x)
        elif ref32 is not None:
            assert g == float(np.float32(ref32[i])), (name, key, g, ref32[i])
        else:  # the restatement's quotient has 1e-8 in its denominator: equal to one float32 rounding
            assert abs(g - x) <= 2 * E * abs(x), (name, key, g, x)
    print("RATIOS", name, "worst |kernel - float64| / bound", round(worst, 4))
    return worst


@pytest.mark.parametrize("name", [c[0] for c in vc.LOSS_CASES])
@pytest.mark.parametrize("dense", [True, False])
def test_fixture_cases(z, name, dense):
    t = lambda k: torch.from_numpy(z[f"loss_{name}_{k}"])  # noqa: E731
    la, gt0, gt1, m0, s0 = vc.la_of(t("la_q")), t("gt0"), t("gt1"), t("m0"), t("scores0")
    asg = t("assignment") if dense else None
    row64 = vr.validation_row(la, gt0, gt1, asg, m0, s0)
    out = validation_metrics(la[None].cuda(), gt0[None].cuda(), gt1[None].cuda(), None if asg is None else asg[None].cuda(),
                             m0[None].cuda(), s0[None].cuda())
    torch.cuda.synchronize()
    check_row(name, out[0].cpu(), row64, len(gt0), z[f"loss_{name}_ref32"], z[f"loss_{name}_ref64"])
    # the module faces give the same numbers under the reference's keys
    pred = {"log_assignment": la[None].cuda(), "matches0": m0[None].cuda(), "matching_scores0": s0[None].cuda()}
    data = {"gt_matches0": gt0[None].cuda(), "gt_matches1": gt1[None].cuda()}
    if dense:
        data["gt_assignment"] = asg[None].cuda()
    nll, weights_, lm = NLLLoss({})(pred, data)
    assert weights_ is None and set(lm) == {"assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable"}
    assert torch.equal(nll, out[:, 4]) and torch.equal(lm["nll_pos"], out[:, 0]) and nll.shape == (1,)
    mm = matcher_metrics(pred, data)
    assert list(mm) == ["match_recall", "match_precision", "accuracy", "average_precision"]
    for i, k in zip((6, 7, 8, 9), mm):
        assert torch.equal(mm[k], out[:, i]), k
    pm = matcher_metrics({"x_matches0": pred["matches0"], "x_matching_scores0": pred["matching_scores0"]},
                         {"gt_y_matches0": data["gt_matches0"]}, prefix="x_", prefix_gt="y_")
    assert list(pm) == ["x_match_recall", "x_match_precision", "x_accuracy", "x_average_precision"]
    assert torch.equal(pm["x_average_precision"], mm["average_precision"])


def test_batch_of_two_at_1024_and_a_pair_alone():
    cases = [vc.loss_case(50 + i, 1024, 1024) for i in range(2)]
    st = lambda k: torch.stack([c[k] for c in cases]).cuda()  # noqa: E731
    la = torch.stack([vc.la_of(c["la_q"]) for c in cases]).cuda()
    for dense in (True, False):
        out = validation_metrics(la, st("gt0"), st("gt1"), st("assignment") if dense else None, st("m0"), st("scores0"),
                                 nll_balancing=0.3)
        torch.cuda.synchronize()
        for i, c in enumerate(cases):
            row64 = vr.validation_row(vc.la_of(c["la_q"]), c["gt0"], c["gt1"], c["assignment"] if dense else None,
                                      c["m0"], c["scores0"], nll_balancing=0.3)
            check_row(f"1024_{i}_{dense}", out[i].cpu(), row64, 1024)
            one = validation_metrics(la[i:i + 1], st("gt0")[i:i + 1], st("gt1")[i:i + 1],
                                     st("assignment")[i:i + 1] if dense else None, st("m0")[i:i + 1],
                                     st("scores0")[i:i + 1], nll_balancing=0.3)
            assert torch.equal(one[0], out[i])


def lightglue_inputs(z):
    kp0, kp1, H = (torch.from_numpy(z[k]) for k in ("lg_kp0", "lg_kp1", "lg_H"))
    back = hr.warp(kp1.double(), torch.linalg.inv(H.double()))
    size = torch.tensor([[640.0, 480.0]])
    return {"keypoints0": kp0[None].cuda(), "keypoints1": kp1[None].cuda(),
            "descriptors0": vc.descriptors_for(kp0)[None].cuda(), "descriptors1": vc.descriptors_for(kp1, partner=back)[None].cuda(),
            "view0": {"image_size": size.cuda()}, "view1": {"image_size": size.cuda()}, "H_0to1": H[None].cuda()}


def test_lightglue_loss_on_its_own_forward(z):
    """300 + 257 points through the module's own forward, its eval-mode loss against the fixture's (the reference's
    LightGlue.loss on the reference's forward).  The precondition is the suite's parity of this matcher (equal matches,
    log assignment within LA_TOL); then nll_* are means of entries each within LA_TOL, and row_norm = mean of sums of
    exp(la) moves by at most exp(LA_TOL) - 1 relative."""
    data = lightglue_inputs(z)
    m = lightglue.LightGlue({"filter_threshold": 0.0}).eval()
    m.load_state_dict(weights.lightglue_state_dict(0), strict=False)
    pred = m.cuda()(data)
    for dense in (True, False):
        gt = HomographyMatcher({"dense_outputs": dense}).eval()(({**data, **pred}))
        assert torch.equal(gt["matches0"][0].cpu(), torch.from_numpy(z["lg_gt_matches0"]))
        assert torch.equal(gt["matches1"][0].cpu(), torch.from_numpy(z["lg_gt_matches1"]))
        labels = {f"gt_{k}": v for k, v in gt.items()}
        losses, metrics = m.loss(pred, {**data, **pred, **labels})
        torch.cuda.synchronize()
        assert list(losses) == ["total", "last", "assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable",
                                "row_norm"]
        assert list(metrics) == ["match_recall", "match_precision", "accuracy", "average_precision"]
        assert torch.equal(losses["total"], losses["assignment_nll"]) and torch.equal(losses["last"], losses["total"])
        got = {k: float(v[0]) for k, v in {**losses, **metrics}.items()}
        # exactly what the restatement makes of the module's own prediction
        row64 = vr.validation_row(pred["log_assignment"][0].cpu(), gt["matches0"][0].cpu(), gt["matches1"][0].cpu(),
                                  gt["assignment"][0].cpu() if dense else None, pred["matches0"][0].cpu(),
                                  pred["matching_scores0"][0].cpu())
        check_row(f"lightglue_{dense}", torch.tensor([got[k] for k in vr.OUT_KEYS]), row64, 300)
        # and the fixture
        assert torch.equal(pred["matches0"][0].cpu(), torch.from_numpy(z["lg_matches0"]))
        for k in ("num_matchable", "num_unmatchable", "match_recall", "match_precision", "accuracy"):
            assert got[k] == float(z[f"lg_{k}"]), (k, got[k], float(z[f"lg_{k}"]))
        for k in ("total", "last", "assignment_nll", "nll_pos", "nll_neg"):
            print("lightglue", k, got[k], float(z[f"lg_{k}"]))
            assert abs(got[k] - float(z[f"lg_{k}"])) <= LA_TOL + 4 * E * abs(got[k]), (k, got[k], float(z[f"lg_{k}"]))
        assert abs(got["row_norm"] - float(z["lg_row_norm"])) <= 1.1 * LA_TOL * got["row_norm"]
        assert abs(got["average_precision"] - float(z["lg_average_precision"])) <= 302 * E


def test_lightglue_loss_refuses_what_it_does_not_hold(z):
    data = lightglue_inputs(z)
    m = lightglue.LightGlue({"filter_threshold": 0.0, "depth_confidence": 0.95}).eval()
    m.load_state_dict(weights.lightglue_state_dict(0), strict=False)
    pred = m.cuda()(data)
    with pytest.raises(NotImplementedError, match="early-stopped"):
        m.loss(pred, {**data, **pred, "gt_matches0": pred["matches0"], "gt_matches1": pred["matches1"]})


PIPE_CONF = {"extractor": {"name": "extractors.superpoint_open", "weights": "synthetic", "max_num_keypoints": 256,
                           "detection_threshold": 0.0, "nms_radius": 3},
             "matcher": {"name": "matchers.lightglue", "weights": "synthetic", "filter_threshold": 0.0, "flash": False},
             "ground_truth": {"name": "matchers.homography_matcher", "th_positive": 3, "th_negative": 5}}


@pytest.mark.parametrize("in_forward", [False, True])
def test_superpoint_lightglue_homography_matcher_through_the_pipeline(in_forward):
    v0, v1 = synthetic.synthetic_pairs(2, 240, 320, seed=5)  # view 1 is view 0 shifted by (16, 8)
    H = torch.tensor([[1.0, 0, 16], [0, 1, 8], [0, 0, 1]]).repeat(2, 1, 1).cuda()
    size = torch.tensor([[320.0, 240.0]] * 2).cuda()
    data = {"view0": {"image": v0.cuda(), "image_size": size}, "view1": {"image": v1.cuda(), "image_size": size},
            "H_0to1": H}
    pipe = TwoViewPipeline({**PIPE_CONF, "run_gt_in_forward": in_forward}).eval().cuda()
    pred = pipe(data)
    assert ("gt_matches0" in pred) == in_forward
    losses, metrics = pipe.loss(pred, data)
    torch.cuda.synchronize()
    assert {"gt_matches0", "gt_matches1", "gt_assignment", "gt_reward", "gt_proj_0to1"} <= set(pred)
    assert set(losses) == {"total", "last", "assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable",
                           "row_norm"} and set(metrics) == {"match_recall", "match_precision", "accuracy",
                                                            "average_precision"}
    assert losses["total"].shape == (2,) and torch.equal(losses["total"], losses["assignment_nll"])
    assert (pred["gt_matches0"] > -1).sum() > 100  # the shift is known: most key points have a partner
    for i in range(2):
        c = lambda k: pred[k][i].cpu()  # noqa: E731
        g = vr.gt_matches_homography(c("keypoints0").double(), c("keypoints1").double(), H[i].cpu().double(), 3.0, 5.0)
        sure0, sure1 = ~g["undecided0"], ~g["undecided1"]
        assert torch.equal(c("gt_matches0")[sure0], g["matches0"][sure0])
        assert torch.equal(c("gt_matches1")[sure1], g["matches1"][sure1])
        row64 = vr.validation_row(c("log_assignment"), c("gt_matches0"), c("gt_matches1"), c("gt_assignment"),
                                  c("matches0"), c("matching_scores0"))
        got = {k: float(v[i]) for k, v in {**losses, **metrics}.items()}
        # (tied top scores: validation_row takes the lowest index among them, the documented choice of the kernel)
        check_row(f"pipeline_{i}", torch.tensor([got[k] for k in vr.OUT_KEYS]), row64, c("matches0").shape[0])


def test_validate_run_on_a_generated_directory(tmp_path):
    """`ValidationPipeline.run` on a generated `homographies` tree: the returned means are the means of the per-pair values
    (`model.loss` pair by pair), one device-to-host read per (M, N) group, and the TSV has one line per pair."""
    import shutil

    from glue_factory_colon_amd import validate
    from glue_factory_colon_amd.registry import get_dataset

    names = er.make_tree(tmp_path, per_sequence=3, hw=(120, 160))
    for n in names:
        shutil.copy(tmp_path / "frames" / "test" / n, tmp_path / "frames" / "val" / n)
    conf = {"data_dir": "frames", "photometric": {"name": "identity"}, "reseed": True, "val_size": 5,
            "homography": {"difficulty": 0.5, "max_angle": 30, "patch_shape": [96, 72]}}
    ds = get_dataset("homographies")(conf, tmp_path, split="val")
    assert len(ds) == 5
    vp = validate.ValidationPipeline({"extractor": {"max_num_keypoints": 128}}, pair_batch=4)
    tsv = tmp_path / "val.tsv"
    seen = []  # the (M, N) of every pair, chunk by chunk, from the predictions `run` itself makes
    inner = vp.model.forward_pairs

    def recording(datas, view_keys=None):
        preds = inner(datas, view_keys=view_keys)
        seen.append([(p["keypoints0"].shape[1], p["keypoints1"].shape[1]) for p in preds])
        return preds

    vp.model.forward_pairs = recording
    res = vp.run(ds.feeder(batch=4, num_workers=0), log_metrics=tsv, step=7)
    vp.model.forward_pairs = inner
    assert res["num_pairs"] == 5 and [len(c) for c in seen] == [4, 1]
    assert vp.reads == sum(len(set(c)) for c in seen)  # ONE device-to-host read per (M, N) group of a chunk
    keys = {"match_recall", "match_precision", "accuracy", "average_precision", "loss/total", "loss/last",
            "loss/assignment_nll", "loss/nll_pos", "loss/nll_neg", "loss/num_matchable", "loss/num_unmatchable",
            "loss/row_norm", "num_pairs"}
    assert set(res) == keys
    per_pair = {k: [] for k in keys - {"num_pairs"}}
    for item in ds.feeder(batch=4, num_workers=0):
        pred = vp.model(item)
        losses, metrics = vp.model.loss(pred, item)
        for k, v in {**metrics, **{"loss/" + k: v for k, v in losses.items()}}.items():
            per_pair[k].append(float(v[0]))
    for k, values in per_pair.items():
        values = [v for v in values if v == v]
        assert abs(res[k] - sum(values) / len(values)) <= 1e-5 * max(1.0, abs(res[k])), (k, res[k], values)
    lines = tsv.read_text().splitlines()
    assert lines[0] == "step\tindex\tname\toverlap\tprecision\trecall\taccuracy\tap" and len(lines) == 6
    for j, line in enumerate(lines[1:]):
        cols = line.split("\t")
        assert cols[0] == "7" and cols[1] == f"{j}_0" and cols[3] == "nan" and len(cols) == 8
        assert abs(float(cols[4]) - per_pair["match_precision"][j]) <= 1e-6
        assert abs(float(cols[7]) - per_pair["average_precision"][j]) <= 1e-6
    vp.run(ds.feeder(batch=4, num_workers=0), log_metrics=tsv, step=8)  # appended, no second header
    assert len(tsv.read_text().splitlines()) == 11


def test_validate_run_on_posed_pairs_and_the_command_line(tmp_path):
    """`ValidationPipeline.run` over a `PosedPairFeeder` with the depth matcher (th_epi 5): the means of the per-pair
    `model.loss` values, and the command line on the same directory."""
    import posed_reference as pr

    from glue_factory_colon_amd import posed_images, validate

    pr.write_dataset(tmp_path, "megadepth1500", (240, 320), 3, [(0, 1), (1, 2), (0, 2)], model="PINHOLE", seed=2)
    ds = posed_images.PosedImages(pr.CONF_B, tmp_path)
    gt = {**validate.DEPTH_GROUND_TRUTH, "th_epi": 5.0}
    vp = validate.ValidationPipeline({"extractor": {"max_num_keypoints": 128}, "ground_truth": gt}, pair_batch=2)
    res = vp.run(posed_images.PosedPairFeeder(ds, "cuda"))
    assert res["num_pairs"] == 3 and 2 <= vp.reads <= 3 and "loss/total" in res and "match_recall" in res
    per_pair = {}
    for item in posed_images.PosedPairFeeder(ds, "cuda"):
        pred = vp.model(item)
        losses, metrics = vp.model.loss(pred, item)
        assert {"gt_matches0", "gt_visible0", "gt_depth_keypoints0"} <= set(pred) and "gt_assignment" not in pred
        for k, v in {**metrics, **{"loss/" + k: v for k, v in losses.items()}}.items():
            per_pair.setdefault(k, []).append(float(v[0]))
    assert sum(per_pair["loss/num_unmatchable"]) > 3  # there are labels: not every point is ignored
    for k, values in per_pair.items():
        values = [v for v in values if v == v]
        # a pair alone against the pair in `forward_pairs`: the suite's bound on the log assignment, 1e-4 (1 + |la|)
        # (tests/test_gpu_models.py); the loss terms are means of such entries, the counts are equal
        assert abs(res[k] - sum(values) / len(values)) <= 1e-4 * (1.0 + abs(res[k])), (k, res[k], values)
    pr.write_dataset(tmp_path, "endomapper_dense1500", (540, 720), 3, [(0, 1), (2, 1)], model="OPENCV_FISHEYE",
                     with_scene_info=True, seed=1)
    cli = validate.main(["--data_dir", str(tmp_path), "--dataset", "posed_images", "--benchmark", "endomapper_dense1500",
                         "--th_epi", "5", "--max_num_keypoints", "128", "--pair_batch", "2",
                         "--log_metrics", str(tmp_path / "posed.tsv")])
    assert cli["num_pairs"] == 2 and len((tmp_path / "posed.tsv").read_text().splitlines()) == 3
