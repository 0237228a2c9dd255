"""The validation pass without a GPU: tests/validation_reference.py (the float64 restatement the GPU tests compare with)
against vectors the reference project produced (tests/golden/validation.npz, made by make_golden_validation.py), the
closed form of ranking_ap, the margin census of the GPU fixtures, and the module contracts (registry names, conf
defaults, refusals, pipeline construction).  Nothing is launched.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import validation_cases as vc  # noqa: E402
import validation_reference as vr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import homography_matcher, lightglue, losses, metrics, two_view_pipeline  # noqa: E402
from glue_factory_colon_amd.registry import get_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT_NAMES = ("exact", "130x67", "twins", "masks", "65x1", "1x65")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "validation.npz"))


def gt_inputs(z, name, dtype=torch.float64):
    t = lambda k: torch.from_numpy(z[f"gt_{name}_{k}"])  # noqa: E731
    v0 = t("valid0") if f"gt_{name}_valid0" in z.files else None
    v1 = t("valid1") if f"gt_{name}_valid1" in z.files else None
    pos, neg = (float(v) for v in z[f"gt_{name}_th"])
    return t("kp0").to(dtype), t("kp1").to(dtype), t("H").to(dtype), pos, neg, v0, v1


def restated(z, name, rule=None):
    kp0, kp1, H, pos, neg, v0, v1 = gt_inputs(z, name)
    return vr.gt_matches_homography(kp0, kp1, H, pos, neg, v0, v1, rule=rule)


@pytest.mark.parametrize("name", GT_NAMES)
def test_gt_restatement_equals_the_reference_vectors(z, name):
    r = restated(z, name)
    for k in ("matches0", "matches1", "assignment"):
        assert np.array_equal(r[k].numpy(), z[f"gt_{name}_{k}"]), (name, k)
    assert np.array_equal(r["reward"].numpy(), z[f"gt_{name}_reward"].astype(np.float64)), name
    for k in ("proj_0to1", "proj_1to0"):
        assert np.abs(r[k].numpy() - z[f"gt_{name}_{k}_f64"]).max() <= 1e-9, (name, k)
    g0 = z[f"gt_{name}_matches0"]
    if name in ("130x67", "twins", "masks"):
        assert (g0 > -1).any() and (g0 == -1).any() and (g0 == -2).any()


@pytest.mark.parametrize("name", [n for n in GT_NAMES if n != "exact"])
def test_margin_census_of_the_gpu_fixtures_is_zero(z, name):
    r = restated(z, name)
    assert int(r["undecided0"].sum()) == 0 and int(r["undecided1"].sum()) == 0 and int(r["undecided_dense"].sum()) == 0


def test_the_exact_case_sits_on_the_threshold_and_nowhere_else(z):
    r = restated(z, "exact")
    assert bool(r["undecided0"][0]) and bool(r["undecided_dense"][0, 0]) and int(r["undecided_dense"].sum()) == 1
    kp0, kp1, H, *_ = gt_inputs(z, "exact", torch.float32)
    d0 = ((vr.warp(kp0, H, 1e-5)[0] - kp1[0]) ** 2).sum()
    assert float(d0) == 9.0 and int(z["gt_exact_matches0"][0]) != 0 and not z["gt_exact_assignment"][0, 0]


@pytest.mark.parametrize("rule,name", [("pos_le", "exact"), ("masked_negatives", "masks"), ("last_index_ties", "twins")])
def test_wrong_rules_are_rejected_by_the_fixture(z, rule, name):
    r = restated(z, name, rule=rule)
    differs = any(not np.array_equal(r[k].numpy(), z[f"gt_{name}_{k}"]) for k in ("matches0", "matches1", "assignment"))
    assert differs, (rule, name)


def test_twins_the_lower_index_carries_the_match(z):
    g0, g1 = z["gt_twins_matches0"], z["gt_twins_matches1"]
    (i_lo, i_hi), (j_lo, j_hi), i = z["gt_twins_dup0"], z["gt_twins_dup1"], int(z["gt_twins_dup_row"])
    assert g0[i] == j_lo and g1[j_lo] == i and g1[j_hi] == -2 and g0[i_lo] > -1 and g0[i_hi] == -2
    assert z["gt_twins_assignment"][i, j_lo] and not z["gt_twins_assignment"][i, j_hi]


def test_masks_invalid_points_are_ignored_never_unmatched(z):
    g0, v0 = z["gt_masks_matches0"], z["gt_masks_valid0"]
    assert not v0[10:20].any() and (g0[~v0] == -2).all() and (z["gt_masks_matches1"][~z["gt_masks_valid1"]] == -2).all()
    assert not z["gt_masks_assignment"][~v0].any() and (z["gt_masks_reward"][~v0] == -1).all()  # +inf > neg_th^2


@pytest.mark.parametrize("name", [c[0] for c in vc.LOSS_CASES])
@pytest.mark.parametrize("dense", [True, False])
def test_loss_restatement_equals_the_reference_vectors(z, name, dense):
    t = lambda k: torch.from_numpy(z[f"loss_{name}_{k}"])  # noqa: E731
    row = vr.validation_row(vc.la_of(t("la_q")), t("gt0"), t("gt1"), t("assignment") if dense else None, t("m0"),
                            t("scores0"))
    ref64, ref32 = z[f"loss_{name}_ref64"], z[f"loss_{name}_ref32"]
    m = len(t("gt0"))
    for i, key in enumerate(vr.OUT_KEYS):
        got = float(row[i])
        if key == "average_precision":  # the reference sums M - 1 rounded float32 products
            assert abs(got - ref32[i]) <= (m + 2) * 2.0**-24, (name, key, got, ref32[i])
        elif key in ("match_recall", "match_precision", "accuracy"):  # float32 in the reference whatever the input
            assert abs(got - ref32[i]) <= 2.0**-23 * abs(ref32[i]) and ref32[i] == ref64[i], (name, key, got, ref32[i])
        else:
            assert abs(got - ref64[i]) <= 1e-12 * max(1.0, abs(ref64[i])), (name, key, got, ref64[i])
            assert abs(ref32[i] - ref64[i]) <= 1e-5 * max(1.0, abs(ref64[i]))


def test_ap_closed_form_equals_the_reference_function(z):
    cases = vc.ap_cases()
    assert len(cases) == 12
    for name, m, gt, s in cases:
        assert np.array_equal(m.numpy(), z[f"ap_{name}_m"]) and np.array_equal(s.numpy(), z[f"ap_{name}_scores"])
        top = s.max()
        assert float(top) == 0.0 or int((s == top).sum()) == 1, name  # unique top score, or none above zero
        closed, ref = vr.ranking_ap_closed(m, gt, s), float(z[f"ap_{name}_ref"])
        assert abs(closed - ref) <= (len(m) + 2) * 2.0**-24, (name, closed, ref)
        assert abs(closed - vr.ranking_ap_sorted(m, gt, s)) <= 1e-12, name
    byname = {c[0]: float(z[f"ap_{c[0]}_ref"]) for c in cases}
    assert byname["zero_scores"] == 0 and byname["all_ignore"] == 0 and byname["none_matchable"] == 0
    assert min(byname["top_true_positive"], byname["top_false_positive"], byname["random5_40"]) > 0


def test_ap_ties_at_the_top_take_the_lowest_index():
    m, gt = torch.tensor([3, 1, -1]), torch.tensor([3, 2, -1])
    s = torch.tensor([0.5, 0.5, 0.0])
    assert vr.ranking_ap_closed(m, gt, s) == vr.ranking_ap_sorted(m, gt, s) == 0.0  # element 0 is the top: its step is lost
    assert vr.ranking_ap_closed(m.flip(0), gt.flip(0), s.flip(0)) > 0.2  # now element 1 (a false positive) is the top


# ---- module contracts ------------------------------------------------------------------------------------------------
def test_registry_names_resolve():
    for name in ("matchers.homography_matcher", "homography_matcher", "gluefactory.models.matchers.homography_matcher"):
        assert get_model(name) is homography_matcher.HomographyMatcher


def test_conf_defaults_equal_the_reference():
    conf = homography_matcher.HomographyMatcher({}).conf
    ref = {"use_points": True, "th_positive": 3.0, "th_negative": 3.0, "use_lines": False, "n_line_sampled_pts": 50,
           "line_perp_dist_th": 5, "overlap_th": 0.2, "min_visibility_th": 0.5}
    assert {k: conf[k] for k in ref} == ref and conf.dense_outputs is True
    assert set(conf) - set(ref) - {"name", "trainable", "freeze_batch_normalization", "timeit"} == {"dense_outputs"}
    m = homography_matcher.HomographyMatcher({})
    assert m.required_data_keys == ["H_0to1", "keypoints0", "keypoints1"]
    assert losses.NLLLoss.default_conf == {"nll_balancing": 0.5, "gamma_f": 0.0}
    assert losses.NLLLoss({"gamma_f": 2.0}).conf == {"nll_balancing": 0.5, "gamma_f": 2.0}
    assert lightglue.LightGlue.default_conf["loss"] == {"gamma": 1.0, "fn": "nll", "nll_balancing": 0.5}
    assert metrics.KEYS == ("match_recall", "match_precision", "accuracy", "average_precision")


def test_refusals():
    with pytest.raises(NotImplementedError, match="use_lines"):
        homography_matcher.HomographyMatcher({"use_lines": True})
    with pytest.raises(NotImplementedError, match="th_positive <= th_negative"):
        homography_matcher.HomographyMatcher({"dense_outputs": False, "th_positive": 5.0, "th_negative": 3.0})
    homography_matcher.HomographyMatcher({"dense_outputs": True, "th_positive": 5.0, "th_negative": 3.0})
    homography_matcher.HomographyMatcher({"dense_outputs": False, "th_positive": 3.0, "th_negative": 3.0})
    with pytest.raises(NotImplementedError):
        homography_matcher.HomographyMatcher({}).loss({}, {})
    with pytest.raises(nat.NativeError, match="no CPU implementation"):
        homography_matcher.HomographyMatcher({})({"H_0to1": torch.eye(3)[None], "keypoints0": torch.zeros(1, 3, 2),
                                                  "keypoints1": torch.zeros(1, 3, 2)})
    lg = lightglue.LightGlue({"weights": "synthetic"}).eval()
    with pytest.raises(nat.NativeError, match="no CPU implementation"):
        lg.loss({"log_assignment": torch.zeros(1, 2, 2), "matches0": torch.zeros(1, 1).long(),
                 "matching_scores0": torch.zeros(1, 1)},
                {"gt_matches0": torch.zeros(1, 1).long(), "gt_matches1": torch.zeros(1, 1).long()})
    with pytest.raises(NotImplementedError, match="training"):
        lg.train().loss({}, {})
    for conf in ({"depth_confidence": 0.95}, {"width_confidence": 0.99}):
        with pytest.raises(NotImplementedError, match="early-stopped"):
            lightglue.LightGlue({"weights": "synthetic", **conf}).eval().loss({}, {})
    with pytest.raises(NotImplementedError, match="re-used weights"):
        losses.NLLLoss({}).forward({}, {}, weights=torch.zeros(1))


def test_pipeline_builds_its_ground_truth_through_the_registry():
    pipe = two_view_pipeline.TwoViewPipeline({"ground_truth": {"name": "matchers.homography_matcher",
                                                               "th_positive": 3, "th_negative": 5}})
    assert isinstance(pipe.ground_truth, homography_matcher.HomographyMatcher)
    assert pipe.ground_truth.conf.th_negative == 5 and pipe.is_initialized()
    for comp in ("filter", "solver"):
        with pytest.raises(NotImplementedError, match=comp):
            two_view_pipeline.TwoViewPipeline({comp: {"name": "anything"}})
    # a pipeline whose components have no loss sums nothing (two_view_pipeline.py:407-429)
    bare = two_view_pipeline.TwoViewPipeline({})
    assert bare.loss({}, {}) == ({"total": 0}, {})


def test_lds_account_of_the_ground_truth_kernel():
    lds = nat.lib().gfc_gt_matches_homography_lds_bytes
    assert lds(0, 0) == 0 and lds(1, 1) == 42 and lds(2048, 2048) == 21 * 4096 and lds(-1, 3) == 0
    assert lds(1560, 1560) <= 64 * 1024 < lds(1561, 1560)
    assert lds(3901, 3900) <= 160 * 1024 < lds(3901, 3901)


def test_the_validation_header_is_parsed_by_the_same_grammar_and_exported():
    """include/gfc_amd_validation.h: three functions, no struct / enum / constant, none of gfc_amd.h's names; every one
    exported by the library with the derived signature, and callable through `nat.call` (checked like the others)."""
    import ctypes

    assert sorted(nat.VALIDATION_FUNCTIONS) == ["gfc_gt_matches_depth", "gfc_gt_matches_homography",
                                                "gfc_gt_matches_homography_lds_bytes", "gfc_gt_project_depth",
                                                "gfc_lg_validation_metrics"]
    assert not set(nat.VALIDATION_FUNCTIONS) & set(nat.FUNCTIONS)
    with open(nat.VALIDATION_HEADER_PATH) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert funcs == nat.VALIDATION_FUNCTIONS and not structs and not enums and not consts
    assert nat.VALIDATION_SIGNATURES["gfc_gt_matches_homography_lds_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    gt = nat.VALIDATION_FUNCTIONS["gfc_gt_matches_homography"]
    assert gt[0] == "int" and len(gt[1]) == 19 and gt[1][-1] == ("stream", "void*")
    assert gt[1][4] == ("valid0", "const uint8_t*") and gt[1][15] == ("positive0", "int32_t*")
    lib = nat.lib()
    for name, (res, args) in nat.VALIDATION_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    with pytest.raises(nat.NativeError, match=r"gfc_lg_validation_metrics: 'gt_matches0' \(const int64_t\*\) is on meta"):
        nat.convert("gfc_lg_validation_metrics", [None, torch.zeros(1, 1, dtype=torch.int32, device="meta")] + [None] * 9)


def test_depth_matcher_contracts():
    from glue_factory_colon_amd import depth_matcher

    for name in ("matchers.depth_matcher", "depth_matcher", "gluefactory.models.matchers.depth_matcher"):
        assert get_model(name) is depth_matcher.DepthMatcher
    m = depth_matcher.DepthMatcher({})
    ref = {"use_points": True, "th_positive": 3.0, "th_negative": 5.0, "th_epi": None, "th_consistency": None,
           "use_lines": False, "n_line_sampled_pts": 50, "line_perp_dist_th": 5, "overlap_th": 0.2,
           "min_visibility_th": 0.5}
    assert {k: m.conf[k] for k in ref} == ref and m.conf.dense_outputs is True
    assert set(m.conf) - set(ref) - {"name", "trainable", "freeze_batch_normalization", "timeit"} == {"dense_outputs"}
    assert m.required_data_keys == ["view0", "view1", "T_0to1", "keypoints0", "keypoints1"]
    with pytest.raises(NotImplementedError, match="use_lines"):
        depth_matcher.DepthMatcher({"use_lines": True})
    with pytest.raises(NotImplementedError, match="th_consistency"):
        depth_matcher.DepthMatcher({"th_consistency": 2.0})
    with pytest.raises(NotImplementedError, match="th_positive <= th_negative"):
        depth_matcher.DepthMatcher({"dense_outputs": False, "th_positive": 6.0})
    depth_matcher.DepthMatcher({"th_epi": 5, "dense_outputs": False})
    with pytest.raises(NotImplementedError):
        m.loss({}, {})
    with pytest.raises(NotImplementedError, match="cc_th"):
        depth_matcher.gt_matches_from_pose_depth(torch.zeros(1, 1, 2), torch.zeros(1, 1, 2), {}, cc_th=1.0)
    pipe = two_view_pipeline.TwoViewPipeline({"ground_truth": {"name": "matchers.depth_matcher", "th_epi": 5}})
    assert isinstance(pipe.ground_truth, depth_matcher.DepthMatcher) and pipe.ground_truth.conf.th_epi == 5


def test_depth_fixture_cases_exercise_the_epi_rule(z):
    """With epi_th the cached / anded cases hold MORE unmatched points than without, and every point the rule moved had
    no valid depth; the dense reward changes with it."""
    for branch in ("cached", "anded"):
        n0, e0 = z[f"depth_0_{branch}_n_matches0"], z[f"depth_0_{branch}_e_matches0"]
        moved = n0 != e0
        assert moved.any() and (n0[moved] == -2).all() and (e0[moved] == -1).all()
        assert not z[f"depth_0_{branch}_valid_depth_keypoints0"][moved].any()
        assert (z[f"depth_0_{branch}_n_reward"] != z[f"depth_0_{branch}_e_reward"]).any()
        assert np.array_equal(z[f"depth_0_{branch}_n_assignment"], z[f"depth_0_{branch}_e_assignment"])
