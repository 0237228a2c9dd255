"""gfc_gt_matches_homography (csrc/gt_matches.hip) through homography_matcher, against the reference's vectors
(tests/golden/validation.npz) and, at sizes no fixture holds, against the float64 restatement tests/validation_reference.py.

Fixture cases (no verdict of theirs is within DELTA of a threshold or of another candidate, test_validation_reference_host.py;
`exact` sits on the threshold by construction, where the rule is the same in any binary arithmetic): matches0/1, assignment
and reward `torch.equal` to the reference's float32 results; the projections within DELTA = 2e-3 px of the reference's
float64 ones, the bound this suite uses for a float32 projection of coordinates below 4096 (tests/hpatches_reference.py;
measured worst on an MI355X: 1.0e-4 px).
Generated cases (tests/hpatches_cases.py): the restatement marks which verdicts are undecided; asserted on the CPU side
first that at most 1 % of the key points (the cap of test_gpu_eval_homography.py) and at most 1e-4 of the dense
elements are (a dense element is undecided when its distance is within 2e-3 px of a threshold: about 4e-7 of uniform
pairs in 640 x 480, so 1e-4 leaves room for the near-duplicates the cases hold); every other value must be equal.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpatches_cases as hc  # noqa: E402
import validation_reference as vr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd.homography_matcher import HomographyMatcher, gt_matches_from_homography  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024
KEYS8 = {"assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0"}


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "validation.npz"))


def fixture_case(z, name):
    t = lambda k: torch.from_numpy(z[f"gt_{name}_{k}"])  # noqa: E731
    pos, neg = (float(v) for v in z[f"gt_{name}_th"])
    data = {"keypoints0": t("kp0")[None].cuda(), "keypoints1": t("kp1")[None].cuda(), "H_0to1": t("H")[None].cuda()}
    if f"gt_{name}_valid0" in z.files:
        data["valid_depth_keypoints0"], data["valid_depth_keypoints1"] = t("valid0")[None].cuda(), t("valid1")[None].cuda()
    return data, pos, neg


@pytest.mark.parametrize("name", ["exact", "130x67", "twins", "masks", "65x1", "1x65"])
def test_fixture_cases_equal_the_reference(z, name):
    data, pos, neg = fixture_case(z, name)
    assert (name in ("twins", "masks")) == (pos < neg)
    out = HomographyMatcher({"th_positive": pos, "th_negative": neg}).eval()(data)
    torch.cuda.synchronize()
    assert set(out) == KEYS8 and out["assignment"].dtype == torch.bool and out["matches0"].dtype == torch.long
    for k in ("matches0", "matches1", "assignment", "reward"):
        assert torch.equal(out[k][0].cpu(), torch.from_numpy(z[f"gt_{name}_{k}"])), (name, k)
    for k in ("proj_0to1", "proj_1to0"):
        err = float((out[k][0].cpu().double() - torch.from_numpy(z[f"gt_{name}_{k}_f64"])).abs().max())
        print(name, k, "max |d proj|", err)
        assert err <= vr.DELTA, (name, k, err)
    for s in ("0", "1"):
        assert torch.equal(out["matching_scores" + s], (out["matches" + s] > -1).float())
    sparse = HomographyMatcher({"th_positive": pos, "th_negative": neg, "dense_outputs": False}).eval()(data)
    assert set(sparse) == KEYS8 - {"assignment", "reward"}
    for k in sparse:
        assert torch.equal(sparse[k], out[k]), (name, k)


def run(case, pos, neg, dense, v0=None, v1=None):
    out = gt_matches_from_homography(case["kp0"].cuda(), case["kp1"].cuda(), case["H"].cuda(), pos, neg,
                                     None if v0 is None else v0.cuda(), None if v1 is None else v1.cuda(), dense=dense)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_generated(name, case, pos, neg, dense, v0=None, v1=None):
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    refs = []
    for i in range(b):  # before the kernel's answer is looked at
        r = vr.gt_matches_homography(case["kp0"][i].double(), case["kp1"][i].double(), case["H"][i].double(), pos, neg,
                                     None if v0 is None else v0[i], None if v1 is None else v1[i])
        share = (int(r["undecided0"].sum()) + int(r["undecided1"].sum())) / (m + n)
        dense_share = float(r["undecided_dense"].float().mean())
        assert share <= 0.01 and dense_share <= 1e-4, ("bad input: too many undecided", share, dense_share)
        refs.append(r)
    out = run(case, pos, neg, dense, v0, v1)
    for i, r in enumerate(refs):
        for k, und in (("matches0", r["undecided0"]), ("matches1", r["undecided1"])):
            differ = out[k][i] != r[k]
            print(name, i, k, "undecided", int(und.sum()), "differ", int(differ.sum()))
            assert not bool((differ & ~und).any()), (name, i, k, torch.nonzero(differ & ~und).flatten()[:10])
        for k in ("proj_0to1", "proj_1to0"):
            assert float((out[k][i].double() - r[k]).abs().max()) <= vr.DELTA
        if dense:
            sure = ~r["undecided_dense"]
            assert torch.equal(out["assignment"][i][sure], r["assignment"][sure]), (name, i)
            assert torch.equal(out["reward"][i][sure].double(), r["reward"][sure]), (name, i)
    return out


def test_batch_of_two_at_the_evaluation_size_sparse():
    case = hc.metric_case(1, 2, 2048, 2048)
    out = check_generated("2048x2048", case, 3.0, 5.0, dense=False)
    # (2048 points in 640 x 480 leave no point 5 px from every other: no -1 here; the smaller cases have all three)
    assert (out["matches0"] > -1).any() and (out["matches0"] == -2).any() and set(out) == KEYS8 - {"assignment", "reward"}


@pytest.mark.parametrize("m,n", [(300, 257), (1025, 1023)])
def test_dense_outputs_and_a_pair_alone_equals_the_pair_in_a_batch(m, n):
    """Row lengths that are no multiple of 64; masks with an all-invalid row set; th_positive > th_negative, which only
    the dense path admits: there a row can be positive in `assignment` and unmatched in `matches0`."""
    b = 2 if m == 300 else 1
    case = hc.metric_case(4, b, m, n)
    g = torch.Generator().manual_seed(5)
    v0, v1 = torch.rand((b, m), generator=g) > 0.1, torch.rand((b, n), generator=g) > 0.1
    v0[:, 20:40] = False
    for pos, neg in ((3.0, 5.0), (3.0, 3.0), (3.0, 1.0)):
        out = check_generated(f"dense_{m}x{n}_{pos}_{neg}", case, pos, neg, dense=True, v0=v0, v1=v1)
        assert (out["matches0"][:, 20:40] == -2).all() and not out["assignment"][:, 20:40].any()
        rows = out["assignment"].any(2)
        assert torch.equal(rows & (out["matches0"] > -1), out["matches0"] > -1)
        if pos > neg:
            assert bool((rows & (out["matches0"] == -1)).any())  # negative overrides positive in matches only
        else:
            assert torch.equal(rows, out["matches0"] > -1)
        for i in range(b):  # one pair at a time: bit for bit the row of the batch
            one = run({k: v[i:i + 1] for k, v in case.items()}, pos, neg, True, v0[i:i + 1], v1[i:i + 1])
            for k in out:
                assert torch.equal(one[k][0], out[k][i]), (k, i)


@pytest.mark.parametrize("m,n", [(1560, 1560), (1561, 1560)])
def test_both_sides_of_64_kb_of_dynamic_lds(m, n):
    lds = nat.lib().gfc_gt_matches_homography_lds_bytes(m, n)
    assert (lds <= 64 * 1024) == ((m, n) == (1560, 1560))
    check_generated(f"{m}x{n}", hc.metric_case(2, 1, m, n), 3.0, 3.0, dense=False)


def test_largest_admitted_shape_and_the_next_one_refused():
    lds_bytes = nat.lib().gfc_gt_matches_homography_lds_bytes
    m, n = 3901, 3900
    assert lds_bytes(m, n) <= LDS_LIMIT < lds_bytes(m, n + 1) and lds_bytes(m + 1, n) > LDS_LIMIT
    check_generated(f"limit_{m}x{n}", hc.metric_case(1, 1, m, n), 3.0, 3.0, dense=False)
    case = hc.metric_case(1, 1, m, n + 1)  # one more key point: refused by the launcher's arithmetic, nothing launched
    with pytest.raises(nat.NativeError, match="UNSUPPORTED"):
        gt_matches_from_homography(case["kp0"].cuda(), case["kp1"].cuda(), case["H"].cuda(), 3.0, 3.0, dense=False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("m,n", [(0, 67), (130, 0), (0, 0)])
def test_an_empty_side_is_the_early_return_of_the_reference(m, n):
    case = hc.metric_case(2, 2, 130, 67)
    out = gt_matches_from_homography(case["kp0"][:, :m].cuda(), case["kp1"][:, :n].cuda(), case["H"].cuda(), 3.0, 3.0)
    assert set(out) == KEYS8
    assert out["matches0"].shape == (2, m) and out["matches1"].shape == (2, n)
    assert (out["matches0"] == -1).all() and (out["matches1"] == -1).all()
    assert out["assignment"].shape == (2, m, n) and out["assignment"].dtype == torch.bool and out["reward"].shape == (2, m, n)
    assert out["proj_0to1"].shape == (2, m, 2) and out["proj_1to0"].shape == (2, n, 2)
    assert not out["matching_scores0"].any() and not out["matching_scores1"].any()
    # the entry itself: NULL for everything an empty side has no array for; what exists is set to -1, nothing else
    H = case["H"].cuda()
    m0 = torch.full((2, m), 7, dtype=torch.long, device="cuda") if m else None
    m1 = torch.full((2, n), 7, dtype=torch.long, device="cuda") if n else None
    pos0 = torch.full((2, m), 7, dtype=torch.int32, device="cuda") if m else None
    nat.call("gfc_gt_matches_homography", None, None, H, H, None, None, 2, m, n, 3.0, 3.0, m0, m1, None, None, pos0, None,
             None, device=H.device)
    for t in (m0, m1, pos0):
        assert t is None or bool((t == -1).all())
    if m:
        with pytest.raises(nat.NativeError, match="INVALID"):
            nat.call("gfc_gt_matches_homography", None, None, H, H, None, None, 2, m, n, 3.0, 3.0, None, None, None, None,
                     None, None, None, device=H.device)


# ---- the depth matcher: the pose_depth.npz geometry, epi_th None and 5, the three ways the depth arrives ----------------
DEPTH_KEYS = {"assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0",
              "depth_keypoints1", "proj_0to1", "proj_1to0", "visible0", "visible1"}
CAM_WIDTH = {"PINHOLE": 6, "RADIAL": 8, "OPENCV": 10, "OPENCV_FISHEYE": 10}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "pose_depth.npz"))


def depth_data(fx, z, c, branch):
    from glue_factory_colon_amd import geometry

    t = lambda k: torch.from_numpy(fx[k][c:c + 1]).cuda()  # noqa: E731
    model = str(fx["models"][c])
    cam = lambda k: geometry.Camera(t(k)[..., :CAM_WIDTH[model]].contiguous(), model=model)  # noqa: E731
    data = {"keypoints0": t("kp0"), "keypoints1": t("kp1"), "T_0to1": geometry.Pose(t("T_0to1")),
            "view0": {"camera": cam("cam0"), "depth": t("depth0")}, "view1": {"camera": cam("cam1"), "depth": t("depth1")}}
    if branch != "sampled":
        for s in "01":
            data["valid_depth_keypoints" + s] = torch.from_numpy(z[f"depth_{c}_{branch}_valid_depth_keypoints{s}"])[None].cuda()
    if branch == "cached":
        data["depth_keypoints0"], data["depth_keypoints1"] = t("depth_kp0"), t("depth_kp1")
    return data


@pytest.mark.parametrize("c,branch", [(0, "sampled"), (0, "cached"), (0, "anded"), (1, "sampled"), (2, "sampled")])
@pytest.mark.parametrize("tag,epi_th", [("n", None), ("e", 5.0)])
def test_depth_matcher_equals_the_reference(fx, z, c, branch, tag, epi_th):
    """The reference's float32 and float64 results agree on every stored value of these cases (the generator asserts
    it), and the pose fixture holds no value within a rounding error of a decision: all must be equal."""
    from glue_factory_colon_amd.depth_matcher import DepthMatcher

    data = depth_data(fx, z, c, branch)
    out = DepthMatcher({"th_positive": 3.0, "th_negative": 5.0, "th_epi": epi_th}).eval()(data)
    torch.cuda.synchronize()
    assert set(out) == DEPTH_KEYS and out["assignment"].dtype == torch.bool and out["visible0"].dtype == torch.bool
    for k in ("matches0", "matches1", "assignment", "reward", "visible0", "visible1"):
        want = torch.from_numpy(z[f"depth_{c}_{branch}_{tag}_{k}"])
        differ = int((out[k][0].cpu() != want).sum())
        print(c, branch, tag, k, "differ", differ)
        assert differ == 0, (c, branch, tag, k, differ)
    if branch == "sampled":  # the projections are those of the pose fixture, under the bound of tests/test_gpu_eval_pose.py
        for k in ("proj_0to1", "proj_1to0"):
            got, want = out[k][0].cpu().double().numpy(), fx[k + "_f64"][c]
            assert np.array_equal(np.isnan(got), np.isnan(want))
            fin = np.isfinite(want) & (np.abs(want) < 4096)
            assert np.abs(got[fin] - want[fin]).max() <= vr.DELTA
    sparse = DepthMatcher({"th_positive": 3.0, "th_negative": 5.0, "th_epi": epi_th, "dense_outputs": False}).eval()(data)
    assert set(sparse) == DEPTH_KEYS - {"assignment", "reward"}
    for k in ("matches0", "matches1", "visible0", "visible1"):
        assert torch.equal(sparse[k], out[k]), k
    if tag == "e" and branch != "sampled":  # the rule did something here: more unmatched points than without it
        n_without = int((torch.from_numpy(z[f"depth_{c}_{branch}_n_matches0"]) == -1).sum())
        assert int((out["matches0"] == -1).sum()) > n_without


def test_depth_matcher_batch_equals_the_pairs_alone_and_an_empty_side(fx, z):
    from glue_factory_colon_amd import geometry
    from glue_factory_colon_amd.depth_matcher import DepthMatcher

    gt = DepthMatcher({"th_epi": 5.0}).eval()
    one = depth_data(fx, z, 0, "sampled")
    alone = gt(one)
    rep = lambda v: torch.cat([v, v.flip(1) if v.dim() == 3 and v.shape[-1] == 2 else v], 0)  # noqa: E731
    two = {"keypoints0": rep(one["keypoints0"]), "keypoints1": rep(one["keypoints1"]),
           "T_0to1": geometry.Pose(one["T_0to1"]._data.repeat(2, 1)),
           "view0": {"camera": geometry.Camera(one["view0"]["camera"]._data.repeat(2, 1), model="PINHOLE"),
                     "depth": one["view0"]["depth"].repeat(2, 1, 1)},
           "view1": {"camera": geometry.Camera(one["view1"]["camera"]._data.repeat(2, 1), model="PINHOLE"),
                     "depth": one["view1"]["depth"].repeat(2, 1, 1)}}
    both = gt(two)
    for k in alone:
        a, b = alone[k][0], both[k][0]
        assert torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) if a.is_floating_point() else torch.equal(a, b), k
    assert not torch.equal(both["matches0"][1], both["matches0"][0])  # the second pair is another pair
    empty = gt({**one, "keypoints1": one["keypoints1"][:, :0]})
    assert set(empty) == DEPTH_KEYS and (empty["matches0"] == -1).all() and empty["matches1"].shape == (1, 0)
    assert not empty["visible0"].any() and empty["assignment"].shape == (1, 257, 0)
    assert empty["depth_keypoints0"].shape == (1, 257) and empty["proj_1to0"].shape == (1, 0, 2)
