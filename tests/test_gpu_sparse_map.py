"""gfc_gt_matches_sparse_map (csrc/gt_sparse_map.hip) and the two matchers built on it, against the reference's vectors
(tests/golden/sparse_map.npz, made by the reference's own two functions) and, at sizes no fixture holds, against the
float64 restatement tests/sparse_map_reference.py.

Fixture cases: no verdict of theirs is within DELTA = 2e-3 px of a threshold or of another candidate (the generator walks
seeds until the restatement flags nothing), so every integer, mask, assignment and reward must be EQUAL to the
reference's float32 results; only the projections are floats, within DELTA of the reference's float64 ones (the bound of
tests/test_gpu_gt_matchers.py for a float32 projection of coordinates below 4096).
Generated cases (sparse_map_reference.entry_case): the restatement marks which verdicts are undecided; asserted on the CPU
side first that at most 1 % of the key points are (the cap of tests/test_gpu_gt_matchers.py) and at most 2 x 1 % + 1e-4
of the dense elements: a dense element is undecided when a distance of it lies within 2e-3 px of a threshold (the 1e-4
of that test) or, with th_epi, when the point of its row or of its column is (whether the point is `ignore` masks the
whole row or column); every other value must be equal.
Sizes: the launcher uses 16 key points per workgroup, 16 lanes per key point and tiles of 256 elements, so the shapes
sit one below, at and one above 16 and 256 (15, 16, 17, 255, 256, 257) and above 16 x 256; the finishing launch has 256
threads per workgroup over the M + N key points of a pair: M + N = 255, 256, 257 (127 + 128, 128 + 128, 127 + 130) and
511, 512, 513 (255 + 256, 255 + 257, 256 + 257) are among the shapes.
The pipeline tests run `ValidationPipeline` and the command line on the generated tree of tests/endomapper_reference.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_map_reference as sr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((3.0, 5.0, None, False), (None, 10.0, None, True), (3.0, 5.0, 5.0, True), (None, None, None, True),
            (6.0, 5.0, None, True))
KEYS20 = {"assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "depth_keypoints0",
          "depth_keypoints1", "proj_0to1", "proj_1to0", "visible0", "visible1"} | {k + s for k in sr.MASK_KEYS for s in "01"}
KP_CAP, DENSE_CAP = 0.01, 2 * 0.01 + 1e-4
CAM_WIDTH = {"PINHOLE": 6, "RADIAL": 8, "OPENCV": 10, "OPENCV_FISHEYE": 10}


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "sparse_map.npz"))


def none(v):
    return -1.0 if v is None else float(v)


def run_entry(case, pos, neg, epi, use_ids=True, dense=False, masks=True, short=0, v3d=True):
    """The entry on an entry_case -> CPU tensors.  short: bytes the workspace is too small by."""
    c = {k: v.cuda().contiguous() for k, v in case.items()}
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    dev = c["kp0"].device
    out = {"matches0": torch.full((b, m), 7, dtype=torch.long, device=dev),
           "matches1": torch.full((b, n), 7, dtype=torch.long, device=dev),
           "masks0": torch.full((b, 4, m), 7, dtype=torch.uint8, device=dev) if masks else None,
           "masks1": torch.full((b, 4, n), 7, dtype=torch.uint8, device=dev) if masks else None,
           "positive0": torch.full((b, m), 7, dtype=torch.int32, device=dev),
           "extra_positives": torch.full((b,), 7, dtype=torch.int32, device=dev),
           "assignment": torch.full((b, m, n), 7, dtype=torch.uint8, device=dev) if dense else None,
           "reward": torch.full((b, m, n), 7.0, device=dev) if dense else None}
    nbytes = nat.call("gfc_gt_matches_sparse_map_workspace_bytes", b, m, n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    ids = (c["ids0"], c["ids1"], c["v3d0"] if v3d else None, c["v3d1"] if v3d else None) if use_ids else (None,) * 4
    nat.call("gfc_gt_matches_sparse_map", c["kp0"], c["kp1"], c["p01"], c["p10"], c["vis0"], c["vis1"], c["valid0"],
             c["valid1"], *ids, c["F"], b, m, n, none(pos), none(neg), none(epi), out["matches0"], out["matches1"],
             out["masks0"], out["masks1"], out["positive0"], out["extra_positives"], out["assignment"], out["reward"], ws,
             nbytes - short, device=dev)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items() if v is not None}


def check_entry(name, case, pos, neg, epi, use_ids=True, dense=False):
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    refs = []
    for i in range(b):  # before the kernel's answer is looked at
        r = sr.labels_of(case, i, pos, neg, epi, use_ids)
        share = (int(r["undecided0"].sum()) + int(r["undecided1"].sum())) / (m + n)
        dense_share = float(r["undecided_dense"].float().mean())
        assert share <= KP_CAP and dense_share <= DENSE_CAP, ("bad input: too many undecided", name, share, dense_share)
        assert r["extra_positives"] == r["extra_positives_dense"]
        refs.append(r)
    out = run_entry(case, pos, neg, epi, use_ids, dense)
    for i, r in enumerate(refs):
        und = {"0": r["undecided0"], "1": r["undecided1"]}
        for s in "01":
            differ = out["matches" + s][i] != r["matches" + s]
            print(name, i, "matches" + s, "undecided", int(und[s].sum()), "differ", int(differ.sum()))
            assert not bool((differ & ~und[s]).any()), (name, i, s, torch.nonzero(differ & ~und[s]).flatten()[:10])
            for q, key in enumerate(sr.MASK_KEYS):
                bad = (out["masks" + s][i, q].bool() != r[key + s]) & ~und[s]
                assert not bool(bad.any()), (name, i, key + s, torch.nonzero(bad).flatten()[:10])
        bad = (out["positive0"][i].long() != r["positive0"]) & ~und["0"]
        assert not bool(bad.any()), (name, i, "positive0")
        if not bool(und["0"].any()):
            assert int(out["extra_positives"][i]) == r["extra_positives"], (name, i)
        if dense:
            sure = ~r["undecided_dense"]
            assert torch.equal(out["assignment"][i].bool()[sure], r["assignment"][sure]), (name, i)
            assert torch.equal(out["reward"][i][sure].double(), r["reward"][sure]), (name, i)
    return out, refs


# ---- the reference's vectors through the two matchers -------------------------------------------------------------------
def fixture_data(z, c, sparse):
    from glue_factory_colon_amd import geometry

    t = lambda k: torch.from_numpy(z[f"c{c}_{k}"])[None].cuda()  # noqa: E731
    model = str(z[f"c{c}_model"])
    cam = lambda k: geometry.Camera(t(k)[..., :CAM_WIDTH[model]].contiguous(), model=model)  # noqa: E731
    data = {"keypoints0": t("kp0"), "keypoints1": t("kp1"), "T_0to1": geometry.Pose(t("T")),
            "view0": {"camera": cam("cam0")}, "view1": {"camera": cam("cam1")}}
    if sparse:
        data.update({"sparse_depth0": t("d0"), "sparse_depth1": t("d1"), "valid_depth_mask0": t("valid0"),
                     "valid_depth_mask1": t("valid1"), "point3D_ids0": t("ids0"), "point3D_ids1": t("ids1"),
                     "valid_3D_mask0": t("v3d0"), "valid_3D_mask1": t("v3d1")})
    else:
        data.update({"depth_keypoints0": t("d0"), "depth_keypoints1": t("d1"), "valid_depth_keypoints0": t("valid0"),
                     "valid_depth_keypoints1": t("valid1"), "point3D_ids0": t("ids0"), "point3D_ids1": t("ids1")})
    return data


@pytest.mark.parametrize("c", range(5))
@pytest.mark.parametrize("sparse", [True, False])
def test_matchers_equal_the_reference(z, c, sparse):
    from glue_factory_colon_amd.registry import get_model

    name = "sparse_depth_matcher" if sparse else "sparse_dense_depth_matcher"
    data = fixture_data(z, c, sparse)
    m, n = data["keypoints0"].shape[1], data["keypoints1"].shape[1]
    for s, (pos, neg, epi, use) in enumerate(SETTINGS):
        assert tuple(z["settings"][s]) == (none(pos), none(neg), none(epi), float(use))
        conf = {"th_positive": pos, "th_negative": neg, "th_epi": epi, "use_gt_pos": use}
        out = get_model("matchers." + name)(conf).eval()(data)
        torch.cuda.synchronize()
        assert set(out) == KEYS20 and out["assignment"].dtype == torch.bool and out["mask_neg_epi0"].dtype == torch.bool
        tag = f"c{c}_{'s' if sparse else 'd'}{s}_"
        for k in ("matches0", "matches1", "visible0", "visible1") + tuple(k + q for k in sr.MASK_KEYS for q in "01"):
            differ = int((out[k][0].cpu() != torch.from_numpy(z[tag + k])).sum())
            assert differ == 0, (tag, k, differ)
        want = np.unpackbits(z[tag + "assignment"])[:m * n].reshape(m, n).astype(bool)
        assert np.array_equal(out["assignment"][0].cpu().numpy(), want), tag
        assert np.array_equal(out["reward"][0].cpu().numpy(), z[tag + "reward"].astype(np.float32)), tag
        for k in ("proj_0to1", "proj_1to0"):
            got, ref = out[k][0].cpu().double().numpy(), z[f"c{c}_{k}_f64"]
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            fin = np.isfinite(ref) & (np.abs(ref) < 4096)
            err = np.abs(got[fin] - ref[fin]).max()
            print(tag, k, "max |d proj|", err)
            assert err <= sr.DELTA
        assert torch.equal(out["depth_keypoints0"], data["sparse_depth0" if sparse else "depth_keypoints0"])
        for q in "01":
            assert torch.equal(out["matching_scores" + q], (out["matches" + q] > -1).float())
        lean = get_model(name)({**conf, "dense_outputs": False}).eval()(data)
        assert set(lean) == (KEYS20 - {"assignment", "reward"}) | {"extra_positives"}
        for k in set(lean) - {"extra_positives"}:
            assert torch.equal(lean[k].nan_to_num(nan=-7.0), out[k].nan_to_num(nan=-7.0)) if lean[k].is_floating_point() \
                else torch.equal(lean[k], out[k]), (tag, k)
        cols = torch.arange(n, device="cuda")[None]
        dense_extra = int((out["assignment"][0] & (cols != out["matches0"][0][:, None])).sum())
        assert lean["extra_positives"].dtype == torch.int32 and int(lean["extra_positives"][0]) == dense_extra, tag
        if sparse and use and c < 3:
            assert dense_extra > 0  # the duplicate ids: positives `matches0` cannot name
        if not (sparse and use):
            assert not out["mask_pos_3d_map0"].any() and dense_extra == 0


def test_refusals_and_missing_keys(z):
    from glue_factory_colon_amd.sparse_dense_depth_matcher import SparseDenseDepthMatcher
    from glue_factory_colon_amd.sparse_depth_matcher import SparseDepthMatcher

    data = fixture_data(z, 0, False)
    for k in ("depth_keypoints1", "valid_depth_keypoints0"):
        with pytest.raises(ValueError, match="Only working with cached features"):
            SparseDenseDepthMatcher({}).eval()({q: v for q, v in data.items() if q != k})
    with pytest.raises(AssertionError, match="Missing key sparse_depth0"):
        SparseDepthMatcher({}).eval()(data)


# ---- the entry against the restatement, and against the one-workgroup kernel --------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 1), (15, 17), (16, 16), (17, 15), (127, 128), (128, 128), (127, 130), (255, 256),
                                 (255, 257), (256, 256), (257, 255), (256, 257), (300, 4097)])
def test_block_and_tile_edges(m, n):
    case = sr.entry_case(3, 1, m, n, twins=True)
    check_entry(f"{m}x{n}", case, 3.0, 5.0, 5.0, dense=m * n < 70000)
    check_entry(f"{m}x{n}_none", case, None, 10.0, None)


def test_1025x1023_dense():
    case = sr.entry_case(4, 1, 1025, 1023, twins=True)
    for pos, neg, epi in ((3.0, 5.0, None), (6.0, 5.0, 5.0), (None, None, None)):
        out, refs = check_entry(f"1025x1023_{pos}_{neg}_{epi}", case, pos, neg, epi, dense=True)
        rows = out["assignment"][0].bool().any(1)
        assert torch.equal(rows & (out["matches0"][0] > -1), rows)  # a positive is never overridden
    assert int(out["extra_positives"][0]) >= 5  # the 3 x 2 duplicate block alone loses five


def test_batch_of_two_at_the_evaluation_size():
    case = sr.entry_case(1, 2, 2048, 2048, twins=True)
    out, _ = check_entry("2x2048x2048", case, None, 10.0, None)
    assert (out["matches0"] > -1).any() and (out["matches0"] == -2).any()
    check_entry("2x2048x2048_epi", case, 3.0, 5.0, 5.0)


def test_a_shape_the_one_workgroup_kernels_refuse():
    m, n = 4000, 3900
    assert nat.lib().gfc_gt_matches_homography_lds_bytes(m, n) > 160 * 1024
    check_entry("4000x3900", sr.entry_case(2, 1, m, n, twins=True), 3.0, 5.0, 5.0)


@pytest.mark.parametrize("m,n", [(300, 257), (2048, 2048)])
def test_ties_resolve_to_the_first_index(m, n):
    """Bit-identical twins on both sides and twin ids (entry_case twins=True): rows 2, m//2, m-3 are one point, columns
    5, n//3, n-1 are one point; ids 99 join rows {2, m-3} and columns {5, n//3, n-1}."""
    case = sr.entry_case(6, 1, m, n, twins=True)
    case["vis0"][:, [2, m // 2, m - 3]] = True
    case["vis1"][:, [5, n // 3, n - 1]] = True
    out = run_entry(case, 3.0, 5.0, None, use_ids=False)
    r = sr.labels_of(case, 0, 3.0, 5.0, None, use_ids=False)
    for s, twins in (("0", [2, m // 2, m - 3]), ("1", [5, n // 3, n - 1])):
        sure = ~r["undecided" + s]
        assert torch.equal(out["matches" + s][0][sure], r["matches" + s][sure])
        got = out["matches" + s][0][twins]
        assert got[0] == got[1] == got[2] or (got[1:] < 0).all()  # one partner for all, or only the first twin matched
    # a column whose nearest row is the twin point names the FIRST twin
    named = out["matches1"][0][out["matches1"][0] > -1]
    assert not bool(((named == m // 2) | (named == m - 3)).any())
    seeded = run_entry(case, None, None, None)
    assert seeded["matches0"][0][2] == 5 and seeded["matches0"][0][m - 3] == 5
    assert seeded["matches1"][0][5] == 2 and seeded["matches1"][0][n // 3] == 2 and seeded["matches1"][0][n - 1] == 2


@pytest.mark.parametrize("epi", [None, 5.0])
def test_without_ids_equals_the_one_workgroup_kernel(epi):
    """ids null and pos_th <= neg_th: matches0/1 and positive0 are those of gfc_gt_matches_depth on the same inputs
    (a negative cannot be positive there, so the two precedence rules coincide)."""
    case = sr.entry_case(8, 3, 1025, 1023, twins=True)
    mine = run_entry(case, 3.0, 5.0, epi, use_ids=False)
    c = {k: v.cuda().contiguous() for k, v in case.items()}
    b, m, n = 3, 1025, 1023
    m0, m1 = torch.empty((b, m), dtype=torch.long, device="cuda"), torch.empty((b, n), dtype=torch.long, device="cuda")
    pos0 = torch.empty((b, m), dtype=torch.int32, device="cuda")
    nat.call("gfc_gt_matches_depth", c["kp0"], c["kp1"], c["p01"], c["p10"], c["vis0"], c["vis1"], c["valid0"],
             c["valid1"], c["F"], b, m, n, 3.0, 5.0, none(epi), m0, m1, pos0, None, None, device=m0.device)
    torch.cuda.synchronize()
    assert torch.equal(mine["matches0"], m0.cpu()) and torch.equal(mine["matches1"], m1.cpu())
    assert torch.equal(mine["positive0"], pos0.cpu())
    assert (m0 > -1).any() and (m0 == -1).any() and (m0 == -2).any()


def run_depth(case):
    """gfc_gt_matches_depth (one workgroup per pair) at pos_th 3, neg_th 5, no epi_th -> CPU tensors."""
    c = {k: v.cuda().contiguous() for k, v in case.items()}
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    out = {"matches0": torch.full((b, m), 7, dtype=torch.long, device="cuda"),
           "matches1": torch.full((b, n), 7, dtype=torch.long, device="cuda"),
           "positive0": torch.full((b, m), 7, dtype=torch.int32, device="cuda")}
    nat.call("gfc_gt_matches_depth", c["kp0"], c["kp1"], c["p01"], c["p10"], c["vis0"], c["vis1"], c["valid0"],
             c["valid1"], None, b, m, n, 3.0, 5.0, -1.0, out["matches0"], out["matches1"], out["positive0"], None, None,
             device=c["kp0"].device)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def run_roma(case):
    """gfc_gt_matches_roma on the projections of an entry_case: every key point valid with certainty 1 and cycle error 0,
    pos_th 3, neg_th 5, none of the four optional thresholds -> CPU tensors."""
    c = {k: v.cuda().contiguous() for k, v in case.items()}
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    dev = c["kp0"].device
    side = lambda k, fill, dtype: torch.full((b, k), fill, dtype=dtype, device=dev)  # noqa: E731
    out = {"matches0": side(m, 7, torch.long), "matches1": side(n, 7, torch.long)}
    nbytes = nat.call("gfc_gt_matches_roma_workspace_bytes", b, m, n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    nat.call("gfc_gt_matches_roma", c["kp0"], c["kp1"], c["p01"], c["p10"], side(m, 1.0, torch.float32),
             side(n, 1.0, torch.float32), side(m, 0.0, torch.float32), side(n, 0.0, torch.float32),
             side(m, 1, torch.uint8), side(n, 1, torch.uint8), b, m, n, 3.0, 5.0, -1.0, -1.0, -1.0, -1.0, out["matches0"],
             out["matches1"], side(m, 7.0, torch.float32), side(n, 7.0, torch.float32), None, None, None, None, ws, nbytes,
             device=dev)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def test_the_three_labellers_agree_where_their_rules_coincide():
    """No ids, pos_th 3 <= neg_th 5, no th_epi: the split sparse-map labeller and the one-workgroup depth labeller state
    one rule, and with every key point visible and valid the RoMa labeller (certainty 1, cycle error 0, no optional
    threshold) states it too.  The three evaluate the same float32 expressions, so the labels are EQUAL.  Shapes one off
    the 16 owned key points, the tile of 256 and the stride of 16 x 256, on either side."""
    cases = [sr.entry_case(seed, b, m, n) for seed, b, m, n in
             ((11, 2, 17, 255), (12, 2, 257, 16), (13, 1, 300, 513), (14, 1, 1, 1), (15, 2, 15, 4097))]
    ones = [{**c, **{k: torch.ones_like(c[k]) for k in ("vis0", "vis1", "valid0", "valid1")}} for c in cases]
    for name, group in (("own", cases), ("all-visible", ones)):  # before any kernel's answer is looked at
        kinds = {"0": set(), "1": set()}
        for c in group:
            for i in range(c["kp0"].shape[0]):
                r = sr.labels_of(c, i, 3.0, 5.0, None, use_ids=False)
                assert not bool(r["undecided0"].any()) and not bool(r["undecided1"].any()), ("bad input", name)
                for s in "01":
                    kinds[s] |= set(r["matches" + s].clamp(max=0).tolist())
        print(name, kinds)
        assert kinds["0"] == kinds["1"] == {0, -1, -2}, ("bad input: a label kind is missing", name, kinds)
    for c, o in zip(cases, ones):
        split, one_wg = run_entry(c, 3.0, 5.0, None, use_ids=False), run_depth(c)
        for k in ("matches0", "matches1", "positive0"):
            assert torch.equal(split[k], one_wg[k]), (c["kp0"].shape, c["kp1"].shape, k)
        split, one_wg, roma = run_entry(o, 3.0, 5.0, None, use_ids=False), run_depth(o), run_roma(o)
        for k in ("matches0", "matches1"):
            assert torch.equal(split[k], one_wg[k]) and torch.equal(split[k], roma[k]), (c["kp0"].shape, c["kp1"].shape, k)
        assert torch.equal(split["positive0"], one_wg["positive0"])


def test_a_pair_alone_equals_the_pair_in_a_batch_of_six():
    case = sr.entry_case(9, 6, 300, 257, twins=True)
    both = run_entry(case, 3.0, 5.0, 5.0, dense=True)
    for i in (0, 3, 5):
        one = run_entry({k: v[i:i + 1] for k, v in case.items()}, 3.0, 5.0, 5.0, dense=True)
        for k in both:
            assert torch.equal(one[k][0], both[k][i]), (k, i)
    assert not torch.equal(both["matches0"][0], both["matches0"][5])


def test_null_inputs_an_empty_side_and_a_short_workspace():
    case = sr.entry_case(10, 2, 130, 67)
    full = run_entry(case, 3.0, 5.0, 5.0)
    lean = run_entry(case, 3.0, 5.0, 5.0, masks=False)
    for k in lean:
        assert torch.equal(lean[k], full[k]), k
    all_valid = {**case, "v3d0": torch.ones_like(case["v3d0"]), "v3d1": torch.ones_like(case["v3d1"])}
    a, b = run_entry(all_valid, 3.0, 5.0, None), run_entry(case, 3.0, 5.0, None, v3d=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k  # valid3d null = all valid
    # one byte short: refused, nothing launched, nothing written
    c = {k: v.cuda() for k, v in case.items()}
    nbytes = nat.call("gfc_gt_matches_sparse_map_workspace_bytes", 2, 130, 67)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    m0 = torch.full((2, 130), 7, dtype=torch.long, device="cuda")
    m1 = torch.full((2, 67), 7, dtype=torch.long, device="cuda")
    args = lambda size, F=c["F"], i1=c["ids1"]: (  # noqa: E731
        c["kp0"], c["kp1"], c["p01"], c["p10"], c["vis0"], c["vis1"], c["valid0"], c["valid1"], c["ids0"], i1, None, None,
        F, 2, 130, 67, 3.0, 5.0, 5.0, m0, m1, None, None, None, None, None, None, ws, size)
    with pytest.raises(nat.NativeError, match="WORKSPACE"):
        nat.call("gfc_gt_matches_sparse_map", *args(nbytes - 1), device=m0.device)
    with pytest.raises(nat.NativeError, match="INVALID"):  # epi_th without F
        nat.call("gfc_gt_matches_sparse_map", *args(nbytes, F=None), device=m0.device)
    with pytest.raises(nat.NativeError, match="INVALID"):  # ids are nullable together
        nat.call("gfc_gt_matches_sparse_map", *args(nbytes, i1=None), device=m0.device)
    torch.cuda.synchronize()
    assert bool((m0 == 7).all()) and bool((m1 == 7).all())
    # an empty side: no kernel, the other side unmatched, masks and extra_positives zero
    for m, n in ((0, 67), (130, 0), (0, 0)):
        side0 = {"kp0", "p01", "vis0", "valid0", "ids0", "v3d0"}
        cut = {k: (v[:, :m] if k in side0 else v[:, :n]) for k, v in case.items() if k != "F"}
        out = run_entry({**cut, "F": case["F"]}, 3.0, 5.0, 5.0, dense=True)
        assert nat.call("gfc_gt_matches_sparse_map_workspace_bytes", 2, m, n) == 0
        assert (out["matches0"] == -1).all() and (out["matches1"] == -1).all() and (out["positive0"] == -1).all()
        assert not out["masks0"].any() and not out["masks1"].any() and not out["extra_positives"].any()


# ---- the labels in the loss ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_depth_matcher", "sparse_dense_depth_matcher"])
def test_matchers_through_the_pipeline_loss(z, name):
    """Cached key points (`allow_no_extract`), LightGlue with scales and orientations, the labels in `loss`.  With
    use_gt_pos False no row has two positives (extra_positives == 0): dense_outputs true and false then give the same
    ten loss and metric values."""
    from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline

    data = fixture_data(z, 0, name == "sparse_depth_matcher")
    g = torch.Generator().manual_seed(3)
    size = torch.tensor([[128.0, 96.0]]).cuda()
    views = {}
    for s in "01":
        k = data["keypoints" + s].shape[1]
        cache = {"keypoints": data.pop("keypoints" + s),
                 "descriptors": torch.nn.functional.normalize(torch.randn((1, k, 128), generator=g), dim=-1).cuda(),
                 "scales": (1 + torch.rand((1, k), generator=g)).cuda(), "oris": (6.28 * torch.rand((1, k), generator=g)).cuda()}
        for key in list(data):
            if key.endswith(s) and key not in ("view0", "view1", "T_0to1"):
                cache[key[:-1]] = data.pop(key)
        views["view" + s] = {**data["view" + s], "image": torch.zeros((1, 1, 96, 128)).cuda(), "image_size": size,
                             "cache": cache}
    item = {**views, "T_0to1": data["T_0to1"]}
    values = []
    for dense in (True, False):
        pipe = TwoViewPipeline({"extractor": {"name": None}, "allow_no_extract": True,
                                "matcher": {"name": "matchers.lightglue", "weights": "synthetic", "filter_threshold": 0.0,
                                            "flash": False, "add_scale_ori": True, "input_dim": 128},
                                "ground_truth": {"name": "matchers." + name, "th_positive": 3.0, "th_negative": 5.0,
                                                 "dense_outputs": dense}}).eval().cuda()
        pred = pipe(item)
        losses, metrics = pipe.loss(pred, item)
        torch.cuda.synchronize()
        assert ("gt_assignment" in pred) == dense and ("gt_extra_positives" in pred) != dense
        assert len(losses) == 8 and len(metrics) == 4 and bool(torch.isfinite(losses["total"]).all())
        if not dense:
            assert int(pred["gt_extra_positives"].sum()) == 0
        assert int((pred["gt_matches0"] > -1).sum()) == int((torch.from_numpy(z["c0_s0_matches0"]) > -1).sum())
        values.append({k: float(v[0]) for k, v in {**losses, **metrics}.items() if k not in ("total", "last")})
    assert len(values[0]) == 10 and values[0] == values[1], values


# ---- the validation pass on a generated map ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import endomapper_reference as er

    tmp = tmp_path_factory.mktemp("endomapper")
    er.write_tree(tmp)
    return tmp


def test_validation_pipeline_on_a_generated_map(tree):
    """20 pairs (ten per map over the overlap bins) in chunks of 8: every pair has 64 + 64 key points and one camera model,
    so a chunk is one group -- three groups, three device-to-host reads."""
    import endomapper_reference as er
    from glue_factory_colon_amd import validate
    from glue_factory_colon_amd.endomapper import Endomapper

    ds = Endomapper(er.CONFS["ten"], tree, "val")
    bins = "0.3:0.5,0.5:0.77,0.9:1.0"
    vp = validate.ValidationPipeline(validate.endomapper_model_conf(), pair_batch=8, eval_overlap_bins=bins)
    assert not hasattr(vp.model, "extractor") and vp.model.matcher.conf.add_scale_ori and vp.model.matcher.conf.input_dim == 128
    feeder = ds.feeder("cuda", num_workers=2, batch=8)
    res = vp.run(feeder, view_key=ds.view_key)
    torch.cuda.synchronize()
    assert res["num_pairs"] == 20 and vp.reads == 3
    assert np.isfinite(res["loss/total"]) and 0.0 <= res["match_recall"] <= 1.0 and res["loss/num_matchable"] > 1
    assert isinstance(res["gt_extra_positives"], int) and res["gt_extra_positives"] >= 0
    overlaps = [float(it[3]) for it in ds.items]
    want = {name for lo, hi, name in validate.overlap_bins(bins) if any(lo <= o < hi for o in overlaps)}
    assert set(res["bins"]) == want == {"overlap_0.30_0.50", "overlap_0.50_0.77", "overlap_0.30_1.00"}  # 0.9:1.0 is empty
    assert res["bins"]["overlap_0.30_1.00"]["loss/total"] == pytest.approx(res["loss/total"], rel=1e-12)
    n_lo = sum(0.3 <= o < 0.5 for o in overlaps)
    both = (res["bins"]["overlap_0.30_0.50"]["accuracy"] * n_lo + res["bins"]["overlap_0.50_0.77"]["accuracy"] * (20 - n_lo)) / 20
    assert both == pytest.approx(res["accuracy"], rel=1e-9)
    # the feeder: a map's npz opened once per batch, a view read once per batch, unpadded views uploaded once
    assert feeder.npz_opened <= 2 * 3 and feeder.views_read < 40 and feeder.views_uploaded < 40
    # the labels of the pass are those of the matcher on the reader's own item
    item = next(iter(ds.feeder("cuda", batch=1)))
    pred = vp.model(item)
    gt = vp.model.ground_truth({**item, **pred})
    assert set(gt) >= {"matches0", "extra_positives", "mask_pos_3d_map0"} and "assignment" not in gt
    assert int((gt["matches0"] > -1).sum()) > 0 and bool(gt["mask_pos_3d_map0"].any())
    # the sparse-dense labels need depth_keypoints, which this cache does not carry: the reference's error
    dense = validate.ValidationPipeline(validate.endomapper_model_conf("sparse_dense_depth_matcher", 3.0, 5.0), pair_batch=8)
    with pytest.raises(ValueError, match="Only working with cached features"):
        dense.run(ds.feeder("cuda", batch=8))


def test_validate_command_line_on_a_generated_tree(tree, capsys):
    import endomapper_reference as er
    from glue_factory_colon_amd import validate

    res = validate.main(["--data_dir", str(tree / er.DATA_DIR), "--dataset", "endomapper", "--max_num_features", "64",
                         "--pair_batch", "64", "--eval_overlap_bins", "0.3:0.5,0.5:1.0", "--num_workers", "1"])
    out = capsys.readouterr().out
    assert res["num_pairs"] == 155 and np.isfinite(res["loss/total"]) and "gt_extra_positives" in res
    assert "num_pairs: 155" in out and "overlap_0.30_0.50:" in out and "gt_extra_positives:" in out
    assert ("fewer positives than the reference's dense assignment" in out) == (res["gt_extra_positives"] > 0)
