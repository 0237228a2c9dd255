"""The SIFT stage kernels (csrc/sift.hip) against the float64 restatement of tests/sift_reference.py.

UNPINNED against OpenCV, pycolmap and CudaSift (absent): what is held here is that the kernels compute the restatement's
algorithm.  Each stage is fed the restatement's fp32-rounded inputs, so it is judged alone:

pyramid   every Gaussian and DoG sample within the bound of sift_reference.pyramid (one level 2 (T + 2) 2^-24 max|x|, a
          chain the sum of its steps, a DoG level its two levels' bounds + 2^-24 |v|), none excused.
detect    the raw list equals the restatement's exactly in (octave, layer, y, x) and in the position after the moves;
          x, y, sigma, score within 1e-6 relative of the restatement's values rounded to fp32 (both sides compute in fp64
          on the same fp32 samples; the kernel stores fp32).
orient    equal numbers of orientations; angles within 4 x the distance between the restatement in float32 and in
          float64 on the same fixture (measured here, each run: the allowance is printed).  No key point of the fixture
          has a peak margin below 1e-4 (test_sift_reference_host.py), so none is excused.
describe  per element within 4 x the float32 / float64 distance of the restatement, none excused.
whole     the `SIFT` module along its own chain, every stage held to the tolerances above (sift_gpu_cases.py).
The comparisons themselves live in tests/sift_gpu_cases.py, shared with tools/sift_parity.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_gpu_cases as gc  # noqa: E402
import sift_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu


def _sift():
    from glue_factory_colon_amd import sift

    return sift


# ----------------------------------------------------------------------------------------------------------- pyramid
PYRAMID_CASES = gc.PYRAMID_CASES  # (why no level is narrower than a tap radius: see sift_gpu_cases.py)


@pytest.mark.parametrize("first_octave", [-1, 0])
@pytest.mark.parametrize("case", list(PYRAMID_CASES))
def test_pyramid_levels_within_the_float64_bound(case, first_octave):
    h, w, valid = PYRAMID_CASES[case]
    imgs = np.stack([gc.image(h, w, 5 + i) for i in range(len(valid))])
    worst_g, worst_d, octaves_ok = gc.pyramid_errors(_sift(), imgs, valid, first_octave, 3)
    print(f"pyramid {case} first_octave {first_octave}: worst error / bound {worst_g:.3f} (Gaussian), {worst_d:.3f} (DoG)")
    assert octaves_ok and worst_g <= 1 and worst_d <= 1  # every sample, none excused



def test_pyramid_refuses_what_it_cannot_serve():
    from glue_factory_colon_amd import _native as nat

    sift = _sift()
    img = torch.zeros(1, 15, 40).cuda()
    for args in ((img, None, 0, 3), (torch.zeros(1, 32, 40).cuda(), None, -2, 3), (torch.zeros(1, 32, 40).cuda(), None, 0, 9)):
        with pytest.raises(nat.NativeError, match="GFC_ERR_UNSUPPORTED"):
            sift.pyramid(*args)


# ------------------------------------------------------------------------------------------------------------ detect
_upload = gc.upload


def _compare_raw(ref, raw_f, raw_i, counts, b=0):
    got = gc.compare_raw(ref, raw_f, raw_i, counts, b)
    assert got["equal"], got  # (octave, layer, y, x), the position after the moves and the counts: 0 excused
    assert got["rel"] <= 1e-6, got  # against the restatement's fp64 values rounded to fp32, as the kernel stores them



@pytest.fixture(scope="module")
def detect_case():
    vol, planted = sr.detect_fixture()
    return vol, planted, sr.detect([vol], 0, sr.DETECT_THR)


def test_detect_equals_the_restatement_on_the_planted_octave(detect_case):
    sift = _sift()
    vol, planted, ref = detect_case
    h, w = sr.DETECT_SHAPE
    lay = sift.pyramid_layout(h, w, 0, 1)
    raw_f, raw_i, counts = sift.detect(_upload(sift, [vol], lay, True), h, w, None, 0, 1, sr.DETECT_THR, 10.0, cap=512)
    _compare_raw(ref, raw_f, raw_i, counts)
    ids = {tuple(r[1:4]) for r in raw_i[0, : int(counts[0, 0])].cpu().tolist()}
    for name in ("over_thr", "negative", "on_margin"):
        assert planted[name] in ids, name
    for name in ("under_0.8_thr", "over_0.8_thr", "under_thr", "tie", "tie_twin", "ridge"):
        assert planted[name] not in ids, name
    moved = raw_i[0, : int(counts[0, 0])].cpu().numpy()
    assert (np.abs(moved[:, 1:4] - moved[:, 4:7]).sum(1) > 0).sum() == ref["fates"]["moved"] >= 1


def test_detect_counts_and_reports_what_exceeds_the_cap(detect_case):
    sift = _sift()
    vol, _, ref = detect_case
    h, w = sr.DETECT_SHAPE
    lay = sift.pyramid_layout(h, w, 0, 1)
    cap = 32
    raw_f, raw_i, counts = sift.detect(_upload(sift, [vol], lay, True), h, w, None, 0, 1, sr.DETECT_THR, 10.0, cap=cap)
    assert int(counts[0, 1]) == ref["n_candidates"] > cap
    assert int(counts[0, 2]) == ref["n_candidates"] - cap  # never a silent drop
    n = int(counts[0, 0])
    assert 0 < n <= cap
    got = [tuple(r) for r in raw_i[0, :n, :4].cpu().tolist()]
    assert got == sorted(got) and set(got) <= {tuple(r) for r in ref["idx"].tolist()}


def test_detect_on_a_whole_pyramid_with_two_valid_sizes():
    """The restatement's own DoG pyramid (fp32-rounded), three octaves, first_octave -1; image 1 is smaller than the
    plane and has fewer octaves."""
    sift = _sift()
    h, w = 48, 60
    valid = [(60, 48), (41, 30)]
    imgs = np.stack([sr.textured_image(h, w, 22 + i, n=14, vignette=False) for i in range(2)])
    lay = sift.pyramid_layout(h, w, -1, 3)
    bufs, refs = [], []
    for b, (vw, vh) in enumerate(valid):
        dogs = [d.astype(np.float32) for d in sr.pyramid(imgs[b, :vh, :vw], -1, 3)["dog"]]
        refs.append(sr.detect(dogs, -1))
        bufs.append(_upload(sift, dogs, lay, True))
    assert len(sr.octave_sizes(30, 41, -1, 3)) == 2 and min(len(r["idx"]) for r in refs) > 3
    raw_f, raw_i, counts = sift.detect(torch.cat(bufs), h, w, torch.tensor(valid, dtype=torch.int32), -1, 3, cap=1024)
    for b in range(2):
        _compare_raw(refs[b], raw_f, raw_i, counts, b)


def test_detect_compacts_more_than_1024_accepted_records_and_none():
    """The bumps of the detection fixture, 7 samples apart on cleared ground.  Image 0: 1800 candidates of which more
    than 1024 are accepted, the rejected ones (under the threshold after refinement) among them on both sides of the
    1024th record; image 1: candidates of which none is accepted."""
    sift = _sift()
    thr = sr.DETECT_THR
    rows, cols = 36, 50
    h, w = 7 * rows + 2, 7 * cols + 2
    amp = np.random.RandomState(3).choice([0.81, 1.5, -2.0, 3.0], size=(rows, cols), p=[0.3, 0.3, 0.2, 0.2])
    vols = np.zeros((2, 5, h, w), np.float32)
    for r in range(rows):
        for c in range(cols):
            for b, value in ((0, amp[r, c] * thr), (1, 0.81 * thr)):
                if b == 1 and r >= 3:
                    continue
                l, y, x = 1 + (r + c) % 3, 7 * r + 4, 7 * c + 4
                vols[b, l - 1: l + 2, y - 1: y + 2, x - 1: x + 2] = 0.5 * value
                vols[b, l, y, x] = value
    refs = [sr.detect([v], 0, thr) for v in vols]
    assert refs[0]["n_candidates"] == rows * cols and 1024 < len(refs[0]["idx"]) < rows * cols - 200
    assert refs[1]["n_candidates"] == 3 * cols and len(refs[1]["idx"]) == 0
    lay = sift.pyramid_layout(h, w, 0, 1)
    dog = torch.cat([_upload(sift, [v], lay, True) for v in vols])
    raw_f, raw_i, counts = sift.detect(dog, h, w, None, 0, 1, thr, 10.0, cap=2048)
    _compare_raw(refs[0], raw_f, raw_i, counts, 0)
    got = gc.compare_raw(refs[1], raw_f, raw_i, counts, 1)
    assert got["equal"] and got["n"] == 0, got
    assert not raw_i[0, int(counts[0, 0]):].any() and not raw_i[1].any()  # nothing is written beyond the count


# ----------------------------------------------------------------------------------------------- orient and describe
@pytest.fixture(scope="module")
def stage_case():
    levels, rec = sr.stage_fixture()
    ref64, ref32 = [], []
    for r in rec:
        lv = levels[int(r[3])][int(r[4])]
        ref64.append(sr.orientations(lv, r[0], r[1], r[2])[0])
        ref32.append(sr.orientations(lv, r[0], r[1], r[2], np.float32)[0])
    return levels, rec, ref64, ref32


_records = gc.records


def test_orientations_match_the_restatement(stage_case):
    sift = _sift()
    levels, rec, ref64, ref32 = stage_case
    h, w = sr.STAGE_SHAPE
    lay = sift.pyramid_layout(h, w, 0, 2)
    gauss = _upload(sift, levels, lay, False)
    raw_f, raw_i, counts = _records(rec, 64)
    ori_f, ori_i, ocounts = sift.orient(gauss, h, w, raw_f, raw_i, counts, None, 0, 2)
    assert [len(a) for a in ref64] == [len(a) for a in ref32]
    measured = max(abs(x - y) for a, c in zip(ref64, ref32) for x, y in zip(a, c))
    allow = 4 * measured
    want = [(i, th) for i, a in enumerate(ref64) for th in a]
    assert int(ocounts[0, 0]) == len(want) and int(ocounts[0, 1]) == 0
    got_i, got = ori_i[0, : len(want)].cpu().numpy(), ori_f[0, : len(want)].cpu().double().numpy()
    assert [int(x) for x in got_i[:, 0]] == [i for i, _ in want]  # the number of orientations per key point
    diff = np.abs(got[:, 7] - np.array([th for _, th in want]))
    diff = np.minimum(diff, 2 * np.pi - diff)
    print(f"orientation: float32 restatement within {measured:.3e} rad of float64, allowance {allow:.3e}, kernel {diff.max():.3e}")
    assert diff.max() <= allow, (diff.max(), allow)
    assert np.array_equal(got[:, 4:7], np.array([rec[i, :3] for i, _ in want]))  # the record travels unchanged
    assert max(len(a) for a in ref64) >= 2  # the fixture has key points with a secondary peak


def test_orient_compacts_across_1024_records_and_reports_the_overflow(stage_case):
    """The fixture's records and one on a constant level (no gradient, so no orientation), repeated beyond 1024: key
    points with 0, 1 and several orientations on both sides of the 1024th record, and an oriented list 37 rows too
    short: the rows that fit are the first ones, the rest is counted."""
    sift = _sift()
    levels, rec, ref64, ref32 = stage_case
    h, w = sr.STAGE_SHAPE
    lay = sift.pyramid_layout(h, w, 0, 2)
    assert not ((rec[:, 3] == 1) & (rec[:, 4] == 5)).any()  # no record of the fixture reads the level made constant
    flat = [lv.copy() for lv in levels]
    flat[1][5][:] = 0.5
    assert sr.orientations(flat[1][5], 16.0, 16.0, 1.7)[0] == []
    unit = np.concatenate([rec, np.array([[16.0, 16.0, 1.7, 1, 5]], np.float32).astype(np.float64)])
    angles = list(ref64) + [[]]
    n = 1024 + 2 * len(unit)
    which = np.arange(n) % len(unit)
    for part in (which[:1024], which[1024:]):
        assert {min(len(angles[u]), 2) for u in part} == {0, 1, 2}
    want = [(i, j, th) for i, u in enumerate(which) for j, th in enumerate(angles[u])]
    ocap = len(want) - 37
    raw_f, raw_i, counts = _records(unit[which], n)
    ori_f, ori_i, ocounts = sift.orient(_upload(sift, flat, lay, False), h, w, raw_f, raw_i, counts, None, 0, 2, ocap=ocap)
    assert ocounts[0].tolist() == [ocap, 37]
    got_i, got = ori_i[0].cpu().numpy(), ori_f[0].cpu().double().numpy()
    assert np.array_equal(got_i[:, 0], [i for i, _, _ in want[:ocap]])  # the key point of every row ...
    assert np.array_equal(got_i[:, 3], [j for _, j, _ in want[:ocap]])  # ... and which of its orientations
    allow = 4 * max(abs(x - y) for a, c in zip(ref64, ref32) for x, y in zip(a, c))
    diff = np.abs(got[:, 7] - np.array([th for _, _, th in want[:ocap]]))
    diff = np.minimum(diff, 2 * np.pi - diff)
    assert diff.max() <= allow, (diff.max(), allow)
    assert np.array_equal(got[:, 4:7], np.array([unit[which[i], :3] for i, _, _ in want[:ocap]]))


def test_descriptors_match_the_restatement(stage_case):
    sift = _sift()
    levels, rec, ref64, _ = stage_case
    h, w = sr.STAGE_SHAPE
    lay = sift.pyramid_layout(h, w, 0, 2)
    gauss = _upload(sift, levels, lay, False)
    # oriented records: the restatement's angles (fp32-rounded), and angle exactly 0 and exactly pi on two of them
    items = [(i, np.float32(th)) for i, a in enumerate(ref64) for th in a]
    items += [(0, np.float32(0.0)), (1, np.float32(np.pi)), (len(rec) - 4, np.float32(0.0))]
    if len(items) % 4 == 0:
        items.append((2, np.float32(1.0)))
    n = len(items)
    assert n % 4 != 0  # no multiple of the waves of a workgroup
    ocap = 2 * n
    ori_f = torch.zeros(1, ocap, 8)
    ori_i = torch.zeros(1, ocap, 4, dtype=torch.int32)
    for j, (i, th) in enumerate(items):
        ori_f[0, j, 4:7] = torch.from_numpy(rec[i, :3]).float()
        ori_f[0, j, 7] = float(th)
        ori_i[0, j] = torch.tensor([i, int(rec[i, 3]), int(rec[i, 4]), 0])
    ocounts = torch.tensor([[n, 0]], dtype=torch.int32)
    desc = sift.describe(gauss, h, w, ori_f.cuda(), ori_i.cuda(), ocounts.cuda(), None, 0, 2).cpu()
    measured = worst = 0.0
    for j, (i, th) in enumerate(items):
        lv = levels[int(rec[i, 3])][int(rec[i, 4])]
        d64 = sr.descriptor(lv, rec[i, 0], rec[i, 1], rec[i, 2], th)
        d32 = sr.descriptor(lv, rec[i, 0], rec[i, 1], rec[i, 2], th, np.float32)
        measured = max(measured, np.abs(d64 - d32).max())
        worst = max(worst, np.abs(desc[0, j].double().numpy() - d64).max())
        assert abs(np.linalg.norm(d64) - 1) < 1e-9
    allow = 4 * measured
    print(f"descriptor: float32 restatement within {measured:.3e} of float64, allowance {allow:.3e}, kernel {worst:.3e}")
    assert worst <= allow, (worst, allow)  # none excused
    assert not desc[0, n:].any()  # rows beyond the count are not written


# ---------------------------------------------------------------------------------------------------- the four stages
def test_a_constant_region_yields_nothing():
    """The fork's black vignette: the DoG is exactly constant there and an exact tie is no extremum."""
    sift = _sift()
    img = sr.textured_image(120, 160, 3)
    assert (img == 0).mean() > 0.02
    out = sift.extract_raw(torch.from_numpy(img)[None].cuda())
    n = int(out["ocounts"][0, 0])
    xy = out["ori_f"][0, :n, :2].cpu().numpy()
    assert n > 20
    yy, xx = np.clip((xy[:, 1] - 0.5).round().astype(int), 0, 119), np.clip((xy[:, 0] - 0.5).round().astype(int), 0, 159)
    inside = np.zeros(n, bool)
    for dy in range(-4, 5):  # a key point sits on structure: not everything within 4 pixels of it is black
        for dx in range(-4, 5):
            inside |= img[np.clip(yy + dy, 0, 119), np.clip(xx + dx, 0, 159)] != 0
    assert inside.all()
    flat = sift.extract_raw(torch.full((1, 64, 64), 0.37).cuda())
    assert int(flat["counts"][0, 1]) == 0 and int(flat["ocounts"][0, 0]) == 0


def test_the_stages_in_sequence_are_deterministic():
    """Two runs agree bit for bit: no order depends on the arrival of atomics, no sum on the order of the lanes."""
    sift = _sift()
    img, fo, no = sr.e2e_fixture()
    dev = torch.from_numpy(img)[None].cuda()
    a = sift.extract_raw(dev, None, fo, no)
    b = sift.extract_raw(dev, None, fo, no)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["ocounts"][0, 0]) > 50 and int(a["ocounts"][0, 1]) == 0 and int(a["counts"][0, 2]) == 0


def test_the_module_follows_the_restatement_along_its_own_chain():
    """The `SIFT` module on the end-to-end fixture (sift_reference.e2e_fixture: 120 x 160 inside a black vignette), held
    to the STAGE tolerances: the pyramid per element within its float64 bound; every later stage of the restatement fed
    what the device produced before it (sift_gpu_cases.whole_extractor_figures), so that detection is exact with x, y,
    sigma, score within 1e-6 relative of the fp32-rounded restatement, orientation within 4 x the float32 / float64
    distance measured on this fixture, descriptors within theirs; the module's output bit-equal to the restated
    post-processing of that list, RootSIFT within 1e-6.  None excused for pyramid rounding; only a key point whose peak
    margin is below 1e-4 may have another number of orientations, at most 1 % of them."""
    fig = gc.whole_extractor_figures(_sift())
    print("whole:", {k: v for k, v in fig.items()})
    assert fig["octaves_agree"]
    assert fig["pyramid_worst_gauss_error_over_bound"] <= 1 and fig["pyramid_worst_dog_error_over_bound"] <= 1
    det = fig["detection"]
    assert det["equal"] and det["n"] == fig["key_points_restatement"] >= 50  # 0 excused
    assert det["rel"] <= 1e-6
    od = fig["orientation_and_descriptor"]
    assert od["orientation_overflow"] == 0
    assert od["of_those_without_a_peak_margin_below_1e-4"] == 0
    assert od["key_points_with_another_number_of_orientations"] <= 0.01 * od["key_points"]
    assert od["orientation_kernel_vs_float64_rad"] <= od["orientation_allowance_rad"]
    assert od["descriptor_kernel_vs_float64"] <= od["descriptor_allowance"]  # none excused
    assert fig["after_filter_dog_point"] > fig["module_kept"] == fig["restated_kept"] == 48  # the top-k cuts
    assert fig["module_equals_restated_post_processing"]
    assert fig["module_rootsift_vs_restated"] <= 1e-6


def test_the_input_is_clipped_to_0_1_like_the_reference():
    """np.clip(image, 0, 1) of extract_single_image: values outside give the pyramid of the clipped image, bit for bit."""
    sift = _sift()
    img = gc.image(40, 56, 9) * 3.0 - 1.0
    assert (img < 0).mean() > 0.02 and (img > 1).mean() > 0.02
    for fo in (-1, 0):
        a = sift.pyramid(torch.from_numpy(img)[None].cuda(), None, fo, 2)
        b = sift.pyramid(torch.from_numpy(np.clip(img, 0, 1))[None].cuda(), None, fo, 2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    wg, wd, _ = gc.pyramid_errors(sift, img[None], [None], -1, 2)
    assert wg <= 1 and wd <= 1


# ------------------------------------------------------------------------------------------------------------ filter
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_post.npz")


@pytest.fixture(scope="module")
def post():
    z = np.load(GOLDEN)
    n, ocap = len(z["points"]), 64
    ori_f = torch.zeros(1, ocap, 8)
    ori_f[0, :n, :2] = torch.from_numpy(z["points"])
    ori_f[0, :n, 2] = torch.from_numpy(z["scales"])
    ori_f[0, :n, 3] = torch.from_numpy(z["scores"])
    ori_f[0, :n, 7] = torch.from_numpy(z["angles"])
    desc = torch.zeros(1, ocap, 128)
    desc[0, :n] = torch.from_numpy(z["desc"])
    return z, ori_f.cuda(), desc.cuda(), torch.tensor([[n, 0]], dtype=torch.int32).cuda()


def _kept(out):
    n = int(out["counts"][0])
    assert (out["index"][0, n:] == -1).all()
    return out["index"][0, :n].cpu().long()


def test_filter_equals_the_reference_vectors(post):
    """gfc_sift_filter on the planted inputs of tests/golden/sift_post.npz: the kept index sets and the top-k sets are
    the reference's own (filter_dog_point, the specular rule, torch.topk), RootSIFT within 1e-6."""
    sift = _sift()
    z, ori_f, desc, ocounts = post
    h, w = (int(v) for v in z["shape"])
    k = int(z["k"])
    for r in (0, 3):
        out = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=r, rootsift=False)
        assert torch.equal(_kept(out).sort().values, torch.from_numpy(z[f"keep_r{r}"]))
        assert torch.equal(_kept(out), _kept(out).sort().values)  # nothing cut: the list order
    out = sift.filter_list(ori_f, desc, ocounts, h, w, specular=torch.from_numpy(z["mask"])[None], nms_radius=None,
                           rootsift=False)
    assert torch.equal(_kept(out), torch.from_numpy(z["specular_keep"]))
    none = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=None, rootsift=False)
    assert torch.equal(_kept(none), torch.arange(len(z["points"])))
    assert torch.equal(none["descriptors"][0, :40].cpu(), torch.from_numpy(z["desc"]))
    out = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=0, k=k, rootsift=False)
    assert torch.equal(_kept(out).sort().values, torch.from_numpy(z["topk_score"]))
    assert torch.equal(_kept(out), torch.from_numpy(z["topk_score_order"]))  # torch.topk's descending order
    sel = _kept(out)
    assert torch.equal(out["keypoints"][0].cpu(), torch.from_numpy(z["points"])[sel])
    assert torch.equal(out["oris"][0].cpu(), torch.from_numpy(z["angles"])[sel])
    out = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=0, scale_weighting=True, k=k, rootsift=False)
    assert torch.equal(_kept(out).sort().values, torch.from_numpy(z["topk_score_scale"]))
    # RootSIFT of every row, and the padded rows of force_num_keypoints (zeros before, the constant after)
    out = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=None, rootsift=True)
    assert (out["descriptors"][0, :40].cpu() - torch.from_numpy(z["rootsift"])).abs().max() <= 1e-6
    pad = int(z["pad"])
    out = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=0, k=k, rootsift=True, out_cap=pad)
    assert int(out["counts"][0]) == k
    assert (out["descriptors"][0].cpu() - torch.from_numpy(z["padded_rootsift"])).abs().max() <= 1e-6
    assert torch.equal(out["scales"][0].cpu(), torch.from_numpy(z["padded_scales"]))
    assert torch.equal(out["oris"][0].cpu(), torch.from_numpy(z["padded_oris"]))
    assert torch.equal(out["keypoint_scores"][0].cpu(), torch.from_numpy(z["padded_scores"]))
    raw = sift.filter_list(ori_f, desc, ocounts, h, w, nms_radius=0, k=k, rootsift=False, out_cap=pad)
    assert torch.equal(raw["descriptors"][0].cpu(), torch.from_numpy(z["padded_desc"]))


def test_extract_in_one_call_equals_the_composition_of_the_stage_calls_bit_for_bit():
    """gfc_sift_extract against pyramid -> detect -> orient -> describe -> filter with the same cap and ocap, on a batch of
    two with differing valid sizes, a specular mask, nms_radius 2 and a top-k that cuts."""
    sift = _sift()
    h, w, cap, ocap, k = 120, 160, 1024, 2048, 40
    img = torch.from_numpy(np.stack([sr.textured_image(h, w, 60 + i, n=60) for i in range(2)])).cuda()
    valid = torch.tensor([[160, 120], [141, 99]], dtype=torch.int32)
    mask = torch.ones(2, h, w, dtype=torch.bool)
    mask[:, 20:50, 30:90] = False
    for fo, no in ((-1, 4), (0, 3)):
        gauss, dog, _ = sift.pyramid(img, valid, fo, no)
        raw_f, raw_i, counts = sift.detect(dog, h, w, valid, fo, no, cap=cap)
        ori_f, ori_i, ocounts = sift.orient(gauss, h, w, raw_f, raw_i, counts, valid, fo, no, ocap=ocap)
        desc = sift.describe(gauss, h, w, ori_f, ori_i, ocounts, valid, fo, no)
        want = sift.filter_list(ori_f, desc, ocounts, h, w, valid, mask, 2, False, k, True, out_cap=64)
        got = sift.extract(img, valid, mask, fo, no, cap=cap, ocap=ocap, nms_radius=2, k=k, rootsift=True, out_cap=64)
        assert got["counts"].tolist() == want["counts"].tolist() and int(want["counts"][0]) == k  # the top-k cuts
        for key in want:
            assert torch.equal(got[key], want[key]), (fo, key)
        assert torch.equal(got["stage_counts"], counts) and torch.equal(got["ocounts"], ocounts)
    from glue_factory_colon_amd import _native as nat

    need = nat.lib().gfc_sift_extract_workspace_bytes(2, h, w, -1, 4, cap, ocap)
    assert need > nat.lib().gfc_sift_filter_workspace_bytes(2, h, w, ocap) + 4 * 2 * ocap * 128
    with pytest.raises(nat.NativeError, match="GFC_ERR_UNSUPPORTED"):
        sift.extract(torch.zeros(1, 12, 40).cuda(), first_octave=0)  # a 12-pixel side: no octave


# ------------------------------------------------------------------------------------------------------------ module
def _batch(n, h=120, w=160, seed=70):
    return torch.from_numpy(np.stack([sr.textured_image(h, w, seed + i, n=60) for i in range(n)]))[:, None]


def test_module_keys_shapes_dtypes_and_padding():
    sift = _sift()
    k = 48
    model = sift.SIFT({"max_num_keypoints": k, "force_num_keypoints": True, "mask_out_padded_kpts": True}).eval()
    img = _batch(2)
    img[1, :, :, 60:] = 0.0  # few key points in the second image: it is padded
    pred = model({"image": img.cuda()})
    want = {"keypoints": ((2, k, 2), torch.float32), "scales": ((2, k), torch.float32), "oris": ((2, k), torch.float32),
            "descriptors": ((2, k, 128), torch.float32), "keypoint_scores": ((2, k), torch.float32),
            "num_keypoints_detected": ((2,), torch.int64), "num_keypoints_padded": ((2,), torch.int64),
            "extractor_core_time_ms": ((2,), torch.float32), "valid_depth_keypoints": ((2, k), torch.bool)}
    assert set(pred) == set(want)
    for key, (shape, dtype) in want.items():
        assert tuple(pred[key].shape) == shape and pred[key].dtype == dtype, key
    det, padded = pred["num_keypoints_detected"].tolist(), pred["num_keypoints_padded"].tolist()
    assert det[0] == k and padded[0] == 0 and 0 < det[1] < k and padded[1] == k - det[1]
    n = det[1]
    assert pred["valid_depth_keypoints"][1].tolist() == [True] * n + [False] * (k - n)
    assert not pred["scales"][1, n:].any() and not pred["oris"][1, n:].any() and not pred["keypoint_scores"][1, n:].any()
    assert (pred["descriptors"][1, n:] - (1 / 128) ** 0.5).abs().max() < 1e-6  # RootSIFT of the zero padding
    kp = pred["keypoints"][1]
    assert (kp[n:] >= kp[:n].min(0).values).all() and (kp[n:] <= kp[:n].max(0).values).all()  # random_c
    assert (pred["keypoint_scores"][0, :-1] >= pred["keypoint_scores"][0, 1:]).all()  # top-k order
    assert (pred["descriptors"][0].norm(dim=-1) - 1).abs().max() < 1e-5
    assert float(pred["extractor_core_time_ms"][0]) > 0
    with pytest.raises(Exception, match="cuda"):
        model({"image": img})  # no CPU path


def test_module_crops_each_item_to_its_image_size():
    """An item of a batch of three with differing image_size equals its own single call bit for bit."""
    sift = _sift()
    k = 128
    model = sift.SIFT({"max_num_keypoints": k, "force_num_keypoints": True}).eval()
    img = _batch(3, seed=80).cuda()
    sizes = torch.tensor([[160.0, 120.0], [131.0, 97.0], [90.0, 120.0]]).cuda()
    pred = model({"image": img, "image_size": sizes})
    for i in range(3):
        one = model({"image": img[i: i + 1], "image_size": sizes[i: i + 1]})
        n = int(one["num_keypoints_detected"][0])
        assert n == int(pred["num_keypoints_detected"][i]) and n > 10
        for key in ("keypoints", "scales", "oris", "descriptors", "keypoint_scores"):
            assert torch.equal(one[key][0, :n], pred[key][i, :n]), (i, key)
        w, h = sizes[i].tolist()
        assert (pred["keypoints"][i, :n, 0] < w).all() and (pred["keypoints"][i, :n, 1] < h).all()
        cropped = model({"image": img[i: i + 1, :, : int(h), : int(w)].contiguous()})  # the reference crops the tensor
        for key in ("keypoints", "scales", "oris", "descriptors", "keypoint_scores"):
            assert torch.equal(cropped[key][0, :n], pred[key][i, :n]), (i, key, "cropped")


def test_module_rgb_input_channel_selection_and_specular_mask():
    sift = _sift()
    rgb = torch.cat([_batch(1, seed=90), _batch(1, seed=91), _batch(1, seed=92)], 1).cuda()  # [1,3,H,W]
    for channel, idx in (("red", 0), ("green", 1), ("blue", 2)):
        a = sift.SIFT({"extractor_channel": channel})({"image": rgb})
        b = sift.SIFT({})({"image": rgb[:, idx: idx + 1].contiguous()})
        assert a["keypoints"].shape[1] > 10
        for key in ("keypoints", "scales", "oris", "descriptors", "keypoint_scores"):
            assert torch.equal(a[key], b[key]), (channel, key)
    grey = rgb[:, 0] * 0.299
    grey = grey + rgb[:, 1] * 0.587
    grey = grey + rgb[:, 2] * 0.114
    a = sift.SIFT({})({"image": rgb})
    b = sift.SIFT({})({"image": grey[:, None].contiguous()})
    for key in ("keypoints", "scales", "oris", "descriptors", "keypoint_scores"):
        assert torch.equal(a[key], b[key]), key
    mask = torch.ones(1, 1, 120, 160, dtype=torch.bool)
    mask[..., 30:90, 40:120] = False
    masked = sift.SIFT({})({"image": rgb, "specular_mask": mask.cuda()})
    keep = sr.specular_keep(a["keypoints"][0].cpu().numpy(), mask.numpy())
    assert 0 < keep.sum() < len(keep)
    assert torch.equal(masked["keypoints"][0], a["keypoints"][0][torch.from_numpy(keep).cuda()])
    ignored = sift.SIFT({"filter_specular_keypoints": False})({"image": rgb, "specular_mask": mask.cuda()})
    assert torch.equal(ignored["keypoints"], a["keypoints"])


def test_module_refuses_to_stack_differing_counts():
    sift = _sift()
    img = _batch(2, seed=95).cuda()
    model = sift.SIFT({"max_num_keypoints": 4096})
    n = [int(model({"image": img[i: i + 1]})["num_keypoints_detected"][0]) for i in range(2)]
    assert n[0] != n[1]
    with pytest.raises(RuntimeError, match="equal size"):
        model({"image": img})
    both = sift.SIFT({"max_num_keypoints": min(n) - 3})({"image": img})  # the top-k equalises them
    assert both["keypoints"].shape == (2, min(n) - 3, 2)
    with pytest.raises(RuntimeError, match="candidate_cap"):
        sift.SIFT({"candidate_cap": 8})({"image": img})  # never a silent drop


def test_two_view_pipeline_with_sift_and_lightglue_scale_ori():
    from glue_factory_colon_amd import weights
    from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline

    pipe = TwoViewPipeline({
        "extractor": {"name": "extractors.sift", "max_num_keypoints": 256},
        "matcher": {"name": "matchers.lightglue", "weights": None, "add_scale_ori": True, "input_dim": 128,
                    "filter_threshold": 0.1},
    }).eval()
    pipe.matcher.load_state_dict(weights.lightglue_state_dict(0, input_dim=128, add_scale_ori=True), strict=False)
    pipe = pipe.cuda()
    datas = []
    for i, (h, w) in enumerate(((120, 160), (96, 144))):
        a = torch.from_numpy(sr.textured_image(h, w, 100 + i, n=80))[None, None].cuda()
        b = torch.roll(a, (3, 5), (2, 3))
        datas.append({"view0": {"image": a}, "view1": {"image": b}})
    with torch.no_grad():
        single = [pipe(d) for d in datas]
        batched = pipe.forward_pairs(datas)
    for s, p in zip(single, batched):
        for key in ("keypoints0", "keypoints1", "scales0", "oris1", "descriptors0", "matches0"):
            assert key in s and torch.equal(s[key], p[key]), key
        assert s["descriptors0"].shape[-1] == 128 and s["keypoints0"].shape[1] == s["scales0"].shape[1] > 20
        assert (s["matching_scores0"] - p["matching_scores0"]).abs().max() < 1e-4
        assert int((s["matches0"] >= 0).sum()) > 0
