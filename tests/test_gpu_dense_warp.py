"""csrc/gt_dense_warp.hip (gfc_dense_cycle_error, gfc_gt_sample_dense_warp, gfc_gt_matches_roma), dense_warp.py and
RomaGTMatcher against the reference's vectors (tests/golden/dense_warp.npz, made by the reference's own cycle_dist and
gt_matches_from_roma) and, at sizes no fixture holds, against the float64 restatement tests/dense_warp_reference.py.

Fixture cases: the restatement flags nothing undecided there, so every integer, mask, assignment and reward must be EQUAL
to the reference's float32 results; the floats (proj, certainty_kp, cycle_error_kp, scores, the cycle fields) must lie
within the restatement's PER-ELEMENT bounds of the reference's float64 values.  The worst fraction of a bound that is
used goes to profiles/dense_warp_parity.json.
Generated cases: the restatement marks which verdicts are undecided; asserted on the CPU side first that at most 1 % of
the key points and 2 x 1 % + 1e-4 of the dense elements are (the caps of tests/test_gpu_sparse_map.py); every other value
must be equal, every float inside its bound.
Sizes: 16 key points per workgroup, 16 lanes per key point and tiles of 256 elements, so the label shapes sit one below,
at and one above 16 and 256 and above 16 x 256; the finishing launch has 256 threads over the M + N key points of a pair:
M + N = 255, 256, 257 and 511, 512, 513 are among the shapes.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_warp_reference as dr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("matches0", "matches1") + tuple(k + q for k in dr.MASK_KEYS for q in "01")
FLOATS = (("proj_0to1", "proj_bound0", "0"), ("proj_1to0", "proj_bound1", "1"), ("certainty_kp0", "cert_bound0", "0"),
          ("certainty_kp1", "cert_bound1", "1"), ("cycle_error_kp0", "cyc_bound0", "0"),
          ("cycle_error_kp1", "cyc_bound1", "1"))
KEYS20 = {"assignment", "reward", "matches0", "matches1", "matching_scores0", "matching_scores1", "proj_0to1", "proj_1to0",
          "certainty_kp0", "certainty_kp1", "cycle_error_kp0", "cycle_error_kp1"} | {k + q for k in dr.MASK_KEYS for q in "01"}
KP_CAP, DENSE_CAP = 0.01, 2 * 0.01 + 1e-4
BIG_IMG = {"img0": (480, 640), "img1": (448, 608)}


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "dense_warp.npz"))


def data_of(case):
    return {"view0": {"image": torch.zeros((case["kp0"].shape[0], 1) + tuple(case["img0_hw"]), device="cuda")},
            "view1": {"image": torch.zeros((case["kp0"].shape[0], 1) + tuple(case["img1_hw"]), device="cuda")}}


def run_gpu(case, setting, mode="taps", dense=True):
    """gt_matches_from_roma on the GPU -> CPU tensors.  mode: how the cycle error is made when the setting has one --
    'taps' (add_cycle_error, at the four taps) or 'field' (both dense fields first, then sampled)."""
    from glue_factory_colon_amd import dense_warp

    pos, neg, pc, pcy, nc, ncy, with_cycle = setting
    c = {k: v.cuda() for k, v in case.items() if isinstance(v, torch.Tensor)}
    kw = {}
    if with_cycle and mode == "field":
        kw = {"cycle_error0": dense_warp.cycle_dist(c["warp0"], c["warp1"]),
              "cycle_error1": dense_warp.cycle_dist(c["warp1"], c["warp0"])}
    elif with_cycle:
        kw = {"add_cycle_error": True}
    out = dense_warp.gt_matches_from_roma(
        c["kp0"], c["kp1"], data_of(case), valid0=c["scores0"] > 0, valid1=c["scores1"] > 0, warp0=c["warp0"],
        warp1=c["warp1"], certainty0=c["certainty0"], certainty1=c["certainty1"], pos_th=pos, neg_th=neg, pos_cert_th=pc,
        pos_cycle_error_th=pcy, neg_cert_th=nc, neg_cycle_error_th=ncy, dense=dense, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def fraction(got, ref, bound, skip=None):
    """The worst |got - ref| / bound where ref is finite (and not skipped); NaN patterns must agree there."""
    got, ref = got.double(), ref.double()
    if bound.ndim < ref.ndim:
        bound = bound[..., None].expand_as(ref)
    keep = torch.ones_like(ref, dtype=torch.bool) if skip is None else ~(skip[..., None].expand_as(ref) if skip.ndim < ref.ndim else skip)
    assert torch.equal(torch.isfinite(got)[keep], torch.isfinite(ref)[keep]), "finite patterns differ"
    fin = torch.isfinite(ref) & keep
    if not bool(fin.any()):
        return 0.0
    return float(((got - ref).abs() / bound.clamp(min=1e-300))[fin].max())


def check_against_restatement(name, case, setting, mode="taps", dense=True):
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    refs = []
    for i in range(b):  # before the kernel's answer is looked at
        r = dr.run(case, setting, i)
        share = (int(r["undecided0"].sum()) + int(r["undecided1"].sum())) / (m + n)
        dense_share = float(r["undecided_dense"].float().mean())
        assert share <= KP_CAP and dense_share <= DENSE_CAP, ("bad input: too many undecided", name, share, dense_share)
        refs.append(r)
    out = run_gpu(case, setting, mode, dense)
    worst = 0.0
    for i, r in enumerate(refs):
        und = {"0": r["undecided0"], "1": r["undecided1"]}
        for k, bk, q in FLOATS:
            f = fraction(out[k][i], r[k], r[bk], skip=r["shaky" + q])
            worst = max(worst, f)
            assert f <= 1.0, (name, i, k, f)
        for q in "01":
            differ = out["matches" + q][i] != r["matches" + q]
            print(name, i, "matches" + q, "undecided", int(und[q].sum()), "differ", int(differ.sum()))
            assert not bool((differ & ~und[q]).any()), (name, i, q, torch.nonzero(differ & ~und[q]).flatten()[:10])
            for key in dr.MASK_KEYS:
                bad = (out[key + q][i] != r[key + q]) & ~und[q]
                assert not bool(bad.any()), (name, i, key + q, torch.nonzero(bad).flatten()[:10])
            f = fraction(out["matching_scores" + q][i], r["matching_scores" + q], r["cert_bound" + q], skip=und[q])
            assert f <= 1.0, (name, i, "matching_scores" + q, f)
        if dense:
            sure = ~r["undecided_dense"]
            assert torch.equal(out["assignment"][i][sure], r["assignment"][sure]), (name, i)
            assert torch.equal(out["reward"][i][sure].double(), r["reward"][sure]), (name, i)
    print(name, "worst fraction of a bound", worst)
    return out, refs


# ---- the reference's vectors --------------------------------------------------------------------------------------------
def equal_to_fixture(z, tag, ftag, out, r, report):
    m, n = out["matches0"].shape[1], out["matches1"].shape[1]
    for k in INT_KEYS:
        differ = int((out[k][0] != torch.from_numpy(z[tag + k])).sum())
        assert differ == 0, (tag, k, differ)
    want = np.unpackbits(z[tag + "assignment"])[:m * n].reshape(m, n).astype(bool)
    assert np.array_equal(out["assignment"][0].numpy(), want), tag
    assert np.array_equal(out["reward"][0].numpy(), z[tag + "reward"].astype(np.float32)), tag
    for k, bk, q in FLOATS:
        f = fraction(out[k][0], torch.from_numpy(z[ftag + k + "_f64"]), r[bk])
        report[tag + k] = f
        assert f <= 1.0, (tag, k, f)
    for q in "01":
        f = fraction(out["matching_scores" + q][0], torch.from_numpy(z[tag + "matching_scores" + q + "_f64"]), r["cert_bound" + q])
        report[tag + "matching_scores" + q] = f
        assert f <= 1.0, (tag, q, f)


def test_fixture_cases_equal_the_reference(z):
    from glue_factory_colon_amd import dense_warp

    report = {}
    for c in range(3):
        case = dr.fixture_case(z, c)
        for s, setting in enumerate(dr.SETTINGS):
            assert tuple(z["settings"][s]) == tuple(-1.0 if v is None else float(v) for v in setting)
            r = dr.run(case, setting)
            ftag = f"c{c}_s{0 if setting[6] else 1}_"
            for mode in ("taps", "field") if setting[6] else ("taps",):
                out = run_gpu(case, setting, mode)
                assert set(out) == KEYS20 and out["assignment"].dtype == torch.bool and out["mask_pos0"].dtype == torch.bool
                assert out["matches0"].dtype == torch.long and out["reward"].dtype == torch.float32
                equal_to_fixture(z, f"c{c}_s{s}_", ftag, out, r, report)
    case = dr.fixture_case(z, 0)
    w0, w1 = case["warp0"].cuda(), case["warp1"].cuda()
    for key, (q, rr) in (("cycle_error0", (w0, w1)), ("cycle_error1", (w1, w0))):
        got = dense_warp.cycle_dist(q, rr)[0].cpu()
        bound = dr.cycle_dist(q[0].cpu().double(), rr[0].cpu().double())[1]
        report["c0_" + key] = fraction(got, torch.from_numpy(z["c0_" + key + "_f64"]), bound)
        assert report["c0_" + key] <= 1.0, key
    worst = max(report.values())
    print("worst fraction of a bound over the fixture", worst)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dense_warp_parity.json"), "w") as f:
        json.dump({"what": "worst |GPU float32 - reference float64| / per-element bound of tests/dense_warp_reference.py "
                           "over tests/golden/dense_warp.npz; integers, masks, assignment and reward are equal",
                   "worst_fraction_of_bound": worst, "per_output": report}, f, indent=1, sort_keys=True)


# ---- cycle error alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,hw,hwr", [(3, (37, 53), (41, 29)), (1, (1, 1), (1, 1)), (2, (560, 560), (560, 560))])
def test_cycle_error_alone(b, hw, hwr):
    from glue_factory_colon_amd import dense_warp

    case = dr.make_case(5, b, 1, 1, field0=hw, field1=hwr, plant=min(hw) > 12)
    got = dense_warp.cycle_dist(case["warp0"].cuda(), case["warp1"].cuda()).cpu()
    assert got.shape == (b,) + hw and got.dtype == torch.float32
    worst = 0.0
    for i in range(b):
        e, bound, shaky = dr.cycle_dist(case["warp0"][i].double(), case["warp1"][i].double())
        worst = max(worst, fraction(got[i], e, bound, skip=shaky))
    print("cycle error", b, hw, hwr, "worst fraction of the bound", worst, "largest bound", float(bound.max()))
    assert worst <= 1.0
    if min(hw) > 12:
        assert bool(torch.isnan(got).any()) and float(got.nan_to_num().max()) > 20.0


@pytest.mark.parametrize("m", [1, 255, 2048])
def test_cycle_error_at_the_taps_is_bit_equal_to_the_dense_field_sampled(m):
    from glue_factory_colon_amd import dense_warp

    case = dr.make_case(6, 2, m, m, field0=(61, 83), field1=(47, 71))
    c = {k: v.cuda() for k, v in case.items() if isinstance(v, torch.Tensor)}
    for kp, w, cert, o, q_hw, t_hw in ((c["kp0"], c["warp0"], c["certainty0"], c["warp1"], dr.IMG0, dr.IMG1),
                                        (c["kp1"], c["warp1"], c["certainty1"], c["warp0"], dr.IMG1, dr.IMG0)):
        field = dense_warp.cycle_dist(w, o)
        a = dense_warp.sample_dense_warp(kp, w, cert, q_hw, t_hw, cycle_error=field)
        t = dense_warp.sample_dense_warp(kp, w, cert, q_hw, t_hw, other_warp=o)
        zero = dense_warp.sample_dense_warp(kp, w, cert, q_hw, t_hw)
        torch.cuda.synchronize()
        for x, y in zip(a, t):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))  # bit for bit, NaN included
        assert torch.equal(zero[0].view(torch.int32), a[0].view(torch.int32)) and not bool(zero[2].any())
        assert bool((a[2] > 0).any())


# ---- the labels against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 1), (15, 17), (16, 16), (17, 15), (127, 128), (128, 128), (127, 130), (255, 256),
                                 (255, 257), (256, 256), (257, 255), (256, 257), (300, 4097)])
def test_block_and_tile_edges(m, n):
    case = dr.make_case(3, 1, m, n, **BIG_IMG)
    check_against_restatement(f"{m}x{n}", case, dr.SETTINGS[0])
    check_against_restatement(f"{m}x{n}_none", case, dr.SETTINGS[1], dense=m * n < 70000)


@pytest.fixture(scope="module")
def large():
    return dr.large_cases()


@pytest.mark.parametrize("name", ["2x2048x2048", "4000x3900"])
def test_large_cases(large, name):
    case, setting = large[name]
    out, refs = check_against_restatement(name, case, setting, dense=False)
    assert (out["matches0"] > -1).any() and (out["matches0"] == -1).any() and (out["matches0"] == -2).any()
    assert out["mask_neg_unreliable0"].any() and out["mask_neg_unreliable1"].any()


def test_2x2048x2048_dense_and_the_field_path(large):
    case, setting = large["2x2048x2048"]
    out, _ = check_against_restatement("2x2048x2048_field", case, setting, mode="field", dense=True)
    rows = out["assignment"].any(2)
    assert torch.equal(rows, out["matches0"] > -1)  # a positive is never overridden, and nothing else is matched


@pytest.mark.parametrize("m,n", [(300, 257), (257, 600), (2048, 2048)])
def test_exact_ties_resolve_to_the_first_index(m, n):
    """tie_case: key points k, k + 100, k + 200, ... of a side are bit-identical, in other lanes and other tiles."""
    case = dr.tie_case(m, n)
    setting = (3.0, 5.0, None, None, None, None, False)
    out = run_gpu(case, setting)
    r = dr.run(case, setting)
    k = min(m, n, 100)
    want0 = torch.full((m,), -2, dtype=torch.long)
    want0[:k] = torch.arange(k)
    want1 = torch.full((n,), -2, dtype=torch.long)
    want1[:k] = torch.arange(k)
    assert torch.equal(r["matches0"], want0) and torch.equal(r["matches1"], want1)  # the restatement says so too
    assert torch.equal(out["matches0"][0], want0) and torch.equal(out["matches1"][0], want1)
    assert torch.equal(out["assignment"][0], r["assignment"]) and int(out["assignment"].sum()) == k
    if m >= 200:  # the twins project to the same bits: their distances are equal floats
        assert torch.equal(out["proj_0to1"][0, :100], out["proj_0to1"][0, 100:200])


def test_an_all_invalid_side_and_an_empty_side():
    from glue_factory_colon_amd import dense_warp

    case = dr.make_case(7, 2, 130, 67, **BIG_IMG)
    case["scores0"] = torch.zeros_like(case["scores0"])
    out, refs = check_against_restatement("all_invalid", case, dr.SETTINGS[0])
    assert (out["matches0"] == -2).all() and not out["mask_pos0"].any() and not out["mask_ign0"].any()
    assert not out["assignment"].any() and (out["reward"] == 0).all()
    assert torch.equal(out["matches1"] == -1, out["mask_neg_far1"] | out["mask_neg_unreliable1"])
    assert out["mask_neg_far1"].any() and torch.equal(out["mask_neg_far1"], out["mask_pos1"])  # a row of +inf is far
    # an empty side: the dict of gt_generation.py:62-94
    c = {k: v.cuda() for k, v in case.items() if isinstance(v, torch.Tensor)}
    for m, n in ((0, 67), (130, 0), (0, 0)):
        e = dense_warp.gt_matches_from_roma(c["kp0"][:, :m], c["kp1"][:, :n], data_of(case))
        torch.cuda.synchronize()
        assert set(e) == KEYS20 and e["assignment"].shape == (2, m, n) and e["reward"].dtype == torch.float32
        assert (e["matches0"] == -1).all() and (e["matches1"] == -1).all()
        assert not e["matching_scores0"].any() and not e["matching_scores1"].any()
        for k in dr.MASK_KEYS:
            assert e[k + "0"].dtype == torch.bool and not e[k + "0"].any() and not e[k + "1"].any()
        assert torch.equal(e["certainty_kp1"], c["kp1"][:, :n, 0]) and torch.equal(e["cycle_error_kp0"], c["kp0"][:, :m, 0])
        assert nat.call("gfc_gt_matches_roma_workspace_bytes", 2, m, n) == 0


def test_a_workspace_one_byte_short_is_refused_with_the_outputs_untouched():
    b, m, n = 2, 130, 67
    g = torch.Generator().manual_seed(1)
    f = lambda *s: torch.rand(s, generator=g).cuda()  # noqa: E731
    kp0, kp1, p01, p10 = f(b, m, 2) * 100, f(b, n, 2) * 100, f(b, m, 2) * 100, f(b, n, 2) * 100
    c0, c1, e0, e1 = f(b, m), f(b, n), f(b, m), f(b, n)
    v0, v1 = torch.ones((b, m), dtype=torch.bool, device="cuda"), torch.ones((b, n), dtype=torch.bool, device="cuda")
    outs = [torch.full((b, m), 7, dtype=torch.long, device="cuda"), torch.full((b, n), 7, dtype=torch.long, device="cuda"),
            torch.full((b, m), 7.0, device="cuda"), torch.full((b, n), 7.0, device="cuda"),
            torch.full((b, 4, m), 7, dtype=torch.uint8, device="cuda"), torch.full((b, 4, n), 7, dtype=torch.uint8, device="cuda"),
            torch.full((b, m, n), 7, dtype=torch.uint8, device="cuda"), torch.full((b, m, n), 7.0, device="cuda")]
    nbytes = nat.call("gfc_gt_matches_roma_workspace_bytes", b, m, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    args = lambda size, pos=3.0: (kp0, kp1, p01, p10, c0, c1, e0, e1, v0, v1, b, m, n, pos, 5.0, 0.05, 2.0, 5e-4, 20.0,  # noqa: E731
                                  *outs, ws, size)
    with pytest.raises(nat.NativeError, match="WORKSPACE"):
        nat.call("gfc_gt_matches_roma", *args(nbytes - 1), device=kp0.device)
    with pytest.raises(nat.NativeError, match="INVALID"):  # pos_th is required
        nat.call("gfc_gt_matches_roma", *args(nbytes, pos=-1.0), device=kp0.device)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7).all())
    nat.call("gfc_gt_matches_roma", *args(nbytes), device=kp0.device)
    torch.cuda.synchronize()
    assert not bool((outs[0] == 7).any()) and not bool((outs[7] == 7).any()) and int(outs[4].max()) <= 1


# ---- the matcher ---------------------------------------------------------------------------------------------------------
CONF = {"th_positive": 3.0, "th_negative": 5.0,
        "roma": {"add_cycle_error": True, "pos_cert_th": 0.05, "pos_cycle_error_th": 2.0, "neg_cert_th": 5e-4,
                 "neg_cycle_error_th": 20.0}}


def matcher_data(case, half=False):
    c = {k: v.cuda() for k, v in case.items() if isinstance(v, torch.Tensor)}
    h = (lambda v: v.half()) if half else (lambda v: v)
    return {**data_of(case), "keypoints0": c["kp0"], "keypoints1": c["kp1"], "keypoint_scores0": c["scores0"],
            "keypoint_scores1": c["scores1"], "warp0": h(c["warp0"]), "warp1": h(c["warp1"]),
            "certainty0": h(c["certainty0"]), "certainty1": h(c["certainty1"])}


def test_matcher_against_the_twenty_keys_of_the_fixture(z):
    from glue_factory_colon_amd import dense_warp
    from glue_factory_colon_amd.registry import get_model

    case = dr.fixture_case(z, 0)
    r = dr.run(case, dr.SETTINGS[0])
    data = matcher_data(case)
    out = get_model("matchers.roma_gt_matcher")(CONF).eval()(data)
    torch.cuda.synchronize()
    assert set(out) == KEYS20
    equal_to_fixture(z, "c0_s0_", "c0_s0_", {k: v.cpu() for k, v in out.items()}, r, {})
    # cycle fields in the data win over add_cycle_error; they give the same bits
    fields = {"cycle_error0": dense_warp.cycle_dist(data["warp0"], data["warp1"]),
              "cycle_error1": dense_warp.cycle_dist(data["warp1"], data["warp0"])}
    both = get_model("roma_gt_matcher")(CONF).eval()({**data, **fields})
    lean = get_model("roma_gt_matcher")({**CONF, "dense_outputs": False}).eval()(data)
    torch.cuda.synchronize()
    assert set(lean) == KEYS20 - {"assignment", "reward"}
    for other in (both, lean):
        for k in other:
            assert torch.equal(other[k].nan_to_num(nan=-7.0), out[k].nan_to_num(nan=-7.0)) if other[k].is_floating_point() \
                else torch.equal(other[k], out[k]), k
    # without add_cycle_error and without fields the cycle thresholds are refused as in the reference
    plain = {**CONF, "roma": {**CONF["roma"], "add_cycle_error": False}}
    with pytest.raises(ValueError, match="requires cycle_error0/1 when cycle thresholds"):
        get_model("roma_gt_matcher")(plain).eval()(data)
    # settings 1: nothing optional, no cycle error
    none = get_model("roma_gt_matcher")({"th_positive": 3.0, "th_negative": 5.0}).eval()(data)
    equal_to_fixture(z, "c0_s1_", "c0_s1_", {k: v.cpu() for k, v in none.items()}, dr.run(case, dr.SETTINGS[1]), {})
    # half-precision fields are cast to float32 on entry: the labels of the rounded fields
    half = get_model("roma_gt_matcher")(CONF).eval()(matcher_data(case, half=True))
    rounded = {**case, **{k: case[k].half().float() for k in ("warp0", "warp1", "certainty0", "certainty1")}}
    want = run_gpu(rounded, dr.SETTINGS[0])
    assert torch.equal(half["matches0"].cpu(), want["matches0"]) and half["proj_0to1"].dtype == torch.float32
    with pytest.raises(NotImplementedError, match="RoMa network is not part of this package"):
        get_model("roma_gt_matcher")(CONF).eval()({k: v for k, v in data.items() if k != "warp1"})


@pytest.mark.parametrize("in_forward", [True, False])
def test_pipeline_loss_on_the_labels(z, in_forward):
    """Cached key points (`allow_no_extract`), no extractor, LightGlue with name-seeded weights, the labels in `loss`."""
    from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline

    case = dr.fixture_case(z, 0)
    data = matcher_data(case)
    g = torch.Generator().manual_seed(3)
    item = {k: data[k] for k in ("warp0", "warp1", "certainty0", "certainty1")}
    for s, hw in (("0", case["img0_hw"]), ("1", case["img1_hw"])):
        k = data["keypoints" + s].shape[1]
        cache = {"keypoints": data["keypoints" + s], "keypoint_scores": data["keypoint_scores" + s],
                 "descriptors": torch.nn.functional.normalize(torch.randn((1, k, 128), generator=g), dim=-1).cuda()}
        item["view" + s] = {"image": data["view" + s]["image"], "cache": cache,
                            "image_size": torch.tensor([[float(hw[1]), float(hw[0])]]).cuda()}
    values = []
    for dense in (True, False):
        pipe = TwoViewPipeline({"extractor": {"name": None}, "allow_no_extract": True, "run_gt_in_forward": in_forward,
                                "matcher": {"name": "matchers.lightglue", "weights": "synthetic", "filter_threshold": 0.0,
                                            "flash": False, "input_dim": 128},
                                "ground_truth": {"name": "matchers.roma_gt_matcher", **CONF, "dense_outputs": dense}}).eval().cuda()
        pred = pipe(item)
        assert ("gt_matches0" in pred) == in_forward
        losses, metrics = pipe.loss(pred, item)
        torch.cuda.synchronize()
        assert len(losses) == 8 and len(metrics) == 4
        for k, v in {**losses, **metrics}.items():
            assert bool(torch.isfinite(v).all()), k
        assert int(losses["num_matchable"][0]) == int((z["c0_s0_matches0"] > -1).sum()) > 0
        values.append({k: float(v[0]) for k, v in {**losses, **metrics}.items()})
    assert values[0] == values[1], values  # no row has two positives: the dense assignment adds nothing
