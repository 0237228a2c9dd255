"""tests/hpatches_reference.py (the float64 checker of the HPatches match-metric and DLT kernels) against vectors the
reference project produced: tests/golden/hpatches_metrics.npz, written by tests/golden/make_golden_hpatches.py.  No GPU.

What is pinned: ground-truth matches of both images and the threshold verdicts exactly, in float64 AND in float32;
per-match errors, warps and the corner error to 1e-9 in float64; the six metrics; that no value of the seeded cases is
undecided (so nothing here is excused); that the fixture tells each deliberately wrong rule (hr.WRONG_RULES) from the
right one.  The weighted DLT has no reference vectors (the reference delegates to kornia's find_homography_dlt, absent
where the fixture is made): it is pinned by what defines it, and parity with kornia's solver and with OpenCV stays
unpinned.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpatches_reference as hr  # noqa: E402
from hpatches_cases import DLT_BOUND_ABS, DLT_BOUND_REL, dlt_cases  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpatches_metrics.npz")
SEEDED, EXACT = (0, 1, 2, 3), 4  # case 4 sits on pos_th by construction (make_golden_hpatches.py)
SIZE = torch.tensor([640.0, 480.0])


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case(fx, c, dtype):
    t = lambda k: torch.from_numpy(fx[f"{k}_{c}"])  # noqa: E731
    return t("kp0").to(dtype), t("kp1").to(dtype), t("matches0"), t("H").to(dtype)


def test_fixture_shapes_and_contents(fx):
    assert [fx[f"kp0_{c}"].shape[0] for c in SEEDED] == [130, 130, 300, 300]
    assert [fx[f"kp1_{c}"].shape[0] for c in SEEDED] == [67, 67, 257, 257]
    assert np.abs(fx["H_1"][2, :2]).min() > 0 and np.abs(fx["H_2"][2, :2]).min() > 0 and (fx["H_0"][2, :2] == 0).all()
    for c in SEEDED:
        g = fx[f"gt_matches0_{c}"]
        assert (g > -1).sum() > 20 and (g == -1).sum() > 20 and (g == -2).sum() > 0, c
        e = fx[f"err_{c}"]
        assert (e < 1).any() and ((e >= 1) & (e < 3)).any() and (e >= 3).any()
        assert max(np.abs(fx[f"kp0_{c}"]).max(), np.abs(fx[f"kp1_{c}"]).max()) < 4096
    # the twins of case 2 are bit-identical copies, and the lower index carries the match on both sides
    (i_lo, i_hi), (j_lo, j_hi), i = fx["dup0_2"], fx["dup1_2"], int(fx["dup_row_2"])
    assert (fx["kp0_2"][i_lo] == fx["kp0_2"][i_hi]).all() and (fx["kp1_2"][j_lo] == fx["kp1_2"][j_hi]).all()
    g0, g1 = fx["gt_matches0_2"], fx["gt_matches1_2"]
    assert g0[i] == j_lo and g1[j_lo] == i and g1[j_hi] == -2
    assert g0[i_lo] > -1 and g1[g0[i_lo]] == i_lo and g0[i_hi] == -2


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("c", SEEDED + (EXACT,))
def test_checker_equals_the_fixture(fx, c, dtype):
    kp0, kp1, m0, H = case(fx, c, dtype)
    g = hr.gt_matches(kp0, kp1, H)
    assert np.array_equal(g["matches0"].numpy(), fx[f"gt_matches0_{c}"])
    assert np.array_equal(g["matches1"].numpy(), fx[f"gt_matches1_{c}"])
    err, _ = hr.match_errors(kp0, kp1, m0, H)
    e = err[m0 > -1].numpy()
    for th in (1, 3):
        assert np.array_equal(e < th, fx[f"err_{c}"] < th)
    got = hr.metrics(kp0, kp1, m0, H)
    want = fx[f"metrics_{c}"]
    assert got[2] == want[2] and got[3] == want[3]
    # the reference's ratios are float32 divisions: 1e-6 is eight float32 roundings of a ratio <= 1
    assert np.abs(np.array(got) - want)[[0, 1, 4, 5]].max() <= 1e-6, (got, want)
    if dtype == torch.float64:
        assert np.abs(e - fx[f"err_f64_{c}"]).max() <= 1e-9
        assert np.abs(hr.warp(kp0, H, 1e-5).numpy() - fx[f"warp_fwd_f64_{c}"]).max() <= 1e-9
        assert np.abs(hr.warp(kp1, torch.linalg.inv(H), 1e-5).numpy() - fx[f"warp_inv_f64_{c}"]).max() <= 1e-9
        H_off = H + torch.tensor([[0, 0, 1.5], [0, 0, -2.5], [0, 0, 0.0]], dtype=dtype)
        assert abs(hr.corner_error(H_off, H, SIZE) - float(fx[f"corner_err_f64_{c}"])) <= 1e-9
        # (the reference forms its ratios from float32 masks whatever the inputs: metrics_f64 is no float64 figure)
        assert np.abs(np.array(got) - fx[f"metrics_f64_{c}"]).max() <= 1e-6


@pytest.mark.parametrize("c", SEEDED)
def test_no_fixture_value_is_undecided(fx, c):
    kp0, kp1, m0, H = case(fx, c, torch.float64)
    g = hr.gt_matches(kp0, kp1, H)
    _, und = hr.match_errors(kp0, kp1, m0, H)
    assert int(g["undecided0"].sum()) == 0 and int(g["undecided1"].sum()) == 0 and int(und.sum()) == 0


def test_undecided_flags_fire_where_they_should(fx):
    """The exact-threshold case IS undecided; a twin is not, but the same point moved by 1e-3 px is."""
    kp0, kp1, m0, H = case(fx, EXACT, torch.float64)
    g = hr.gt_matches(kp0, kp1, H)
    assert bool(g["undecided0"][0]) and bool(g["undecided1"][0]) and not g["undecided0"][1:].any()
    kp0, kp1, m0, H = case(fx, 2, torch.float64)
    j_lo, j_hi = fx["dup1_2"]
    i = int(fx["dup_row_2"])
    kp1 = kp1.clone()
    kp1[j_hi, 0] += 1e-3
    g = hr.gt_matches(kp0, kp1, H)
    assert bool(g["undecided0"][i]) and bool(g["undecided1"][j_lo]) and bool(g["undecided1"][j_hi])
    # an error within DELTA of 1 px: kp1 = warp(kp0) + (1 + 1e-3, 0) under a pure translation
    a = torch.tensor([[10.0, 10.0], [50.0, 60.0]], dtype=torch.float64)
    T = torch.tensor([[1.0, 0, 5], [0, 1.0, 7], [0, 0, 1]], dtype=torch.float64)
    b = hr.warp(a, T) + torch.tensor([[1.0 + 1e-3, 0.0], [0.5, 0.0]], dtype=torch.float64)
    err, und = hr.match_errors(a, b, torch.tensor([0, 1]), T)
    assert und.tolist() == [True, False] and abs(float(err[0]) - 1.001) < 1e-9
    # an index >= N is an infinite error, no match is NaN
    err, und = hr.match_errors(a, b, torch.tensor([2, -1]), T)
    assert float(err[0]) == float("inf") and bool(torch.isnan(err[1])) and not und.any()


@pytest.mark.parametrize("rule", hr.WRONG_RULES)
def test_fixture_rejects_wrong_rules(fx, rule):
    differs = 0
    for c in SEEDED + (EXACT,):
        kp0, kp1, m0, H = case(fx, c, torch.float64)
        g = hr.gt_matches(kp0, kp1, H, rule=rule)
        differs += int(not (np.array_equal(g["matches0"].numpy(), fx[f"gt_matches0_{c}"])
                            and np.array_equal(g["matches1"].numpy(), fx[f"gt_matches1_{c}"])))
    assert differs > 0, rule
    # and each is rejected by the case built for it
    c = {"last_index_ties": 2, "dist_negatives": 2, "pos_le": EXACT}[rule]
    kp0, kp1, m0, H = case(fx, c, torch.float64)
    assert not np.array_equal(hr.gt_matches(kp0, kp1, H, rule=rule)["matches0"].numpy(), fx[f"gt_matches0_{c}"])
    assert hr.metrics(kp0, kp1, m0, H, rule=rule)[4:] != hr.metrics(kp0, kp1, m0, H)[4:]


def test_chunking_does_not_change_the_answer(fx):
    kp0, kp1, m0, H = case(fx, 2, torch.float64)
    a, b = hr.gt_matches(kp0, kp1, H, chunk=7), hr.gt_matches(kp0, kp1, H, chunk=4096)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for rule in hr.WRONG_RULES:
        a, b = hr.gt_matches(kp0, kp1, H, rule=rule, chunk=7), hr.gt_matches(kp0, kp1, H, rule=rule, chunk=4096)
        assert torch.equal(a["matches0"], b["matches0"]) and torch.equal(a["matches1"], b["matches1"])


def test_empty_sides():
    H = torch.eye(3, dtype=torch.float64)
    kp = torch.rand((5, 2), dtype=torch.float64) * 100
    none = kp[:0]
    g = hr.gt_matches(kp, none, H)
    assert g["matches0"].tolist() == [-1] * 5 and g["matches1"].numel() == 0 and not g["undecided0"].any()
    g = hr.gt_matches(none, kp, H)
    assert g["matches1"].tolist() == [-1] * 5 and g["matches0"].numel() == 0
    assert hr.metrics(kp, none, torch.full((5,), -1), H) == [0.0, 0.0, 0.0, 2.5, 0.0, 0.0]
    assert hr.metrics(none, kp, torch.zeros(0, dtype=torch.long), H) == [0.0, 0.0, 0.0, 2.5, 0.0, 0.0]


# ---- weighted DLT ----------------------------------------------------------------------------------------------------


def test_dlt_exact_correspondences_recover_h():
    cases = dlt_cases()
    for name in ("noise0", "scale", "four"):
        for item in cases[name]:
            r = hr.dlt(item["kp0"], item["kp1"], item["m0"], item["scores"], item["H"], SIZE)
            Hgt = item["H"].double() / item["H"].double()[2, 2]
            # float32 key points: the correspondences are exact to half an ulp of a coordinate (3e-5 px at 640)
            assert (r["H"][0] - Hgt).abs().max() <= 1e-4 * Hgt.abs().max(), (name, r["H"][0], Hgt)
            assert r["err"] < 1e-3, (name, r["err"])
            assert (r["H"][0] - r["H"][1]).abs().max() <= 1e-6 * Hgt.abs().max()


def test_dlt_too_few_and_out_of_range():
    cases = dlt_cases()
    for item in cases["three"]:
        r = hr.dlt(item["kp0"], item["kp1"], item["m0"], item["scores"], item["H"], SIZE)
        assert torch.isinf(r["H"]).all() and r["err"] == float("inf") and r["kappa"] == float("inf")
    for item in cases["out_of_range"]:
        n = item["kp1"].shape[0]
        assert int((item["m0"] >= n).sum()) >= 2
        keep = torch.where(item["m0"] >= n, torch.full_like(item["m0"], -1), item["m0"])
        a = hr.dlt(item["kp0"], item["kp1"], item["m0"], item["scores"], item["H"], SIZE)
        b = hr.dlt(item["kp0"], item["kp1"], keep, item["scores"], item["H"], SIZE)
        assert torch.equal(a["H"], b["H"]) and a["err"] == b["err"]


def test_dlt_cases_are_well_conditioned_and_the_weights_matter():
    """What the GPU test leans on, shown on the CPU: every case's eigen-problem is conditioned so that a float64 solver's
    error (kappa * 2^-52) is 100 x below the absolute term of the GPU bound, and on the weighted-outlier case dropping
    the weights moves H by more than 100 x that bound -- a kernel that ignored the weights could not pass."""
    cases = dlt_cases()
    for name, items in cases.items():
        for item in items:
            r = hr.dlt(item["kp0"], item["kp1"], item["m0"], item["scores"], item["H"], SIZE)
            if r["kappa"] != float("inf"):
                assert r["kappa"] * 2.0**-52 <= 1e-11, (name, r["kappa"])
    for item in cases["weighted_outliers"]:
        a = hr.dlt(item["kp0"], item["kp1"], item["m0"], item["scores"], item["H"], SIZE)
        b = hr.dlt(item["kp0"], item["kp1"], item["m0"], item["scores"], item["H"], SIZE, use_weights=False)
        bound = DLT_BOUND_REL * a["H"][0].abs() + DLT_BOUND_ABS * a["H"][0].abs().max()
        assert ((a["H"][0] - b["H"][0]).abs() / bound).max() > 100
        assert abs(a["err"] - b["err"]) > 100 * hr.DELTA
        assert a["err"] < 1.0 < b["err"]  # the down-weighted outliers barely move the estimate; unweighted they do


def test_lds_account_of_the_match_metric_kernels():
    """What the launchers count (host arithmetic, no GPU): the dynamic arrays of the kernel plus its static LDS, and a
    pair is admitted exactly up to 160 KB.  M = 4736, N = 4400 (arrays of 163 776 bytes) is within the limit once the
    static part is counted as itself and no longer as 64 bytes on top of a dynamic request that already held 64."""
    from glue_factory_colon_amd import _native as nat

    lib, limit = nat.lib(), 160 * 1024
    hom, dep = lib.gfc_eval_matches_homography_lds_bytes, lib.gfc_eval_matches_depth_lds_bytes
    for f, per_m, per_n in ((hom, 16, 20), (dep, 24, 28)):
        static = f(0, 0)
        assert 0 < static <= 64 and static % 16 == 0
        for m, n in ((1, 0), (0, 1), (2048, 2048), (4736, 4400), (3150, 3149)):
            assert f(m, n) == per_m * m + per_n * n + static
        assert f(-1, 5) == 0
    assert hom(4736, 4400) == 163776 + hom(0, 0) <= limit
    assert hom(1800, 1800) <= 64 * 1024 < hom(1900, 1800) and dep(1250, 1250) <= 64 * 1024 < dep(1300, 1250)
    assert dep(3150, 3149) <= limit < dep(3150, 3150)
