"""gfc_eval_matches_homography and gfc_eval_homography_dlt (csrc/eval_metrics.hip, through eval_utils) against the float64
checker tests/hpatches_reference.py, at the evaluation's size and around the LDS limits.

Match metrics.  The checker marks the key points and matches whose verdict rests on a decision within DELTA (2e-3 px)
of going the other way; a float32 kernel may differ THERE and nowhere else.  Every case asserts, on the CPU side and
before the kernel's answer is looked at, that at most 1 % of its key points and at most 1 % of its matches are so
marked (the cap of test_gpu_ransac.py); a case that does not meet it is a bad input, not a reason to excuse more.
Asserted per pair: the ground-truth rows that are not undecided equal the checker's exactly; num_matches and
num_keypoints exactly; round(prec@k * num_matches) in [sure, sure + undecided]; recall and precision equal to 1e-6 the
values recomputed in float64 from the kernel's OWN ground-truth rows (the reduction, pinned apart from the verdicts).
Shapes: a batch of three with different matrices, 1800 x 1800 (last below 64 KB of LDS), 1900 x 1800 (first above), 2048 x
2048 (the evaluation), the largest shape the launcher admits and the next one up (refused before any launch), empty
and one-point sides, exact twins, match indices >= N.

DLT.  Per element against the nearer of the checker's two eigenvector signs: |dH_ij| <= 2^-23 |H_ij| + 1e-9 max|H|
(hpatches_cases.py); each case asserts kappa * 2^-52 <= 1e-11 on the CPU side.  The corner error within DELTA.

Not covered: parity with kornia's find_homography_dlt and with OpenCV (neither is available to make vectors from).
The worst measured ratios and the undecided shares go to profiles/eval_homography_parity.json when GFC_WRITE_PROFILES=1.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpatches_cases as hc  # noqa: E402
import hpatches_reference as hr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import eval_utils  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hpatches_metrics.npz")
LDS_LIMIT = 160 * 1024
CAP = 0.01
_record = {"metrics": {}, "dlt": {}}


@pytest.fixture(scope="module", autouse=True)
def _write_profile():
    yield
    if os.environ.get("GFC_WRITE_PROFILES") == "1" and _record["metrics"] and _record["dlt"]:
        with open(os.path.join(ROOT, "profiles", "eval_homography_parity.json"), "w") as f:
            json.dump({"what": "gfc_eval_matches_homography / gfc_eval_homography_dlt against tests/hpatches_reference.py "
                               "(float64): per case the share of key points and matches the checker marks undecided "
                               "(cap 0.01) and how many decided-elsewhere rows differed (must be 0); for the DLT the worst "
                               "|dH_ij| / (2^-23 |H_ij| + 1e-9 max|H|), the worst |d corner error| / 2e-3 px and the worst "
                               "kappa * 2^-52 / 1e-11 (each must be <= 1)",
                       "device": torch.cuda.get_device_name(0), **_record}, f, indent=1)


def run_metrics(case):
    out, gt = eval_utils.match_metrics(case["H"].cuda(), case["kp0"].cuda(), case["kp1"].cuda(), case["m0"].cuda(),
                                       return_gt=True)
    torch.cuda.synchronize()
    return out.cpu().double(), gt.cpu()


def checker(case, i):
    """Float64 verdicts of pair i and the CPU-side condition on the input: at most 1 % undecided."""
    kp0, kp1, H, m0 = case["kp0"][i].double(), case["kp1"][i].double(), case["H"][i].double(), case["m0"][i]
    g = hr.gt_matches(kp0, kp1, H)
    err, und_e = hr.match_errors(kp0, kp1, m0, H)
    nm = int((m0 > -1).sum())
    share_kp = float(g["undecided0"].float().mean()) if len(m0) else 0.0
    share_m = float(und_e.sum()) / max(nm, 1)
    assert share_kp <= CAP and share_m <= CAP, ("bad input: too many undecided", share_kp, share_m)
    return g, err, und_e, nm, share_kp, share_m


def check_metrics(name, case):
    b, m, n = case["kp0"].shape[0], case["kp0"].shape[1], case["kp1"].shape[1]
    assert max(float(case["kp0"].abs().max()) if m else 0.0, float(case["kp1"].abs().max()) if n else 0.0) < 4096
    refs = [checker(case, i) for i in range(b)]  # before the kernel's answer is looked at
    out, gt = run_metrics(case)
    rec = {"shape": [b, m, n], "undecided_keypoint_share": max(r[4] for r in refs),
           "undecided_match_share": max(r[5] for r in refs), "decided_rows_that_differ": 0,
           "undecided_rows_that_differ": 0}
    for i, (g, err, und_e, nm, _, _) in enumerate(refs):
        m0 = case["m0"][i]
        sure = ~g["undecided0"]
        differ = gt[i] != g["matches0"]
        rec["decided_rows_that_differ"] += int((differ & sure).sum())
        rec["undecided_rows_that_differ"] += int((differ & ~sure).sum())
        print(name, i, "undecided", int((~sure).sum()), "of", m, "differ", int(differ.sum()), out[i].tolist())
        assert torch.equal(gt[i][sure], g["matches0"][sure]), (name, i, torch.nonzero(differ & sure).flatten()[:10])
        assert float(out[i, 2]) == nm and float(out[i, 3]) == (m + n) / 2.0
        valid = m0 > -1
        for th, col in ((1.0, 0), (3.0, 1)):
            sure_true = int((valid & ~und_e & (err < th)).sum())
            k = round(float(out[i, col]) * nm)
            assert sure_true <= k <= sure_true + int(und_e.sum()), (name, i, th, k, sure_true, int(und_e.sum()))
            assert abs(float(out[i, col]) - (k / nm if nm else 0.0)) <= 1e-6
        recall, precision = hr.match_ratios(m0, gt[i])  # from the kernel's own ground truth
        assert abs(float(out[i, 4]) - recall) <= 1e-6 and abs(float(out[i, 5]) - precision) <= 1e-6, (name, i)
    _record["metrics"][name] = rec
    return out, gt


def largest_admitted(lds_bytes, m):
    """The largest N the launcher admits beside M = m, from the library's own account of its LDS."""
    n = 0
    while lds_bytes(m, n + 1) <= LDS_LIMIT:
        n += 1
    return n


@pytest.mark.parametrize("m,n", [(130, 67), (67, 130)])
def test_batch_of_three_with_different_matrices(m, n):
    case = hc.metric_case(1, 3, m, n)
    assert not torch.equal(case["H"][0], case["H"][1]) and not torch.equal(case["H"][1], case["H"][2])
    out, gt = check_metrics(f"b3_{m}x{n}", case)
    assert (gt > -1).any() and (gt == -1).any() and (gt == -2).any()
    for i in range(3):  # one pair at a time: bit for bit the row of the batch
        o1, g1 = run_metrics({k: v[i:i + 1] for k, v in case.items()})
        assert torch.equal(o1[0], out[i]) and torch.equal(g1[0], gt[i])


@pytest.mark.parametrize("b,m,n,seed", [(1, 1800, 1800, 1), (1, 1900, 1800, 1), (2, 2048, 2048, 1)])
def test_around_64_kb_and_at_the_evaluation_size(b, m, n, seed):
    lds = nat.lib().gfc_eval_matches_homography_lds_bytes(m, n)
    assert (lds <= 64 * 1024) == ((m, n) == (1800, 1800))
    check_metrics(f"{m}x{n}", hc.metric_case(seed, b, m, n))


def test_largest_admitted_shape_and_the_next_one_refused():
    lds_bytes = nat.lib().gfc_eval_matches_homography_lds_bytes
    m = 4736
    n = largest_admitted(lds_bytes, m)
    assert n >= 4400 and lds_bytes(m, n) <= LDS_LIMIT < lds_bytes(m, n + 1)
    check_metrics(f"limit_{m}x{n}", hc.metric_case(1, 1, m, n))
    # one more key point: refused by the launcher's own arithmetic, nothing is launched
    case = hc.metric_case(1, 1, m, n + 1)
    with pytest.raises(nat.NativeError, match="UNSUPPORTED"):
        eval_utils.match_metrics(case["H"].cuda(), case["kp0"].cuda(), case["kp1"].cuda(), case["m0"].cuda())
    torch.cuda.synchronize()


@pytest.mark.parametrize("edge", ["M0", "N0", "N1", "no_matches"])
def test_empty_and_one_point_sides(edge):
    case = hc.metric_case(2, 2, 130, 67)
    if edge == "M0":
        case.update(kp0=case["kp0"][:, :0], m0=case["m0"][:, :0])
    elif edge == "N0":
        case.update(kp1=case["kp1"][:, :0], m0=torch.full_like(case["m0"], -1))
    elif edge == "N1":
        case.update(kp1=case["kp1"][:, :1].contiguous(), m0=torch.where(case["m0"] == 0, case["m0"], torch.full_like(case["m0"], -1)))
        case["m0"][:, 3] = 0
    else:
        case.update(m0=torch.full_like(case["m0"], -1))
    out, gt = check_metrics(edge, case)
    if edge == "N0":
        assert (gt == -1).all()
    if edge in ("M0", "N0", "no_matches"):
        assert (out[:, [0, 1, 2, 4, 5]] == 0).all()


def test_twins_the_lower_index_wins_exactly():
    """Case 2 of the reference's fixture: bit-identical copies of a true correspondence in kp1 and in kp0.  No value of it is
    undecided (test_hpatches_reference_host.py), so the kernel must give the reference's integers, all of them."""
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[f"{k}_2"])[None]  # noqa: E731
    case = {"H": t("H"), "kp0": t("kp0"), "kp1": t("kp1"), "m0": t("matches0")}
    out, gt = check_metrics("twins", case)
    assert _record["metrics"]["twins"]["undecided_keypoint_share"] == 0
    assert np.array_equal(gt[0].numpy(), z["gt_matches0_2"])
    (i_lo, i_hi), (j_lo, j_hi), i = z["dup0_2"], z["dup1_2"], int(z["dup_row_2"])
    assert int(gt[0, i]) == j_lo and int(gt[0, i_lo]) > -1 and int(gt[0, i_hi]) == -2
    assert np.abs(out[0].numpy() - z["metrics_2"]).max() <= 1e-6
    # the other way round (images swapped, H inverted): the twins of kp0 are now the columns
    Hinv = torch.linalg.inv(case["H"].double()).float()
    swapped = {"H": Hinv, "kp0": case["kp1"], "kp1": case["kp0"], "m0": torch.full((1, case["kp1"].shape[1]), -1)}
    _, gt1 = check_metrics("twins_swapped", swapped)
    assert int(gt1[0, j_lo]) == i and int(gt1[0, j_hi]) == -2 and int(gt1[0, int(z["gt_matches0_2"][i_lo])]) == i_lo


def test_match_indices_beyond_n():
    """An index >= N names no key point: never read, counted in num_matches, infinite error, equal to no ground truth."""
    case = hc.metric_case(3, 2, 130, 67)
    plain, gt_plain = run_metrics(case)
    n = case["kp1"].shape[1]
    rows_n, rows_n5 = [2, 30, 64], [9, 100]  # matched and unmatched rows alike
    was = case["m0"][:, rows_n + rows_n5] > -1
    case["m0"][:, rows_n] = n
    case["m0"][:, rows_n5] = n + 5
    out, gt = check_metrics("beyond_n", case)
    assert torch.equal(gt, gt_plain)
    assert torch.equal(out[:, 2], plain[:, 2] + (~was).sum(1))
    for i in range(2):
        err, _ = hr.match_errors(case["kp0"][i].double(), case["kp1"][i].double(), case["m0"][i], case["H"][i].double())
        assert bool(torch.isinf(err[rows_n + rows_n5]).all())
        assert float(out[i, 1]) <= 1.0 - 5 / float(out[i, 2]) + 1e-6  # five matches can be in no prec@


# ---- weighted DLT ----------------------------------------------------------------------------------------------------
def run_dlt(items):
    s = hc.stack(items)
    size = hc.SIZE.repeat(len(items), 1)
    Hd, err = eval_utils.homography_dlt(s["H"].cuda(), s["kp0"].cuda(), s["kp1"].cuda(), s["m0"].cuda(), s["scores"].cuda(),
                                        size.cuda())
    torch.cuda.synchronize()
    return Hd.cpu().double(), err.cpu().double()


@pytest.mark.parametrize("name", ["noise0", "noise07", "noise2", "scale", "four", "three", "out_of_range",
                                  "weighted_outliers"])
def test_dlt_against_the_checker(name):
    items = hc.dlt_cases()[name]
    assert len(items) > 1
    refs = [hr.dlt(it["kp0"], it["kp1"], it["m0"], it["scores"], it["H"], hc.SIZE) for it in items]
    for r in refs:  # the condition the bound rests on, on the CPU side
        assert r["kappa"] == float("inf") or r["kappa"] * 2.0**-52 <= 1e-11, (name, r["kappa"])
    Hd, err = run_dlt(items)
    rec = {"H_ratio": 0.0, "corner_ratio": 0.0, "kappa_ratio": 0.0}
    for i, r in enumerate(refs):
        if r["err"] == float("inf"):
            assert name == "three" and bool(torch.isinf(Hd[i]).all()) and bool((Hd[i] > 0).all()) and float(err[i]) == float("inf")
            continue
        ratios = []
        for s in range(2):
            bound = hc.DLT_BOUND_REL * r["H"][s].abs() + hc.DLT_BOUND_ABS * r["H"][s].abs().max()
            ratios.append(float(((Hd[i] - r["H"][s]).abs() / bound).max()))
        corner = abs(float(err[i]) - r["err"]) / hr.DELTA
        print(name, i, "H ratio", min(ratios), "corner", float(err[i]), r["err"], "kappa", r["kappa"])
        rec = {"H_ratio": max(rec["H_ratio"], min(ratios)), "corner_ratio": max(rec["corner_ratio"], corner),
               "kappa_ratio": max(rec["kappa_ratio"], r["kappa"] * 2.0**-52 / 1e-11)}
        assert min(ratios) <= 1.0, (name, i, ratios, Hd[i], r["H"])
        assert corner <= 1.0, (name, i, float(err[i]), r["err"])
    _record["dlt"][name] = rec
    if name == "three":
        assert all(r["err"] == float("inf") for r in refs)
    if name == "weighted_outliers":  # and the un-weighted answer is far outside the bound (the host test shows > 100 x)
        for i, it in enumerate(items):
            flat = hr.dlt(it["kp0"], it["kp1"], it["m0"], it["scores"], it["H"], hc.SIZE, use_weights=False)
            assert abs(float(err[i]) - flat["err"]) > 100 * hr.DELTA


def test_dlt_degenerate_input_is_inf_or_finite_never_nan():
    Hd, err = run_dlt(hc.degenerate_dlt_batch())
    assert not bool(torch.isnan(Hd).any()) and not bool(torch.isnan(err).any())
    for i in range(len(err)):
        all_inf = bool((Hd[i] == float("inf")).all())
        assert all_inf or bool(torch.isfinite(Hd[i]).all()), Hd[i]
        assert (float(err[i]) == float("inf")) == all_inf, (i, Hd[i], err[i])
    assert bool(torch.isfinite(Hd[2]).all()) and float(err[2]) < 5.0  # the ordinary item beside them is untouched
