"""BASELINE.json configs[3] at its per-GPU batch: 32 pairs of 1024 x 1024 images, 2048 key points (256 pairs over 8
GPUs), through extractor and matcher exactly as `bench.py --workload c4` does (both views in one extractor call of
64 images, `force_num_keypoints`).

Only at this batch does the library dispatch the kernel variants that workload is timed on: `attention_kernel<2>` on
2048 x 2048 problems (64 problems x 4 heads x 8 query blocks), the 128 x 128 GEMM tile and the row-owning FFN GEMM on
131072 rows, the two-sweep assignment tail on a [32, 2049, 2049] matrix (537 MB).  Checked here:
  * 4 of the 32 pairs against THE REFERENCE ITSELF (tests/golden/c4_pairs.npz: the reference's TwoViewPipeline on
    the same pairs in the build container, make_golden.py::golden_c4_pairs): key points, scores, descriptors and
    matches0 / matches1 / matching scores index by index through the key-point correspondence;
  * the matcher stage-isolated AT THIS BATCH: the features of those 4 pairs as the batch-32 matcher call received
    them, through the CPU oracle's matcher -> `torch.equal(matches0 / matches1)` with the rows of the batch-32 output;
  * 2 of the 32 pairs end to end against the live CPU oracle (reference path restated, oracle/): key-point sets
    (0 unexplained flips), matched coordinate pairs, scores <= 1e-4 (GFC_TEST_ORACLE_PAIRS=9 for the round-5 spread);
  * batch invariance: all 32 pairs identical on every integer output (key points, matches0/1) -- and within 1e-4 on
    the scores -- to the same pairs run 2 at a time (other GEMM tile, attention_kernel<1>).
Reference: gluefactory/models/matchers/lightglue.py:422-553, extractors/superpoint_open.py:126-232.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from glue_factory_colon_amd import lightglue, superpoint_open, synthetic, weights  # noqa: E402
from oracle import lightglue as olg  # noqa: E402
from oracle import superpoint as osp  # noqa: E402
from parity_utils import compare_keypoints, compare_with_reference_pair, image_sha256, match_pairs, record  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from bench_inputs import C4_PAIRS  # noqa: E402

DEV = "cuda"
H, W, K, B = 1024, 1024, 2048, 32
ORACLE_PAIRS = (0, 3, 7, 12, 16, 21, 26, 29, 31) if int(os.environ.get("GFC_TEST_ORACLE_PAIRS", 2)) >= 9 else (7, 26)


def run_batch(ext, mat, v0, v1):
    """bench.py::step on a list of pairs."""
    b = v0.shape[0]
    size = torch.tensor([[float(W), float(H)]] * b, device=DEV)
    torch.manual_seed(7)  # pad_random_c (only used when an image has fewer than K detections)
    pj = ext({"image": torch.cat([v0, v1], 0), "image_size": torch.cat([size, size], 0)})
    p0 = {k: v[:b] for k, v in pj.items()}
    p1 = {k: v[b:] for k, v in pj.items()}
    out = mat({"keypoints0": p0["keypoints"], "keypoints1": p1["keypoints"], "descriptors0": p0["descriptors"],
               "descriptors1": p1["descriptors"], "view0": {"image_size": size}, "view1": {"image_size": size}})
    return p0, p1, out


@pytest.fixture(scope="module")
def c4_batch32():
    v0, v1 = synthetic.synthetic_pairs(B, H, W, seed=1234, device=DEV)  # bench.py --workload c4, rank 0 inputs
    ext = superpoint_open.SuperPoint({"weights": "synthetic", "max_num_keypoints": K, "detection_threshold": 0.0,
                                      "nms_radius": 3, "force_num_keypoints": True}).eval().to(DEV)
    mat = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.1, "depth_confidence": -1,
                               "width_confidence": -1}).eval().to(DEV)
    with torch.no_grad():
        p0, p1, out = run_batch(ext, mat, v0, v1)
    torch.cuda.synchronize()
    return v0, v1, ext, mat, p0, p1, out


def test_c4_batch32_vs_oracle(c4_batch32):
    v0, v1, _, _, p0, p1, out = c4_batch32
    sd_sp, sd_lg = weights.superpoint_open_state_dict(0), weights.lightglue_state_dict(0)
    size = torch.tensor([[float(W), float(H)]])
    n_ref_total = n_same = 0
    worst = 0.0
    for i in ORACLE_PAIRS:
        imgs = torch.cat([v0[i:i + 1], v1[i:i + 1]], 0).cpu()
        o = osp.extract(sd_sp, imgs, "open", nms_radius=3, max_num_keypoints=K, detection_threshold=0.0)
        okp, osc, ode = torch.stack(o["keypoints"]), torch.stack(o["keypoint_scores"]), torch.stack(o["descriptors"])
        assert okp.shape == (2, K, 2)  # every image of this workload has more than K detections: no padding
        for side, p in ((0, p0), (1, p1)):
            compare_keypoints(f"c4_b32_pair{i}_view{side}", p["keypoints"][i], p["keypoint_scores"][i],
                              p["descriptors"][i], okp[side], osc[side], ode[side], radius=3)
        ref = olg.match(sd_lg, okp[:1], okp[1:], ode[:1], ode[1:], size, size, filter_threshold=0.1)
        mine = match_pairs(p0["keypoints"][i], p1["keypoints"][i], out["matches0"][i])
        theirs = match_pairs(okp[0], okp[1], ref["matches0"][0])
        n_ref_total += len(theirs)
        n_same += len(mine & theirs)
        assert len(theirs) > 1000
        assert mine == theirs, (i, len(mine), len(theirs), len(mine ^ theirs))  # measured: identical since round 2

        def by_pair(kp0, kp1, m0, s0):
            kp0, kp1, m0, s0 = kp0.cpu(), kp1.cpu(), m0.cpu(), s0.cpu()
            return {(*kp0[a].tolist(), *kp1[int(m0[a])].tolist()): float(s0[a])
                    for a in (m0 >= 0).nonzero().flatten().tolist()}
        sm = by_pair(p0["keypoints"][i], p1["keypoints"][i], out["matches0"][i], out["matching_scores0"][i])
        sr = by_pair(okp[0], okp[1], ref["matches0"][0], ref["matching_scores0"][0])
        err = max(abs(sm[q] - sr[q]) for q in set(sm) & set(sr))
        worst = max(worst, err)
        assert err < 1e-4, (i, err)  # north star: scores within 1e-4 fp32
    record("c4_batch32_vs_oracle", pairs=len(ORACLE_PAIRS), ref_matches=n_ref_total, identical=n_same, score_err=worst)


def test_c4_batch32_vs_reference_fixture(c4_batch32, golden):
    """Four pairs of the batch against what the reference itself produced for them."""
    v0, v1, _, _, p0, p1, out = c4_batch32
    g = golden("c4_pairs")
    assert tuple(g["pair_ids"].tolist()) == C4_PAIRS
    n_ref = n_idx = 0
    worst = 0.0
    for j, i in enumerate(C4_PAIRS):
        assert image_sha256(v0[i], v1[i]) == str(g["image_sha256"][j]), i  # the fixture's inputs ARE these images
        r, n, w = compare_with_reference_pair(f"c4_b32_pair{i}", g, j, p0, p1, out, i, radius=3, min_matches=1000)
        n_ref, n_idx, worst = n_ref + r, n_idx + n, max(worst, w)
    record("c4_batch32_vs_reference", pairs=len(C4_PAIRS), ref_matches=n_ref, indices_compared=n_idx,
           indices_identical=n_idx, matching_score_err=worst)


def test_c4_batch32_matcher_stage_isolated(c4_batch32):
    """Rows C4_PAIRS of the ONE matcher call on 32 pairs (attention_kernel<2> on 2048 x 2048 problems, 128 x 128 GEMM
    tiles, the two-sweep assignment tail), element-wise: the same inputs through the CPU oracle's matcher must give the
    same matches0 / matches1, index by index (lightglue.py:294-319)."""
    _, _, _, _, p0, p1, out = c4_batch32
    sd_lg = weights.lightglue_state_dict(0)
    size = torch.tensor([[float(W), float(H)]])
    rows = torch.tensor(C4_PAIRS)
    s_err = la_err = 0.0
    n_matches = 0
    for i in C4_PAIRS:  # one pair per oracle call: [1, 4, 2048, 2048] attention tensors
        ref = olg.match(sd_lg, p0["keypoints"][i:i + 1].cpu(), p1["keypoints"][i:i + 1].cpu(),
                        p0["descriptors"][i:i + 1].cpu(), p1["descriptors"][i:i + 1].cpu(), size, size, filter_threshold=0.1)
        for key in ("matches0", "matches1"):
            assert torch.equal(out[key][i:i + 1].cpu(), ref[key]), (i, key, int((out[key][i:i + 1].cpu() != ref[key]).sum()))
        for key in ("matching_scores0", "matching_scores1"):
            s_err = max(s_err, float((out[key][i:i + 1].cpu() - ref[key]).abs().max()))
        la = ref["log_assignment"]
        la_err = max(la_err, float(((out["log_assignment"][i:i + 1].cpu() - la).abs() / (1 + la.abs())).max()))
        n_matches += int((ref["matches0"] >= 0).sum())
    assert n_matches > 1000 * len(C4_PAIRS)
    assert s_err < 1e-4 and la_err < 1e-4, (s_err, la_err)
    record("c4_batch32_matcher_stage_isolated", matcher_stage_isolated_identical=f"{len(rows)}/{len(rows)} (of a batch of {B})",
           matches=n_matches, matching_score_err=s_err, log_assignment_rel_err=la_err)


def test_c4_batch32_batch_invariance(c4_batch32):
    v0, v1, ext, mat, p0, p1, out = c4_batch32
    keys_ext_exact = ("keypoints", "keypoint_scores", "descriptors")
    assert (p0["keypoint_scores"] > 0).all() and (p1["keypoint_scores"] > 0).all()  # no random padding anywhere
    # structural properties of the full batch (filter_matches, lightglue.py:294-319)
    m0, m1 = out["matches0"], out["matches1"]
    assert m0.dtype == torch.long and m0.shape == (B, K) and int(m0.max()) < K and int(m0.min()) >= -1
    ok = m0 >= 0
    back = torch.gather(m1, 1, m0.clamp(min=0))
    assert torch.equal(back[ok], torch.arange(K, device=DEV).expand(B, K)[ok])  # mutual consistency
    assert int(ok.sum(1).min()) > 1000
    worst = 0.0
    with torch.no_grad():
        for s in range(0, B, 2):  # 2 at a time: 64 x 64 GEMM tiles, attention_kernel<1>
            q0, q1, o2 = run_batch(ext, mat, v0[s:s + 2], v1[s:s + 2])
            for k in keys_ext_exact:
                assert torch.equal(q0[k], p0[k][s:s + 2]) and torch.equal(q1[k], p1[k][s:s + 2]), (s, k)
            assert torch.equal(o2["matches0"], m0[s:s + 2]), s
            assert torch.equal(o2["matches1"], m1[s:s + 2]), s
            worst = max(worst, float((o2["matching_scores0"] - out["matching_scores0"][s:s + 2]).abs().max()),
                        float((o2["matching_scores1"] - out["matching_scores1"][s:s + 2]).abs().max()))
    assert worst < 1e-4, worst
    record("c4_batch32_batch_invariance", score_diff_vs_batch2=worst)
