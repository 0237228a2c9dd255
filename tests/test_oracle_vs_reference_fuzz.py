"""Differential sweep of the ORACLE against the reference's own modules on random configurations (CPU): this pins the
restatement on shapes and options the other fixtures do not hold: image sizes that are not multiples of 8, batches,
every NMS radius, thresholds, border widths, top-k above / below the candidate count, RGB input, official legacy / fixed
sampling with image_size, LightGlue on tiny and unequal key-point sets.  The configurations are drawn from seeds
(tests/golden/fuzz_cases.py); what the reference returned for them is tests/golden/reference_fuzz.npz, written by
tests/golden/make_golden.py::golden_reference_fuzz (the reference imported with the omegaconf stand-in, name-seeded
weights, no network).  Descriptors and log-assignment matrices: SAMPLE_ROWS rows element-wise, every row through a
weighted checksum (bounded by what the element-wise tolerance implies); key points as pixel indices (centre - 0.5)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fuzz_cases import (auc_cases, lightglue_cases, row_checksums, row_weights, sample_rows,  # noqa: E402
                        superpoint_official_cases, superpoint_open_cases)


def _keypoints(g, key):
    """The reference's key points: stored as pixel indices (int16), the points are the pixel centres."""
    return g[key].float() + 0.5


def _descriptors_close(g, prefix, d, tol):
    """d [N, D] against the reference's rows `prefix`_sample (element-wise) and `prefix`_checksums (every row; stored
    as float32, whose rounding, below 1e-6 for unit rows, the tolerances leave room for)."""
    rows = g[prefix + "_rows"]
    assert torch.equal(rows, torch.as_tensor(sample_rows(d.shape[0]))), prefix
    err = (d[rows] - g[prefix + "_sample"]).abs().max().item() if len(rows) else 0.0
    c_err = (row_checksums(d) - g[prefix + "_checksums"].double()).abs().max().item() if d.shape[0] else 0.0
    assert err <= tol and c_err <= tol, (prefix, err, c_err)
    return max(err, c_err)


def _log_assignment_close(g, prefix, la, tol):
    """la [R, C] against the reference within |la - ref| <= tol * (1 + |la|) element-wise on the sampled rows, and on
    every row's checksum within the bound that this element-wise tolerance implies: tol * (|w| . (1 + |la|))."""
    rows = g[prefix + "_rows"]
    assert torch.equal(rows, torch.as_tensor(sample_rows(la.shape[0]))), prefix
    ref = g[prefix + "_sample"]
    assert ((ref - la[rows]).abs() / (1 + la[rows].abs())).max().item() <= tol, prefix
    c_err = (row_checksums(la) - g[prefix + "_checksums"]).abs()
    bound = tol * ((1 + la.double().abs()) @ row_weights(la.shape[-1]).abs())
    assert (c_err <= bound).all(), (prefix, (c_err / bound).max().item())


def test_superpoint_open_oracle_equals_reference_on_random_configurations(golden):
    from glue_factory_colon_amd import weights
    from oracle import superpoint as osp

    g = golden("reference_fuzz")
    sd = weights.superpoint_open_state_dict(0)
    checked = ragged = 0
    worst = 0.0
    with torch.no_grad():
        for case, img, conf in superpoint_open_cases():
            b, h, w = img.shape[0], img.shape[-2], img.shape[-1]
            for i in range(b):  # the reference stacks per-image lists: it ran image by image (b == 1 is its eval use)
                o = osp.extract(sd, img[i:i + 1], "open", **conf)  # same batch size: the CPU convolutions block by batch
                key = f"open{case}_{i}"
                assert torch.equal(_keypoints(g, key + "_keypoints"), o["keypoints"][0]), (case, conf, h, w)
                if len(o["keypoints"][0]):
                    es = (g[key + "_keypoint_scores"] - o["keypoint_scores"][0]).abs().max().item()
                    assert es <= 1e-6, (case, conf, h, w, es)
                    ed = _descriptors_close(g, key + "_descriptors", o["descriptors"][0], 1e-5)
                    worst = max(worst, es, ed)
                checked += 1
            ragged += int(h % 8 != 0 or w % 8 != 0)
    print('open: worst float difference', worst)
    assert checked >= 12 and ragged >= 5, (checked, ragged)


def test_superpoint_official_oracle_equals_reference_on_random_configurations(golden):
    from glue_factory_colon_amd import weights
    from oracle import superpoint as osp

    g = golden("reference_fuzz")
    sd = weights.superpoint_state_dict(0)
    checked = 0
    with torch.no_grad():
        for case, img, size, conf in superpoint_official_cases():
            h, w = img.shape[-2:]
            o = osp.extract(sd, img, "official", image_size=size, **conf)
            key = f"official{case}"
            assert torch.equal(_keypoints(g, key + "_keypoints"), o["keypoints"][0]), (case, conf, h, w, size)
            if len(o["keypoints"][0]):
                assert (g[key + "_keypoint_scores"] - o["keypoint_scores"][0]).abs().max().item() <= 1e-6
                _descriptors_close(g, key + "_descriptors", o["descriptors"][0], 1e-5)
            checked += 1
    assert checked == 10


def test_lightglue_oracle_equals_reference_on_random_key_point_sets(golden):
    from glue_factory_colon_amd import weights
    from oracle import lightglue as olg

    g = golden("reference_fuzz")
    sd = weights.lightglue_state_dict(0)
    with torch.no_grad():
        for case, data, th in lightglue_cases():
            kp0, kp1, d0, d1 = data["keypoints0"], data["keypoints1"], data["descriptors0"], data["descriptors1"]
            size = data["view0"]["image_size"]
            (b, m_), n_ = kp0.shape[:2], kp1.shape[1]
            o = olg.match(sd, kp0, kp1, d0, d1, size, size, filter_threshold=th)
            key = f"lg{case}"
            assert torch.equal(g[key + "_matches0"], o["matches0"]) and torch.equal(g[key + "_matches1"], o["matches1"]), \
                (case, m_, n_, th)
            # (measured 1.1e-5; the path's bar is 1e-4)
            assert (g[key + "_matching_scores0"] - o["matching_scores0"]).abs().max().item() <= 5e-5
            la_o = o["log_assignment"]
            assert g[key + "_log_assignment_shape"].tolist() == list(la_o.shape) == [b, m_ + 1, n_ + 1]
            # (the restatement and the reference associate the attention / soft-max sums differently: measured 1.9e-5)
            _log_assignment_close(g, key + "_log_assignment", la_o.reshape(-1, n_ + 1), 5e-5)
            for i in range(b):
                _descriptors_close(g, f"{key}_{i}_ref_descriptors0", o["ref_descriptors0"][i].reshape(m_, -1), 1e-4)


def test_host_side_restatements_against_the_reference(golden):
    """Host logic restated in the package against the reference's own function on random inputs: the AUC of the
    evaluation summaries (utils/tools.py:137-149).  (`read_homography`, datasets/hpatches.py:23-35, is tested on files
    the test writes, tests/test_hpatches_reader.py.)"""
    from glue_factory_colon_amd.eval_hpatches import cal_error_auc

    g = golden("reference_fuzz")
    for n, errors, ths in auc_cases():
        assert [float(a) for a in cal_error_auc(errors, ths)] == g[f"auc{n}_{ths[0]}"].tolist(), (n, ths)
