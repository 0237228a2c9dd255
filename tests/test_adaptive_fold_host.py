"""CPU checks of the 128-d and add_scale_ori cases of tests/adaptive_pairs_reference.py, on the oracle alone: what the
GPU tests of the adaptive paths with an input projection and with scales / orientations
(tests/test_gpu_adaptive_pairs.py) may excuse, and that their add_scale_ori configuration prunes and stops nothing, is
fixed before any GPU output exists."""
import torch

import adaptive_pairs_reference as apr
import adaptive_reference as ar
from oracle import lightglue as olg

MIN_MARGIN = 2.0   # points between every stop ratio and depth_confidence, as tests/test_adaptive_pairs_host.py


def test_128d_pairs_prune_and_at_most_one_has_band_rows():
    depth, width = apr.CONFIG_128
    runs = apr.traced128()
    assert "input_proj.weight" in apr.state_dict128()
    with_band = 0
    for p, (d, (layers, final, bands)) in enumerate(zip(apr.inputs128(), runs)):
        m, n = apr.SHAPES[apr.PAIRS_128[p]]
        assert d["descriptors0"].shape == (1, m, 128) and d["descriptors1"].shape == (1, n, 128)
        assert float((d["descriptors0"].norm(dim=-1) - 1).abs().max()) < 1e-6
        rows = [r["m"] + r["n"] for r in layers]
        margins = [bd["ratio_margin"] for bd in bands if bd["ratio_margin"] is not None]
        band = sum(bd["n_unsure"] for bd in bands)
        print(f"128-d pair {p}: stop {final['stop_layer']}, rows {rows}, min ratio margin {min(margins):.2f} points, "
              f"band rows {band}")
        assert rows[-1] < rows[0], (p, rows)   # pruned at one layer at least
        assert final["ind0"].numel() > 0 and final["ind1"].numel() > 0
        assert min(margins) >= MIN_MARGIN, (p, margins)
        with_band += band > 0
    assert with_band <= 1
    # the two pairs as the oracle gave them when (depth, width) were chosen: four pruning layers, stop after the fifth
    assert [final["stop_layer"] for _, final, _ in runs] == [5, 5]


def test_scale_ori_case_keeps_every_point_at_every_layer():
    d, sd, ref = apr.scale_ori_case()
    assert d["keypoints0"].shape == (1, 65, 2) and d["keypoints1"].shape == (1, 64, 2)
    assert d["scale_ori0"].shape == (1, 65, 2) and d["scale_ori1"].shape == (1, 64, 2)
    keep_thr = 1 - apr.SCALE_ORI_WIDTH
    lowest = 1.0
    for i, (x0, x1) in enumerate(ref["layers"][:-1]):
        for x in (x0, x1):
            sc = torch.sigmoid(olg._linear(sd, f"log_assignment.{i}.matchability", x))
            lowest = min(lowest, float(sc.min()))
    print(f"add_scale_ori: lowest matchability {lowest:.4f}, keep threshold {keep_thr:.1e}")
    assert lowest > keep_thr + ar.DELTA
    assert int((ref["matches0"] >= 0).sum()) > 20   # a real assignment, not the empty one
