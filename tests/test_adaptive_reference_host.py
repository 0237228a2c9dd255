"""CPU checks of tests/adaptive_reference.py: the traced loop equals the oracle's `match_adaptive`, and the inputs the
GPU test of the adaptive path shares are fit for it -- judged on the oracle alone, so that the GPU test's exclusion
rules are fixed before any GPU output exists (tests/test_gpu_isolated_small_kernels.py)."""
import pytest
import torch

import adaptive_reference as ar
from oracle import lightglue as olg


@pytest.fixture(scope="module")
def runs():
    d = ar.inputs()
    out = []
    for depth, width, pz in ar.CONFIGS:
        sd = ar.state_dict(pz)
        args = (sd, d["keypoints0"], d["keypoints1"], d["descriptors0"], d["descriptors1"], d["size"], d["size"])
        kw = dict(depth_confidence=depth, width_confidence=width, filter_threshold=ar.FILTER_THRESHOLD)
        out.append((depth, width, args, kw, ar.trace(*args, **kw)))
    return out


def test_trace_equals_match_adaptive(runs):
    for depth, width, args, kw, (layers, final, _, _) in runs:
        ref = olg.match_adaptive(*args, **kw)
        for k, v in ref.items():
            if torch.is_tensor(v):
                assert torch.equal(final[k], v), (depth, width, k)
            else:
                assert final[k] == v, (depth, width, k)
        assert len(layers) == ref["stop_layer"]
        # the kept intermediates are the loop's own: the last layer's rows are the returned descriptors
        assert torch.equal(layers[-1]["x0"], ref["ref_descriptors0"][0, 0])
        assert torch.equal(final["ind0"], (ref["prune0"][0] == ref["prune0"].max()).nonzero().flatten())


def test_inputs_exercise_every_decision_layer(runs):
    for c, (depth, width, _, _, (layers, final, _, _)) in enumerate(runs):
        assert final["stop_layer"] == 9 and len(layers) == 9  # no early stop: all 8 decision layers run
        pruning = sum(1 for r in layers[:-1] if len(r["keep0"]) < r["m"] or len(r["keep1"]) < r["n"])
        if c < 2:
            assert pruning >= 6, (c, pruning)
        assert pruning >= 1
        # the survivors of the last layer, as measured with the oracle when the inputs were chosen: a change of the
        # inputs or weights that collapses (or inflates) the pruning shows here
        assert (layers[-1]["m"], layers[-1]["n"]) == ((658, 663), (135, 147), (1019, 1018))[c], (c, layers[-1]["m"])
        assert (layers[1]["m"], layers[1]["n"]) == ((951, 958), (780, 783), (1024, 1024))[c]
        for i, bd in enumerate(ar.bands(layers, depth, width)):
            assert bd["n_unsure"] <= 0.01 * bd["rows"], (c, i, bd["n_unsure"], bd["rows"])
            if bd["ratio_margin"] is not None:
                assert bd["ratio_margin"] > 1.0, (c, i, bd["ratio_margin"])  # farther than one point from the threshold
        skip0, skip1 = ar.near_tie_rows(final["log_assignment"])
        assert int(skip0.sum()) <= 0.01 * skip0.numel() and int(skip1.sum()) <= 0.01 * skip1.numel()
        assert int((final["matches0"] >= 0).sum()) > 50  # a case with matches to compare
