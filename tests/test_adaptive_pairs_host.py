"""CPU checks of tests/adaptive_pairs_reference.py: the four shared pairs make the oracle stop at different layers, prune
at every layer, and leave few points near a threshold -- judged on the oracle alone, so that what the GPU test of the
batched adaptive path (tests/test_gpu_adaptive_pairs.py) may excuse is fixed before any GPU output exists."""
import adaptive_pairs_reference as apr
import adaptive_reference as ar

# stop layers per pair, as the oracle gave them when the inputs were chosen
STOP_LAYERS = {0.85: (7, 3, 3, 3), 0.89: (9, 3, 3, 9)}
MAX_BAND_ROWS = 6   # per pair, summed over its layers, at ar.DELTA
MAX_BAND_ROWS_PRUNE_ONLY = 8   # the same count over the nine layers of the prune-only trace
MIN_MARGIN = 2.0   # points between every stop ratio and depth_confidence


def _band_rows(bands):
    return sum(bd["n_unsure"] for bd in bands)


def test_inputs_have_the_documented_shapes():
    for d, (m, n) in zip(apr.inputs(), apr.SHAPES):
        assert d["keypoints0"].shape == (1, m, 2) and d["keypoints1"].shape == (1, n, 2)
        assert d["descriptors0"].shape == (1, m, 256) and d["descriptors1"].shape == (1, n, 256)


def test_early_stop_configs_stop_at_different_layers_with_margin():
    assert ar.DELTA == 1e-4
    for depth, width, pz in apr.CONFIGS[:2]:
        runs = apr.traced(depth, width, pz)
        stops = tuple(final["stop_layer"] for _, final, _ in runs)
        print(f"depth {depth}: stop layers {stops}")
        assert stops == STOP_LAYERS[depth], (depth, stops)
        for p, (layers, final, bands) in enumerate(runs):
            margins = [bd["ratio_margin"] for bd in bands if bd["ratio_margin"] is not None]
            print(f"depth {depth} pair {p}: min ratio margin {min(margins):.2f} points, band rows {_band_rows(bands)}")
            assert min(margins) >= MIN_MARGIN, (depth, p, margins)
            assert _band_rows(bands) <= MAX_BAND_ROWS, (depth, p, _band_rows(bands))
            # pruning is at work before the stop: the pair's rows shrink
            if len(layers) > 1:
                assert layers[-1]["m"] + layers[-1]["n"] < layers[0]["m"] + layers[0]["n"]


def test_prune_only_config_shrinks_every_pair_at_every_layer():
    depth, width, pz = apr.CONFIGS[2]
    runs = apr.traced(depth, width, pz)
    last = []
    for p, (layers, final, bands) in enumerate(runs):
        assert final["stop_layer"] == 9 and len(layers) == 9, (p, final["stop_layer"])
        rows = [r["m"] + r["n"] for r in layers]
        assert all(b < a for a, b in zip(rows, rows[1:])), (p, rows)
        assert layers[-1]["m"] > 0 and layers[-1]["n"] > 0
        # the oracle's own count on this trace: 8, 2, 2 and 3 band rows (pair 0 has more than the 6 of the stop traces);
        # pinned here so that the room the GPU test's band exit has under this configuration is fixed on the oracle
        print(f"prune only pair {p}: band rows {_band_rows(bands)} ({[bd['n_unsure'] for bd in bands]})")
        assert _band_rows(bands) <= MAX_BAND_ROWS_PRUNE_ONLY, (p, _band_rows(bands))
        last.append((layers[-1]["m"], layers[-1]["n"]))
    print("prune only: rows of the last layer", last)
    assert last[2] == (3, 5), last  # the smallest pair: down to a handful of rows
