"""`HomographyPairFeeder` and `Endopatches1800Pipeline` on a generated tree: 8 sources of 48 x 64 (H x W) PNG in two
sequences, patch 48 x 36, 3 x 3 levels = 72 pairs.

The feeder's images are held to the float64 warp restatement under its bound (tests/warp_reference.py: UNPINNED against
OpenCV, 7 * 2^-24 * max|tap| per pixel, a pixel left out only within 1e-7 of a rounding tie, at most 0.01 % of them);
`H_0to1` is the host value tests/test_endopatches_host.py checks against the reference's draws; a source costs ONE warp
call per batch; view 0 is one tensor for a source's nine items.  The pipeline writes `predictions.h5` and the HPatches
summary keys, and gives the same kind of result from the tree's saved form (8-bit images: counts and finiteness are
compared, not values)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endopatches_reference as er  # noqa: E402
import warp_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu
CONF = {"data_dir": "frames", "test_size": 72, "test_seed": 0, "test_sequences": ["Seq_003", "Seq_016"],
        "test_homography_levels": [0.3, 0.5, 0.7], "test_photometric_levels": [0.25, 0.6, 0.95], "test_source_dir": None,
        "photometric": {"name": "identity"}, "crop_vignette": False,
        "homography": {"difficulty": 0.7, "max_angle": 45, "patch_shape": [48, 36]}}


def _counted(feeder):
    calls = []
    inner = feeder.warp

    def warp(src, index, mats, size, **kw):
        calls.append((src.data_ptr(), int(index.numel())))
        return inner(src, index, mats, size, **kw)

    feeder.warp = warp
    return calls


def test_feeder_renders_the_schedule(tmp_path):
    from glue_factory_colon_amd import homographies as hg
    from glue_factory_colon_amd.image_io import read_image

    er.make_tree(tmp_path, per_sequence=4)
    ds = hg.HomographyPairs(CONF, tmp_path)
    assert len(ds) == 72
    feeder = ds.feeder(batch=36)
    calls = _counted(feeder)
    items = list(feeder)
    assert len(items) == 72 and len(calls) == 8  # 2 batches x 4 sources
    assert all(n == 10 for _, n in calls)         # view 0 once + nine variants
    planes = {}
    left_out = 0
    for i, (it, sched) in enumerate(zip(items, ds.items)):
        assert it["name"] == [sched["name"]] and it["scene"] == [sched["scene"]] and it["source_name"] == [sched["source_name"]]
        assert int(it["idx"]) == i
        geo = ds.geometry(i)
        assert it["H_0to1"].dtype == torch.float32 and np.array_equal(it["H_0to1"][0].numpy(), geo["H_0to1"])
        name = sched["source_name"]
        if name not in planes:
            planes[name] = wr.to_float(read_image(tmp_path / "frames" / "test" / name))
        for tag in ("view0", "view1"):
            v = it[tag]
            assert tuple(v["image"].shape) == (1, 3, 36, 48) and v["image"].is_cuda
            assert v["image_size"].tolist() == [[48.0, 36.0]] and v["scales"].tolist() == [[1.0, 1.0]]
            ref = wr.warp(planes[name], np.linalg.inv(geo[tag]["H"]), (36, 48))
            left_out += wr.check(v["image"][0].cpu().numpy(), ref, what=f"{sched['name']} {tag}")
        assert float(it["view1"]["image"].abs().max()) > 0.1
    assert left_out <= 1e-4 * 144 * 36 * 48, left_out
    # view 0 of a source: one tensor for its nine items, named as one image; view 1 never
    for s in range(8):
        group = items[9 * s: 9 * s + 9]
        assert len({g["view0"]["image"].data_ptr() for g in group}) == 1
        assert len({ds.view_key(g, 0) for g in group}) == 1 and all(ds.view_key(g, 1) is None for g in group)
        assert len({g["view1"]["image"].data_ptr() for g in group}) == 9
    assert len({ds.view_key(items[9 * s], 0) for s in range(8)}) == 8
    # a batch that cuts sources: every (source, batch) still costs one call -- 4 + 5 + 1
    feeder = ds.feeder(batch=32, num_workers=0)
    calls = _counted(feeder)
    again = list(feeder)
    assert [n for _, n in calls] == [10, 10, 10, 6, 5, 10, 10, 10, 2, 9]
    assert calls[3][0] == calls[4][0] and calls[8][0] == calls[9][0]  # a cut source stays where it was uploaded
    assert feeder.h2d_bytes == 8 * 48 * 64 * 3                       # every source travels once
    for a, b in zip(items, again):
        assert torch.equal(a["view0"]["image"], b["view0"]["image"]) and torch.equal(a["view1"]["image"], b["view1"]["image"])
    # this rank's share only, in groups of a source's nine items
    mine = list(ds.feeder(batch=36).shard(1, 2, group=9))
    assert [i for i, _ in mine] == [i for i in range(72) if (i // 9) % 2 == 1]
    assert all(torch.equal(it["view1"]["image"], items[i]["view1"]["image"]) for i, it in mine)
    # grayscale: the fp32 grey sum after the warp
    gray_ds = hg.HomographyPairs({**CONF, "grayscale": True}, tmp_path)
    first = next(iter(gray_ds.feeder(batch=9)))
    assert tuple(first["view1"]["image"].shape) == (1, 1, 36, 48)
    geo = ds.geometry(0)
    ref = wr.warp(planes[ds.items[0]["source_name"]], np.linalg.inv(geo["view1"]["H"]), (36, 48))
    assert wr.check(first["view1"]["image"][0].cpu().numpy(), ref, gray=True, what="gray view1") == 0


def test_pipeline_generated_and_saved(tmp_path):
    from glue_factory_colon_amd import eval_endopatches
    from glue_factory_colon_amd.export_predictions import load_predictions

    er.make_tree(tmp_path, per_sequence=4)
    pipe = eval_endopatches.Endopatches1800Pipeline(CONF, data_root=tmp_path, pair_batch=36)
    assert pipe.shard_group == 9 and len(pipe.dataset) == 72
    # Name-seeded weights, at most 256 key points.  A DLT estimate needs four matches (with fewer its error is +inf by
    # the reference's own rule, eval/utils.py:291-292), and random weights put little confidence on any: measured on
    # this tree with the evaluation's nms_radius 3 / filter_threshold 0.1, ~36 key points and 2-7 matches per pair.
    # So: nms_radius 1 (more key points in a 36 x 48 patch) and filter_threshold 0 (every mutual best assignment is a
    # match -- scores are exp(.) > 0 -- about half the key points of a random score matrix).
    from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline

    model = TwoViewPipeline({
        "extractor": {"name": "extractors.superpoint_open", "weights": "synthetic", "max_num_keypoints": 256,
                      "detection_threshold": 0.0, "nms_radius": 1},
        "matcher": {"name": "matchers.lightglue", "weights": "synthetic", "filter_threshold": 0.0,
                    "depth_confidence": -1, "width_confidence": -1}}).eval().cuda()
    summaries, results = pipe.run(tmp_path / "exp", model)
    assert (tmp_path / "exp" / "predictions.h5").exists() and len(load_predictions(tmp_path / "exp" / "predictions.h5")) == 72
    assert results["names"] == [it["name"] for it in pipe.dataset.items]
    keys = ("prec@1px", "prec@3px", "num_matches", "num_keypoints", "gt_match_recall@3px", "gt_match_precision@3px",
            "H_error_dlt")
    for key in keys:
        assert f"mean_{key}" in summaries and f"med_{key}" in summaries, key
    assert all(f"H_error_dlt@{th}px" in summaries for th in (1, 3, 5))
    # the saved form of the same tree (8-bit PNG of the GPU warps), read back through the file path
    root = pipe.dataset.save_dataset(tmp_path / "saved")
    saved = eval_endopatches.Endopatches1800Pipeline(
        {**CONF, "read_dataset_from_disk": True, "saved_dataset_dir": "saved", "photometric": {"name": "lg"}},
        data_root=tmp_path, pair_batch=36)
    assert root == tmp_path / "saved" and len(saved.dataset) == 72
    s_summaries, s_results = saved.run(tmp_path / "exp_saved", model)
    assert set(s_summaries) == set(summaries) and s_results["names"] == results["names"]
    for r, what in ((results, "generated"), (s_results, "saved")):
        print(what, "num_keypoints", r["num_keypoints"][:12], "num_matches", r["num_matches"][:12])
        print(what, "H_error_dlt", [round(float(v), 2) for v in r["H_error_dlt"][:12]])
        print(what, "pairs with a finite H_error_dlt:", int(np.isfinite(r["H_error_dlt"]).sum()), "of 72; fewest matches",
              min(r["num_matches"]))
    for r in (results, s_results):
        assert all(np.isfinite(r["num_keypoints"])) and min(r["num_keypoints"]) > 0
        assert all(np.isfinite(r["H_error_dlt"]))
    # the saved images are the generated ones quantised to 8 bits: the homographies are the same numbers
    for i in (0, 40, 71):
        assert torch.equal(saved.dataset.meta(i)["H_0to1"], pipe.dataset.meta(i)["H_0to1"])
