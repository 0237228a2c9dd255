"""`posed_images.PosedPairFeeder` and `PosePairsPipeline.run` on a generated dataset directory against the restatement
of the reference's reader (tests/posed_reference.py), in two configurations under one data root:
(a) scene `endomapper_dense1500`: 540x720 files, the Endomapper-dense crop, per-image depth scales, packed specular masks,
    no resize, 3 images / 2 pairs -- every pixel operation is a copy or one fp32 product, so every tensor is exact;
(b) scene `megadepth1500`: 240x320 files, no crop, `preprocessing = {resize: 160, side: long}`, 3 pairs -- the image goes
    through the antialiased bilinear resize (5e-7, the bound of tests/test_preprocess.py) and the depth through
    blur-then-nearest (5e-7 * max)."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posed_reference as pr  # noqa: E402

from glue_factory_colon_amd import eval_pose_pairs, posed_images  # noqa: E402
from glue_factory_colon_amd.eval_hpatches import build_model  # noqa: E402
from glue_factory_colon_amd.export_predictions import load_predictions  # noqa: E402

pytestmark = pytest.mark.gpu
TENSOR_KEYS = ("image", "depth", "valid_depth", "specular_mask", "scales", "image_size", "original_image_size", "transform")


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("posed")
    pr.write_dataset(root, "endomapper_dense1500", (540, 720), 3, [(0, 1), (2, 1)], model="OPENCV_FISHEYE",
                     with_scene_info=True, seed=1)
    pr.write_dataset(root, "megadepth1500", (240, 320), 3, [(0, 1), (1, 2), (0, 2)], model="PINHOLE", seed=2)
    return root


@pytest.fixture(scope="module")
def restated(data_root):
    return {"a": pr.read_items(data_root, pr.CONF_A), "b": pr.read_items(data_root, pr.CONF_B)}


def _check_geometry_and_names(item, ref):
    assert item["name"] == [ref["name"]] and item["query_name"] == [ref["query_name"]] and item["scene"] == [ref["scene"]]
    assert item["references"] == [[r] for r in ref["references"]] and int(item["nviews"][0]) == ref["nviews"] == 2
    T = item["T_0to1"]
    assert tuple(T._data.shape) == (1, 12)
    assert float((T.R[0] - ref["T_0to1"][0]).abs().max()) <= 1e-6 and float((T.t[0] - ref["T_0to1"][1]).abs().max()) <= 1e-6
    for v in ("view0", "view1"):
        got, want = item[v], ref[v]
        assert got["name"] == [want["name"]] and got["camera"].model == want["model"]
        cam = got["camera"]._data
        assert tuple(cam.shape) == (1, want["camera"].shape[0])
        assert float((cam[0] - want["camera"]).abs().max()) <= 1e-6 * float(want["camera"].abs().max())
        assert float((got["T_w2cam"].R[0] - want["R"]).abs().max()) <= 1e-6
        assert float((got["T_w2cam"].t[0] - want["t"]).abs().max()) <= 1e-6


def test_feeder_crop_scale_masks_exact(data_root, restated):
    ds = posed_images.PosedImages(pr.CONF_A, data_root)
    items = list(posed_images.PosedPairFeeder(ds, "cuda"))
    assert len(items) == len(ds) == len(restated["a"]) == 2
    for item, ref in zip(items, restated["a"]):
        _check_geometry_and_names(item, ref)
        for v in ("view0", "view1"):
            for key in TENSOR_KEYS:
                got, want = item[v][key], ref[v][key]
                assert got.shape[0] == 1 and got.dtype == want.dtype, (key, got.dtype, want.dtype)
                assert torch.equal(got[0].cpu(), want), (v, key)
            assert tuple(item[v]["image"].shape) == (1, 3, 512, 672) and item[v]["specular_mask"].dtype == torch.bool
            assert item[v]["image"].is_cuda and item[v]["depth"].is_cuda and item[v]["scales"].is_cuda
            assert 0 < int(item[v]["specular_mask"].sum()) < 512 * 672 and 0 < int(item[v]["valid_depth"].sum()) < 512 * 672
    # a depth map that has neither the raw nor the cropped image's shape: the reference's error
    import numpy as np
    bad = data_root / "endomapper_dense1500" / "depths" / "seq_000" / "img0.npz"
    keep = bad.read_bytes()
    try:
        np.savez(bad, depth=np.ones((500, 700), np.float32))
        with pytest.raises(ValueError, match=r"Depth shape mismatch for .*img0.npz: \(500, 700\) vs image \(512, 672\)"):
            next(iter(posed_images.PosedPairFeeder(ds, "cuda")))
    finally:
        bad.write_bytes(keep)


def test_feeder_resized(data_root, restated):
    ds = posed_images.PosedImages(pr.CONF_B, data_root)
    feeder = posed_images.PosedPairFeeder(ds, "cuda")
    items = list(feeder)
    assert len(items) == 3
    for item, ref in zip(items, restated["b"]):
        _check_geometry_and_names(item, ref)
        for v in ("view0", "view1"):
            got, want = item[v], ref[v]
            assert tuple(got["image"].shape) == (1, 3, 120, 160) and tuple(got["depth"].shape) == (1, 120, 160)
            assert float((got["image"][0].cpu() - want["image"]).abs().max()) <= 5e-7
            d = want["depth"]
            assert float((got["depth"][0].cpu() - d).abs().max()) <= 5e-7 * float(d.max())
            # the input's depth is >= 0.5 or exactly 0 in blocks wider than the blur: no pixel of the restatement is
            # within 1e-5 of 0 without being 0, so the comparison of valid_depth leaves none out
            sure = (d.abs() > 1e-5) | (d == 0)
            assert bool(sure.all()) and 0 < int((d == 0).sum()) < d.numel()
            assert torch.equal(got["valid_depth"][0].cpu()[sure], want["valid_depth"][sure])
            for key in ("scales", "image_size", "original_image_size", "transform"):
                assert torch.equal(got[key][0].cpu(), want[key]), key
    # a rank's share: its indices and its items
    shard = list(feeder.shard(1, 2))
    assert [i for i, _ in shard] == [1] and shard[0][1]["name"] == items[1]["name"]


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_run_and_command_line(data_root, restated, tmp_path):
    ds = posed_images.PosedImages(pr.CONF_B, data_root)
    model = build_model("synthetic", "synthetic", official=False, max_num_keypoints=256).to("cuda")
    pipe = eval_pose_pairs.PosePairsPipeline(eval_conf={"estimator": "gfc_amd", "ransac_th": 1.0}, pair_batch=2)
    summaries, results = pipe.run(tmp_path / "exp", model, posed_images.PosedPairFeeder(ds, "cuda"))
    pred_file = tmp_path / "exp" / "predictions.h5"
    names = [it["name"] for it in restated["b"]]
    assert set(load_predictions(pred_file)) == set(names) and len(names) == 3 and results["names"] == names
    assert "rel_pose_error_mAA" in summaries and "mean_num_matches" in summaries and "mean_epi_prec@1e-3" in summaries
    assert json.loads((tmp_path / "exp" / "summaries.json").read_text()).keys() == summaries.keys()
    ref_summaries, _ = pipe.run_eval(pr.eval_items(restated["b"]), pred_file)
    assert ref_summaries.keys() == summaries.keys()
    for key in summaries:
        assert _same(summaries[key], ref_summaries[key]), (key, summaries[key], ref_summaries[key])
    # the command line, on the same data directory (the benchmark whose files are npz: the Endomapper-dense scene)
    out = tmp_path / "cli"
    assert eval_pose_pairs.main(["--data_dir", str(data_root), "--benchmark", "endomapper_dense1500", "--experiment_dir",
                                 str(out), "--open", "--max_num_keypoints", "256", "--estimator", "gfc_amd",
                                 "--pair_batch", "2"]) == 0
    cli = json.loads((out / "summaries.json").read_text())
    assert "rel_pose_error_mAA" in cli and len(load_predictions(out / "predictions.h5")) == 2
    with pytest.raises(NotImplementedError, match="image_pairs"):
        eval_pose_pairs.main(["--data_dir", str(data_root), "--benchmark", "scannet1500"])
