"""CPU checks of the Endomapper reader against the reference's own dataset class (tests/golden/endomapper_items.npz, made
by gluefactory.datasets.endomapper._PairDataset on the tree of tests/endomapper_reference.py), and of the overlap-bin
arithmetic of `validate`."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endomapper_reference as er  # noqa: E402

from glue_factory_colon_amd import registry, validate  # noqa: E402
from glue_factory_colon_amd.endomapper import CACHE_KEYS, Endomapper  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "endomapper_items.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("endomapper")
    er.write_tree(tmp)
    return tmp


@pytest.mark.parametrize("name", list(er.CONFS))
def test_items_equal_the_references(z, tree, name):
    assert registry.get_dataset("endomapper") is Endomapper
    ds = Endomapper(er.CONFS[name], tree, "val")
    assert ds.seqs_maps == ["Seq_001_map0", "Seq_001_map1"]  # Seq_002_map0 has 5 images, Seq_003 no map
    assert len(ds) == len(z[f"{name}_seq_map"]) == {"all": 155, "ten": 20, "pairs": 3}[name]
    assert [it[0] for it in ds.items] == list(z[f"{name}_seq_map"])
    assert [str(it[1]) for it in ds.items] == list(z[f"{name}_name0"])
    assert [str(it[2]) for it in ds.items] == list(z[f"{name}_name1"])
    assert np.array_equal(np.array([it[3] for it in ds.items], dtype=np.float32), z[f"{name}_overlap"])
    if name == "ten":  # the top bin (0.767, 1.0] holds four pairs, fewer than 2 x 3: the other two bins give five each
        assert max(it[3] for it in ds.items) <= 0.3 + 2 * 0.7 / 3 and sorted({it[0] for it in ds.items}) == ds.seqs_maps
    ds_sorted = Endomapper({**er.CONFS[name], "sort_by_overlap": True}, tree, "val")
    overlaps = [it[3] for it in ds_sorted.items]
    assert overlaps == sorted(overlaps, reverse=True) and sorted(map(str, ds_sorted.items)) == sorted(map(str, ds.items))


def test_views_equal_the_references(z, tree):
    ds = Endomapper(er.CONFS["all"], tree, "val")
    seen = {"truncated_valid": False, "truncated_mixed": False, "padded": False, "full": False}
    for i in z["view_items"]:
        item = ds[int(i)]
        assert item["idx"] == int(i) and item["names"] == str(z[f"item{i}_names"])
        assert np.float32(item["overlap_0to1"]) == z[f"item{i}_overlap"]
        assert np.array_equal(item["T_0to1"]._data.numpy(), z[f"item{i}_T_0to1"])
        assert np.array_equal(item["T_1to0"]._data.numpy(), z[f"item{i}_T_1to0"])
        for v in ("view0", "view1"):
            view = item[v]
            assert set(view["cache"]) == set(CACHE_KEYS) and "image" not in view
            for k, t in view["cache"].items():
                want = z[f"item{i}_{v}_{k}"]
                assert t.shape[0] == er.LIMIT and t.numpy().dtype == want.dtype, (i, v, k)
                assert np.array_equal(t.numpy(), want), (i, v, k)  # the pads too: the same generator stream
            assert np.array_equal(view["camera"]._data.numpy(), z[f"item{i}_{v}_camera"])
            assert view["camera"].model == "OPENCV_FISHEYE" and view["camera"]._data.dtype == torch.float32
            assert np.array_equal(view["T_w2cam"]._data.numpy(), z[f"item{i}_{v}_T_w2cam"])
            assert np.array_equal(view["image_size"].numpy(), z[f"item{i}_{v}_image_size"])
            assert view["name"] == str(z[f"item{i}_{v}_name"])
            n_valid = int(view["cache"]["valid_3D_mask"].sum())
            pads = int((view["cache"]["point3D_ids"] == -1).sum() - (~view["cache"]["valid_3D_mask"]).sum())
            if view["name"] == "000000" and view["seq_map"] == "Seq_001_map0":
                seen["truncated_valid"] = n_valid == er.LIMIT
            elif view["name"] == "000001" and view["seq_map"] == "Seq_001_map0":
                seen["truncated_mixed"] = n_valid == 30
            elif view["seq_map"] == "Seq_001_map1":
                seen["full"] = True
            else:
                seen["padded"] = bool((view["cache"]["sparse_depth"][-1] == -1) and not view["cache"]["valid_depth_mask"][-1])
            assert pads == 0  # every id of -1 is an invalid 3D point (generated or padded)
    assert all(seen.values()), seen
    again = ds[int(z["view_items"][0])]  # seeded per item: the same pads again
    assert torch.equal(again["view1"]["cache"]["descriptors"], torch.from_numpy(z[f"item{z['view_items'][0]}_view1_descriptors"]))


def test_refusals_and_the_key_frame_fallback(tree):
    with pytest.raises(NotImplementedError, match="Triplet"):
        Endomapper({**er.BASE_CONF, "views": 3}, tree)
    with pytest.raises(NotImplementedError, match="views: 1"):
        Endomapper({**er.BASE_CONF, "views": 1}, tree)
    with pytest.raises(NotImplementedError, match="num_neg"):
        Endomapper({**er.BASE_CONF, "val_num_per_scene": [10, 2]}, tree)
    with pytest.raises(FileExistsError):
        Endomapper({**er.BASE_CONF, "data_dir": "missing"}, tree)
    with pytest.raises(ValueError, match="No Endomapper sequences"):
        Endomapper({**er.BASE_CONF, "val_split": ["Seq_002"]}, tree)
    ds = Endomapper({**er.BASE_CONF, "val_split": ["Seq_001"], "read_image": True, "grayscale": True}, tree)
    view = ds[0]["view0"]
    assert view["name"].startswith("Keyframe_") and view["image"].shape == (1, er.H, er.W) and not view["image"].any()
    assert Endomapper.default_conf["max_num_features"] == 2048 and Endomapper.default_conf["seq_lists_dir"] is None


def test_overlap_bins_arithmetic():
    bins = validate.overlap_bins("0:0.2,0.2:0.4,0.4:1.0")
    assert [b[2] for b in bins] == ["overlap_0.00_0.20", "overlap_0.20_0.40", "overlap_0.40_1.00", "overlap_0.00_1.00"]
    assert validate.overlap_bins([[0.0, 1.0], [0.0, 0.5]])[-1] == (0.0, 0.5, "overlap_0.00_0.50")  # overall already there
    assert validate.overlap_bins(None) is None and validate.overlap_bins("") is None
    with pytest.raises(ValueError, match="pairs"):
        validate.overlap_bins([[0.1, 0.2, 0.3]])
    overlaps = [0.0, 0.2, 0.39, 0.4, float("nan"), 1.0]
    rows = [{"a": float(i), "b": float("nan") if i == 2 else 1.0} for i in range(6)]
    out = validate.bin_results(validate.overlap_bins("0:0.2,0.2:0.4,0.4:1.0,1.5:2.0"), overlaps, rows)
    assert set(out) == {"overlap_0.00_0.20", "overlap_0.20_0.40", "overlap_0.40_1.00", "overlap_0.00_2.00"}  # empty bin left out
    assert out["overlap_0.00_0.20"] == {"a": 0.0, "b": 1.0}            # low <= overlap < high
    assert out["overlap_0.20_0.40"]["a"] == 1.5 and out["overlap_0.20_0.40"]["b"] == 1.0  # NaN values left out
    assert out["overlap_0.40_1.00"]["a"] == 3.0                        # 1.0 itself is outside [0.4, 1.0)
    assert out["overlap_0.00_2.00"]["a"] == (0 + 1 + 2 + 3 + 5) / 5 and not math.isnan(out["overlap_0.00_2.00"]["b"])
