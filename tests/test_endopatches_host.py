"""Host side of the EndoPatches pair generator (glue_factory_colon_amd.homographies), no GPU:
  * the sampler against the REFERENCE's own draws (tests/golden/endopatches_homographies.npz, written by
    tests/golden/make_golden_endopatches.py): H and the warped corners to 1e-12 relative, H_0to1 equal as float32;
  * the test schedule on a generated tree (2 sequences x 2 sources x 3 x 3 levels, test_size 36) against the
    restatement of tests/endopatches_reference.py: names, seeds, order, the three ways of choosing sources, every
    ValueError;
  * save_dataset -> read_dataset_from_disk: the same item list, H bit for bit through "%.18e", images
    floor(clip(x * 255)) / 255;
  * the photometric key: `lg` raises when generating (the message names both ways out), and is not consulted when a saved
    benchmark is read."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endopatches_reference as er  # noqa: E402

from glue_factory_colon_amd import homographies as hg  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "endopatches_homographies.npz")
ENDO = {"patch_shape": [580, 426], "max_angle": 45, "translation": 1.0, "n_angles": 10, "min_convexity": 0.05}
CONF = {"data_dir": "frames", "test_size": 36, "test_seed": 3, "test_sequences": ["Seq_003", "Seq_016"],
        "test_homography_levels": [0.3, 0.5, 0.7], "test_photometric_levels": [0.25, 0.6, 0.95],
        "photometric": {"name": "identity"}, "homography": {"difficulty": 0.7, "max_angle": 45, "patch_shape": [48, 36]}}


def _close(a, b):
    return np.all(np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), 1.0))


def test_sampler_equals_the_references_draws():
    fx = np.load(GOLDEN)
    size = tuple(int(v) for v in fx["size"])
    assert [int(v) for v in fx["patch"]] == ENDO["patch_shape"]
    for li, level in enumerate(fx["levels"]):
        for s in (int(v) for v in fx["seeds"]):
            conf = {**ENDO, "difficulty": float(level)}
            H, full, corners, _ = hg.sample_homography_corners(size, **conf, rng=np.random.RandomState(s))
            assert H.dtype == np.float64 and _close(H, fx[f"H_{li}_{s}"]) and _close(corners, fx[f"corners_{li}_{s}"])
            v0 = hg.sample_view(size, {**ENDO, "difficulty": 0.0}, np.random.RandomState(2 * s))
            v1 = hg.sample_view(size, conf, np.random.RandomState(2 * s + 1))
            assert v0["coords"].dtype == np.float32 and v0["H_"].dtype == np.float32
            H01 = hg.compute_homography(v0["coords"], v1["coords"], [1, 1]).astype(np.float32)
            assert np.array_equal(H01, fx[f"H0to1_{li}_{s}"]), (li, s)
    # view 0 of a scheduled item: difficulty 0 multiplies every draw by zero -- the same H whatever the seed
    assert all(np.array_equal(fx["H_0_0"], fx[f"H_0_{s}"]) for s in fx["seeds"])
    rsize = tuple(int(v) for v in fx["rsize"])
    for s in (int(v) for v in fx["seeds"]):  # the dataset's own defaults (revisitop1m)
        H, _, corners, _ = hg.sample_homography_corners(rsize, **hg.HomographyPairs.default_conf["homography"],
                                                        rng=np.random.RandomState(s))
        assert _close(H, fx[f"rH_{s}"]) and _close(corners, fx[f"rcorners_{s}"])
    # numpy's global generator seeded with s is the stream of RandomState(s): what fork_rng(seed) gives the reference
    np.random.seed(4)
    H, _, _, _ = hg.sample_homography_corners(size, **{**ENDO, "difficulty": 0.5})
    assert _close(H, fx["H_2_4"])


def _as_tuples(ds):
    return [(it["name"], it["seed"], it["source_name"], it["scene"], it["homography_level"], it["photometric_level"])
            for it in ds.items]


def _raises_like(fn_module, fn_reference):
    with pytest.raises(ValueError) as want:
        fn_reference()
    with pytest.raises(ValueError) as got:
        fn_module()
    assert str(got.value) == str(want.value), (str(got.value), str(want.value))


def test_schedule_matches_the_restatement(tmp_path):
    names = er.make_tree(tmp_path, per_sequence=3)
    assert [hg.HomographyPairs._parse_test_sequence(n) for n in ("Seq_003_000001.png", "a/b_c_12.jpg", "plain.png", "x_1a.png")] \
        == [er.sequence_of(n) for n in ("Seq_003_000001.png", "a/b_c_12.jpg", "plain.png", "x_1a.png")] \
        == ["Seq_003", "b_c", None, None]
    # route 1: the per-sequence permutation under RandomState(test_seed + sequence index)
    ds = hg.HomographyPairs(CONF, tmp_path)
    want = er.schedule(names, CONF)
    assert len(ds) == 36 and _as_tuples(ds) == want
    assert [it["idx"] for it in ds.items] == list(range(36)) and ds.items[10]["name"].endswith("/h0_p1.png")
    assert ds.items[10]["homography_file"] == f"H_{ds.items[10]['source_dir']}_h0_p1.txt"
    assert ds.items[10]["homography_conf"] == {"difficulty": 0.3, "translation": 1.0, "max_angle": 45, "n_angles": 10,
                                               "patch_shape": [48, 36], "min_convexity": 0.05}
    assert len({w[2] for w in want}) == 4 and {w[3] for w in want} == {"Seq_003", "Seq_016"}
    assert _as_tuples(hg.HomographyPairs({**CONF, "test_seed": 4}, tmp_path)) == er.schedule(names, {**CONF, "test_seed": 4}) != want
    # the sequence filter: only the named sequences' frames are test images
    one = {**CONF, "test_sequences": ["Seq_016"], "test_size": 18}
    assert _as_tuples(hg.HomographyPairs(one, tmp_path)) == er.schedule([n for n in names if n.startswith("Seq_016")], one)
    # route 2: a list file (relative to the image tree, then to the data root)
    listed = [names[4], names[0], names[5], names[2]]
    (tmp_path / "frames" / "sources.txt").write_text("\n".join(listed) + "\n\n")
    by_list = {**CONF, "test_image_list": "sources.txt"}
    assert _as_tuples(hg.HomographyPairs(by_list, tmp_path)) == er.schedule(names, CONF, listed)
    # route 3: a directory <dir>/<sequence>/ of the sources' files, sequences in configuration order, names sorted
    for n in listed:
        d = tmp_path / "picked" / er.sequence_of(n)
        d.mkdir(parents=True, exist_ok=True)
        (d / n).write_bytes(b"")
    by_dir = {**CONF, "test_source_dir": "picked"}
    in_dir = sorted(n for n in listed if n.startswith("Seq_003")) + sorted(n for n in listed if n.startswith("Seq_016"))
    assert _as_tuples(hg.HomographyPairs(by_dir, tmp_path)) == er.schedule(names, CONF, in_dir)
    # every ValueError, with the restatement's text
    for bad in ({"test_size": 35}, {"test_size": 27}, {"test_size": 72}):
        _raises_like(lambda: hg.HomographyPairs({**CONF, **bad}, tmp_path), lambda: er.schedule(names, {**CONF, **bad}))
    for lines in (["Seq_003_000009.png", *listed[1:]], listed[:3], [listed[0], listed[0], *listed[2:]]):
        (tmp_path / "frames" / "bad.txt").write_text("\n".join(lines) + "\n")
        _raises_like(lambda: hg.HomographyPairs({**CONF, "test_image_list": "bad.txt"}, tmp_path),
                     lambda: er.schedule(names, CONF, lines, "bad.txt"))
    (tmp_path / "picked" / "Seq_003" / "Seq_003_000042.png").write_bytes(b"")
    _raises_like(lambda: hg.HomographyPairs(by_dir, tmp_path),
                 lambda: er.schedule(names, CONF, sorted([*in_dir[:2], "Seq_003_000042.png"]) + in_dir[2:], "picked"))
    with pytest.raises(ValueError, match="test_source_dir and read_dataset_from_disk are mutually exclusive"):
        hg.HomographyPairs({**by_dir, "read_dataset_from_disk": True}, tmp_path)
    with pytest.raises(FileNotFoundError):
        hg.HomographyPairs({**CONF, "test_source_dir": "nowhere"}, tmp_path)
    with pytest.raises(FileNotFoundError):
        hg.HomographyPairs({**CONF, "data_dir": "nowhere"}, tmp_path)
    for key in ({"triplet": True}, {"load_features": {"do": True}}):
        with pytest.raises(NotImplementedError):
            hg.HomographyPairs({**CONF, **key}, tmp_path)
    # without a schedule the test split is the list of frames, and the train split the train folder
    plain = hg.HomographyPairs({**CONF, "test_size": 0}, tmp_path)
    assert plain.items is None and plain.image_names == names and plain.view_key({"source_name": ["x"]}, 0) is None
    assert hg.HomographyPairs(CONF, tmp_path, split="train").image_names == ["Seq_000_000000.png"]
    from glue_factory_colon_amd.registry import get_dataset
    assert get_dataset("homographies") is hg.HomographyPairs


def test_scheduled_geometry_is_the_fixtures(tmp_path):
    """582 x 429 frames with the EndoPatches homography settings: item k of two sources x three levels x one photometric
    level has seed k and level k % 3, so its H_0to1 is the fixture's (views drawn under 2 k and 2 k + 1)."""
    fx = np.load(GOLDEN)
    er.make_tree(tmp_path, sequences=("Seq_003",), per_sequence=2, hw=(429, 582), flat=True)
    conf = {**CONF, "test_size": 6, "test_seed": 0, "test_sequences": ["Seq_003"], "test_photometric_levels": [0.5],
            "homography": {**ENDO, "difficulty": 0.7}}
    ds = hg.HomographyPairs(conf, tmp_path)
    for k in range(6):
        geo = ds.geometry(k)
        assert np.array_equal(geo["H_0to1"], fx[f"H0to1_{k % 3 + 1}_{k}"]), k
        assert _close(geo["view0"]["H"], fx["H_0_0"])
        meta = ds.meta(k)
        assert torch.equal(meta["H_0to1"], torch.from_numpy(fx[f"H0to1_{k % 3 + 1}_{k}"])) and meta["name"] == ds.items[k]["name"]
        assert meta["view0"]["image_size"].tolist() == [580.0, 426.0] and meta["view1"]["scales"].tolist() == [1.0, 1.0]
    # the vignette crop of a larger frame gives the same geometry: the window is the image
    er.make_tree(tmp_path, sequences=("Seq_003",), per_sequence=2, hw=(540, 720), flat=True, name="full")
    cropped = hg.HomographyPairs({**conf, "data_dir": "full", "crop_vignette": True, "vignette_crop_coords": [81, 663, 55, 484]},
                                 tmp_path)
    assert cropped.window(540, 720) == (81, 55, 582, 429)
    assert np.array_equal(cropped.geometry(4)["H_0to1"], fx["H0to1_2_4"])
    # reseed (no schedule): both views draw in turn from RandomState(conf.seed + idx)
    free = hg.HomographyPairs({**conf, "test_size": 0, "reseed": True, "seed": 7, "left_view_difficulty": 0.0}, tmp_path)
    rng = np.random.RandomState(7 + 1)
    v0 = hg.sample_view((582, 429), {**ENDO, "difficulty": 0.0}, rng)
    v1 = hg.sample_view((582, 429), {**ENDO, "difficulty": 0.7}, rng)
    assert np.array_equal(free.geometry(1)["H_0to1"], hg.compute_homography(v0["coords"], v1["coords"], [1, 1]).astype(np.float32))


def test_save_then_read_round_trip(tmp_path):
    er.make_tree(tmp_path, per_sequence=2)
    ds = hg.HomographyPairs(CONF, tmp_path)
    g = torch.Generator().manual_seed(0)
    view0 = {it["source_name"]: torch.rand((1, 3, 36, 48), generator=g) * 1.2 - 0.1 for it in ds.items}  # some < 0, some > 1
    pairs = [{"view0": {"image": view0[it["source_name"]]}, "view1": {"image": torch.rand((1, 3, 36, 48), generator=g) * 1.2 - 0.1},
              "H_0to1": torch.from_numpy(ds.geometry(i)["H_0to1"])[None]} for i, it in enumerate(ds.items)]
    root = ds.save_dataset(tmp_path / "saved", pairs)
    assert (root / "source_names.txt").read_text().splitlines() == list(dict.fromkeys(it["source_name"] for it in ds.items))
    first = (root / ds.items[0]["source_dir"] / "attribs.txt").read_text().splitlines()
    assert len(first) == 10 and first[0] == f"source.png {ds.items[0]['source_name']} Seq_003 source -1 0.000000 -1 0.000000"
    assert first[2] == f"h0_p1.png {ds.items[0]['source_name']} Seq_003 variant 0 0.300000 1 0.600000"
    # read back; `lg` is not consulted, and the photometric key of the generated run is not needed either
    saved = hg.HomographyPairs({**CONF, "photometric": {"name": "lg"}, "read_dataset_from_disk": True,
                                "saved_dataset_dir": "saved"}, tmp_path)
    assert len(saved) == len(ds) == 36
    for a, b in zip(ds.items, saved.items):
        assert {k: a[k] for k in b} == b  # every key of a saved item, with the generated item's value
    assert sorted(saved.items[0]) == sorted(["idx", "name", "scene", "source_name", "source_dir", "variant_name",
                                             "homography_file", "homography_idx", "homography_level", "photometric_idx",
                                             "photometric_level"])
    for i in (0, 7, 35):
        raw, meta = saved[i], saved.meta(i)
        H = ds.geometry(i)["H_0to1"]
        assert raw["H_0to1"].dtype == torch.float32 and np.array_equal(raw["H_0to1"][0].numpy(), H)
        assert np.array_equal(meta["H_0to1"].numpy(), H) and meta["name"] == ds.items[i]["name"] == raw["name"]
        assert meta["view0"]["image_size"].tolist() == [48.0, 36.0]
        for tag, x in (("view0", view0[ds.items[i]["source_name"]]), ("view1", pairs[i]["view1"]["image"])):
            want = np.floor(np.clip(x[0].numpy() * 255.0, 0, 255)).astype(np.uint8).transpose(1, 2, 0)
            assert raw[tag]["image"].dtype == torch.uint8 and np.array_equal(raw[tag]["image"].numpy(), want)
            assert want.min() == 0 and want.max() == 255
    assert saved.view_key(saved[3], 0) == saved.view_key(saved[5], 0) != saved.view_key(saved[9], 0)
    assert saved.view_key(saved[3], 1) is None
    with pytest.raises(ValueError):
        saved.geometry(0)
    with pytest.raises(FileNotFoundError, match="source_names.txt"):
        hg.HomographyPairs({**CONF, "read_dataset_from_disk": True, "saved_dataset_dir": "missing"}, tmp_path)
    # generating with `lg` (or `dark`, the dataset's default) is refused, naming both ways out
    for conf in ({**CONF, "photometric": {"name": "lg"}}, {k: v for k, v in CONF.items() if k != "photometric"}):
        with pytest.raises(NotImplementedError) as e:
            hg.HomographyPairs(conf, tmp_path)
        assert "photometric.name: identity" in str(e.value) and "read_dataset_from_disk" in str(e.value)


def test_pipeline_defaults_are_the_references():
    from glue_factory_colon_amd import eval_endopatches as ee
    from glue_factory_colon_amd.eval_hpatches import HPatchesPipeline

    assert issubclass(ee.Endopatches1800Pipeline, HPatchesPipeline)
    d = ee.Endopatches1800Pipeline.default_data_conf
    assert d["test_size"] == 1800 and d["test_sequences"] == ["Seq_003", "Seq_016"] and d["photometric"] == {"name": "lg"}
    assert d["vignette_crop_coords"] == [81, 663, 55, 484] and d["homography"] == {"difficulty": 0.7, "max_angle": 45,
                                                                                  "patch_shape": [580, 426]}
    assert d["test_homography_levels"] == [0.3, 0.5, 0.7] and d["test_photometric_levels"] == [0.25, 0.6, 0.95]
    for name in ("get_predictions", "run_eval", "run", "_robust_conf"):
        assert getattr(ee.Endopatches1800Pipeline, name) is getattr(HPatchesPipeline, name)
    assert HPatchesPipeline.shard_group == 5


def test_image_dir_lists_without_split_folders(tmp_path):
    """No train/ and val/ folders: `image_dir` + glob / list file / list, shuffled with `shuffle_seed`, then cut into
    train and val (homographies.py:143-176); the test split is empty."""
    from PIL import Image

    folder = tmp_path / "flat" / "jpg" / "sub"
    folder.mkdir(parents=True)
    names = sorted(f"sub/im_{k}.png" for k in range(5))
    for n in names:
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "flat" / "jpg" / n)
    base = {"data_dir": "flat", "image_dir": "jpg/", "train_size": 3, "val_size": 2, "photometric": {"name": "identity"}}
    want = list(names)
    np.random.RandomState(0).shuffle(want)
    by_glob = hg.HomographyPairs({**base, "image_list": None}, tmp_path, split="train")
    assert by_glob.image_names == want[:3] and by_glob.images["val"] == want[3:5] and by_glob.images["test"] == []
    assert by_glob.items is None and len(by_glob) == 3 and by_glob.image_dir == tmp_path / "flat" / "jpg"
    listed = [names[3], names[1], names[4]]
    (tmp_path / "flat" / "list.txt").write_text("\n".join(listed) + "\n")
    want = list(listed)
    np.random.RandomState(5).shuffle(want)
    by_file = hg.HomographyPairs({**base, "image_list": "list.txt", "shuffle_seed": 5, "check_file_exists": True}, tmp_path, "val")
    assert by_file.images["train"] == want and by_file.image_names == []
    assert hg.HomographyPairs({**base, "image_list": listed, "shuffle_seed": None}, tmp_path, "train").image_names == listed
    meta = by_glob.meta(0)  # unseeded pairs draw from numpy's global generator
    assert meta["name"] == by_glob.image_names[0] and meta["scene"] == "" and tuple(meta["H_0to1"].shape) == (3, 3)
    with pytest.raises(FileNotFoundError, match="Cannot find image list"):
        hg.HomographyPairs({**base, "image_list": "nolist.txt"}, tmp_path)
    with pytest.raises(FileNotFoundError):
        hg.HomographyPairs({**base, "image_list": ["sub/none.png"], "check_file_exists": True}, tmp_path)
    with pytest.raises(ValueError, match="Cannot find any image in folder"):
        hg.HomographyPairs({**base, "image_list": None, "glob": ["*.jpg"]}, tmp_path)
    with pytest.raises(ValueError):
        hg.HomographyPairs({**base, "image_list": 7}, tmp_path)
