"""The posed-image reader on the host (glue_factory_colon_amd/posed_images.py, no GPU): parsing, lists, file
loaders, the Endomapper-dense crop geometry, and one check of the checker -- that the `nearest` shapes of the GPU test
(tests/test_gpu_resample.py) tell torch's legacy rule from the two rules a kernel could mistake for it."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posed_reference as pr  # noqa: E402

from glue_factory_colon_amd import geometry, posed_images  # noqa: E402
from glue_factory_colon_amd.image_preprocessor import ImagePreprocessor, endomapper_dense_window  # noqa: E402

R9 = "0 -1 0 1 0 0 0 0 1".split()


def test_parse_pose_camera_models():
    pose, cam = posed_images.parse_pose_camera([*R9, "0.5", "-1", "2", "PINHOLE", "640", "480", "500", "510", "320", "240"])
    assert isinstance(pose, geometry.Pose) and isinstance(cam, geometry.Camera)
    assert pose._data.dtype == torch.float32 and cam._data.dtype == torch.float32
    assert torch.equal(pose.R, torch.tensor([[0., -1, 0], [1, 0, 0], [0, 0, 1]])) and pose.t.tolist() == [0.5, -1, 2]
    assert cam._data.tolist() == [640, 480, 500, 510, 320, 240] and cam.model == "PINHOLE"
    _, cam = posed_images.parse_pose_camera([*R9, "0", "0", "0", "SIMPLE_RADIAL", "640", "480", "500", "320", "240", "0.25"])
    assert cam._data.tolist() == [640, 480, 500, 500, 320, 240, 0.25, 0] and geometry.model_id(cam) == geometry.GFC_CAM_RADIAL
    _, cam = posed_images.parse_pose_camera([*R9, "0", "0", "0", "OPENCV_FISHEYE", "720", "540", "300", "301", "360", "270",
                                             "0.5", "0.25", "0.125", "0.0625"])
    assert cam._data.tolist() == [720, 540, 300, 301, 360, 270, 0.5, 0.25, 0.125, 0.0625]
    assert cam.model == "OPENCV_FISHEYE" and geometry.model_id(cam) == geometry.GFC_CAM_OPENCV_FISHEYE


def test_lists_names_poses_and_extra_keys(tmp_path):
    names = pr.write_dataset(tmp_path, "megadepth1500", (24, 32), 3, [(0, 1), (1, 2), (0, 2)], model="SIMPLE_RADIAL")
    (tmp_path / "megadepth1500" / "extra.txt").write_text("# name overlap tag\n" + "".join(
        f"{n} {0.25 * i} 'tag{i}'\n" for i, n in enumerate(names)))
    conf = {**pr.CONF_B, "extra_data": "{scene}/extra.txt", "extra_keys": ["overlap", "tag"]}
    ds = posed_images.PosedImages(conf, tmp_path)
    assert len(ds) == 3 and ds.items[1] == ["megadepth1500", names[1], names[2]]
    assert set(posed_images.DEFAULT_CONF) <= set(ds.conf) and ds.conf["preprocessing"]["resize"] == 160
    raw = ds.raw_item(2)
    assert raw["names"] == [names[0], names[2]] and raw["scene"] == "megadepth1500"
    v = raw["views"][1]
    assert v["image"].dtype == np.uint8 and v["image"].shape == (24, 32, 3)
    assert v["depth"].dtype == np.float32 and v["depth"].shape == (24, 32) and v["depth_scale"] is None
    assert v["extra"] == {"overlap": 0.5, "tag": "tag2"} and v["specular_mask_packed"] is None
    assert posed_images.names_to_pair(names[0], names[2]) == "seq_000-img0.png/seq_000-img2.png"
    ref = pr.read_items(tmp_path, pr.CONF_B)[2]
    T = raw["views"][1]["T_w2cam"] @ raw["views"][0]["T_w2cam"].inv()
    assert float((T.R - ref["T_0to1"][0]).abs().max()) <= 1e-6 and float((T.t - ref["T_0to1"][1]).abs().max()) <= 1e-6
    assert ref["name"] == "seq_000-img0.png/seq_000-img2.png"
    # scene_list: a file, and the directory listing
    (tmp_path / "scenes.txt").write_text("megadepth1500\n")
    assert posed_images.PosedImages({**pr.CONF_B, "scene_list": "scenes.txt"}, tmp_path).scenes == ["megadepth1500"]
    # views without groups: one item per image
    assert len(posed_images.PosedImages({**pr.CONF_B, "view_groups": None}, tmp_path)) == 3


def test_missing_file_asserts(tmp_path):
    names = pr.write_dataset(tmp_path, "megadepth1500", (24, 32), 2, [(0, 1)])
    depth = tmp_path / "megadepth1500" / "depths" / "seq_000" / "img1.npz"
    depth.unlink()
    with pytest.raises(AssertionError, match="img1.npz"):
        posed_images.PosedImages(pr.CONF_B, tmp_path)
    posed_images.PosedImages({**pr.CONF_B, "depth_dir": None}, tmp_path)  # depth is optional
    (tmp_path / "megadepth1500" / "images" / names[0]).unlink()
    with pytest.raises(AssertionError, match="img0.png"):
        posed_images.PosedImages({**pr.CONF_B, "depth_dir": None}, tmp_path)
    with pytest.raises(AssertionError):
        posed_images.PosedImages(pr.CONF_B, tmp_path / "nowhere")
    pr.write_dataset(tmp_path / "second", "megadepth1500", (24, 32), 2, [(0, 1)])
    with pytest.raises(ValueError, match="specular_scene_info_dir"):
        posed_images.PosedImages({**pr.CONF_B, "read_specular_mask": True}, tmp_path / "second")


def test_load_depth_masking_and_errors(tmp_path):
    depth = np.arange(12, dtype=np.float64).reshape(3, 4) + 1
    mask = np.zeros((3, 4), np.uint8)
    mask[1] = 1
    np.savez(tmp_path / "d.npz", depth=depth, mask=mask)
    out = posed_images.load_depth(tmp_path / "d.npz", "npz")
    assert out.dtype == np.float32 and np.array_equal(out, np.where(mask.astype(bool), depth, 0).astype(np.float32))
    np.savez(tmp_path / "plain.npz", depth=depth)
    assert np.array_equal(posed_images.load_depth(tmp_path / "plain.npz", "npz"), depth.astype(np.float32))
    np.savez(tmp_path / "bad.npz", depth=depth, mask=mask[:2])
    with pytest.raises(ValueError, match="Depth/mask shape mismatch"):
        posed_images.load_depth(tmp_path / "bad.npz", "npz")
    with pytest.raises(ValueError):
        posed_images.load_depth(tmp_path / "d.npz", "exr")
    from PIL import Image
    d16 = (np.arange(12, dtype=np.uint16).reshape(3, 4) * 5000)
    Image.fromarray(d16).save(tmp_path / "d.png")
    assert np.array_equal(posed_images.load_depth(tmp_path / "d.png", "png"), d16.astype(np.float32) / 256)
    from glue_factory_colon_amd import _hdf5
    if _hdf5.available():
        _hdf5.write_records(tmp_path / "g.h5", {"g": {"depth": depth.astype(np.float32)}})
        assert np.array_equal(_hdf5.read_dataset(tmp_path / "g.h5", "/g/depth"), depth.astype(np.float32))


def test_packed_mask_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    mask = rng.random((61, 53)) > 0.5  # 3233 bits: the last byte is partial, rows are not byte-aligned
    np.savez(tmp_path / "m.npz", mask_packbits=np.packbits(mask.reshape(-1)), mask_shape=np.array([61, 53]))
    packed, hw = posed_images.load_specular_mask(tmp_path / "m.npz")
    assert hw == (61, 53) and packed.dtype == np.uint8 and packed.shape == ((61 * 53 + 7) // 8,)
    assert torch.equal(pr.unpack(packed, hw), torch.from_numpy(mask))
    k = np.arange(61 * 53)  # the bit rule the kernel implements
    assert np.array_equal(((packed[k >> 3] >> (7 - (k & 7))) & 1).reshape(hw).astype(bool), mask)
    np.savez(tmp_path / "nomask.npz", mask_shape=np.array([61, 53]))
    with pytest.raises(KeyError, match="Specular mask array not found"):
        posed_images.load_specular_mask(tmp_path / "nomask.npz")


def test_crop_endomapper_dense_geometry():
    pre = ImagePreprocessor({})
    x = torch.arange(540 * 720, dtype=torch.float32).reshape(1, 540, 720)
    out, off = pre.crop_endomapper_dense(x)
    assert off == (36.0, 14.0) and tuple(out.shape) == (1, 512, 672)
    assert torch.equal(out, x[..., 0:540, 35:710][..., 14:526, 1:673])
    assert endomapper_dense_window(540, 720) == (36, 14, 672, 512) == pr.endomapper_window(540, 720)
    y = torch.zeros(3, 512, 672)
    same, off = pre.crop_endomapper_dense(y)
    assert same is y and off == (0.0, 0.0) and endomapper_dense_window(512, 672) == (0, 0, 672, 512)
    for hw in ((539, 720), (540, 709)):
        with pytest.raises(ValueError, match="Image too small for Endomapper dense crop"):
            pre.crop_endomapper_dense(torch.zeros(1, *hw))
        with pytest.raises(ValueError, match="Image too small for Endomapper dense crop"):
            endomapper_dense_window(*hw)
    cam = geometry.Camera(torch.tensor([720., 540, 300, 301, 360, 270]))
    cropped = cam.crop(off if False else (36.0, 14.0), (672, 512))
    assert cropped._data.tolist() == [672, 512, 300, 301, 324, 256]


def test_scene_info_and_prefix_stripping(tmp_path):
    names = pr.write_dataset(tmp_path, "endomapper_dense1500", (24, 32), 3, [(0, 1)], model="OPENCV_FISHEYE",
                             with_scene_info=True)
    ds = posed_images.PosedImages({**pr.CONF_A, "crop_endomapper_dense": False}, tmp_path)
    root = tmp_path / "endomapper_dense1500"
    # the first path is stored as endomapper_dense/masks/..., the others as masks/...: both land under <root>/<scene>/masks
    assert [ds.specular_masks[n] for n in names] == [root / "masks" / "seq_000" / f"img{i}.npz" for i in range(3)]
    assert [ds.depth_scales[n] for n in names] == [float(np.float32(0.37 + 0.11 * i)) for i in range(3)]
    v = ds.raw_item(0)["views"][1]
    assert v["depth_scale"] == float(np.float32(0.48)) and v["specular_mask_shape"] == (24, 32)
    with np.load(root / "masks" / "seq_000" / "img1.npz") as z:
        assert np.array_equal(v["specular_mask_packed"], z["mask_packbits"])
    assert v["camera"].model == "OPENCV_FISHEYE"


def test_nearest_shapes_discriminate_the_rules():
    """torch's `nearest` is floor(dst * scale) with scale in fp32.  At the shapes of the GPU test the formula restated
    here reproduces F.interpolate exactly, and both `nearest-exact` and the float64 evaluation differ from it somewhere:
    a kernel built on either cannot pass."""
    differs = {"exact": 0, "f64": 0}
    for (h, w), (oh, ow), crop in pr.SHAPES:
        _, _, cw, ch = pr.window((h, w), crop)
        src = torch.arange(ch * cw, dtype=torch.float32).reshape(1, 1, ch, cw)
        got = F.interpolate(src, size=(oh, ow), mode="nearest")[0, 0].long()
        iy, ix = pr.nearest_index(ch, oh, "legacy"), pr.nearest_index(cw, ow, "legacy")
        assert torch.equal(got, torch.from_numpy(iy[:, None] * cw + ix[None, :]))
        for rule in differs:
            differs[rule] += int((pr.nearest_index(ch, oh, rule) != iy).sum() + (pr.nearest_index(cw, ow, rule) != ix).sum())
    assert differs["exact"] > 0 and differs["f64"] > 0, differs
