"""`gfc_preprocess_resample` (csrc/preprocess.hip: crop window -> nearest / area resample, one launch) against the
restatement of tests/posed_reference.py, at the smallest shapes that can go wrong: odd sizes, an up-scale, an axis left
unchanged, a single output pixel, more than one 32x8 block, and a crop whose packed bits straddle bytes (W = 53,
left = 5).  `nearest` and the crop are exact (torch.equal against F.interpolate / slicing).  The blurred `nearest`
holds the bound tests/test_preprocess.py holds the same blur code to (5e-7 for sources in [0, 1]: here times max|src|).
`area` is held to the fp32 summation bound against float64 box means: n additions and one division on values of
magnitude <= max|src| give at most (n + 2) * 2^-24 * max|src|, n the largest box of the shape."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posed_reference as pr  # noqa: E402

from oracle import preprocess as opp  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [f"{h}x{w}-{oh}x{ow}{'-crop' if crop else ''}" for (h, w), (oh, ow), crop in pr.SHAPES]
BLURRED = [pr.SHAPES[0], pr.SHAPES[2], pr.SHAPES[5]]  # the two down-scaling shapes and the cropped one


def _depth(hw, c=1, seed=0):
    """Depth-like planes: values in [0.5, 5) with about a fifth of the pixels exactly 0."""
    g = torch.Generator().manual_seed(1000 * hw[0] + hw[1] + seed)
    x = 0.5 + 4.5 * torch.rand((c, *hw), generator=g)
    x[torch.rand((c, *hw), generator=g) < 0.2] = 0.0
    return x


def _mask(hw, seed=0):
    g = torch.Generator().manual_seed(77 * hw[0] + hw[1] + seed)
    return torch.rand(hw, generator=g) < 0.4


def _packed(mask):
    return torch.from_numpy(np.packbits(mask.numpy().reshape(-1)))


@pytest.mark.parametrize("hw,size,crop", pr.SHAPES, ids=IDS)
def test_nearest_is_torchs_nearest(hw, size, crop):
    from glue_factory_colon_amd import image_preprocessor as ip

    x = _depth(hw, c=2)
    left, top, _, _ = pr.window(hw, crop)
    x[0, top, left] = 0.0  # output pixel (0, 0) of channel 0 takes this one: a zero reaches even a 1 x 1 output
    ref = F.interpolate(pr.crop_plane(x, crop)[None], size=size, mode="nearest")[0]
    out, valid = ip.resample(x.cuda(), size, "nearest", crop=crop, want_valid=True)
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), ref)
    assert int((ref == 0).sum()) > 0 and int((ref > 0).sum()) > 0 and torch.equal(valid.cpu(), (ref > 0).float())
    assert torch.equal(ip.resample(x[0].cuda(), size, "nearest", crop=crop).cpu(), ref[0])  # [H,W] in, [oh,ow] out
    # value_scale: the product in fp32 at load, i.e. torch's `depth * s` before crop and resize
    scaled = ip.resample(x.cuda(), size, "nearest", crop=crop, value_scale=0.37).cpu()
    assert torch.equal(scaled, F.interpolate(pr.crop_plane(x * 0.37, crop)[None], size=size, mode="nearest")[0])
    # the two mask sources: a byte plane, and numpy.packbits of the whole uncropped mask
    m = _mask(hw)
    mref = F.interpolate(pr.crop_plane(m.float(), crop)[None, None], size=size, mode="nearest")[0, 0] > 0.5
    plane = ip.resample(m.cuda(), size, "nearest", crop=crop)
    bits = ip.resample(_packed(m).cuda(), size, "nearest", crop=crop, bits_shape=hw)
    assert plane.dtype == torch.bool and bits.dtype == torch.bool
    assert torch.equal(plane.cpu(), mref) and torch.equal(bits.cpu(), mref)
    # a batch of two planes: every plane starts at its own ceil(H W / 8) bytes
    m2 = _mask(hw, seed=1)
    both = ip.resample(torch.stack([_packed(m), _packed(m2)]).cuda(), size, "nearest", crop=crop, bits_shape=hw).cpu()
    assert torch.equal(both[0], mref)
    assert torch.equal(both[1], F.interpolate(pr.crop_plane(m2.float(), crop)[None, None], size=size, mode="nearest")[0, 0] > 0.5)


@pytest.mark.parametrize("hw,size,crop", BLURRED, ids=[IDS[0], IDS[2], IDS[5]])
def test_nearest_after_the_antialias_blur(hw, size, crop):
    from glue_factory_colon_amd import image_preprocessor as ip

    x = _depth(hw, c=2)
    ref = pr.resample(x, size, "nearest", crop=crop, antialias=True)
    assert not torch.equal(ref, pr.resample(x, size, "nearest", crop=crop))  # the blur does something here
    out = ip.resample(x.cuda(), size, "nearest", crop=crop, antialias=True).cpu()
    err, bound = float((out - ref).abs().max()), 5e-7 * float(x.abs().max())
    print(f"blurred nearest {hw}->{size}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    # reflection happens at the WINDOW's edge: constant inside, something else outside -> the constant (the weights sum
    # to 1 within rounding, so "the constant" is held to the same bound; a tap outside the window would be off by ~97)
    left, top, cw, ch = pr.window(hw, crop)
    big = torch.full((1, hw[0] + 8, hw[1] + 8), 100.0)
    big[:, top + 4: top + 4 + ch, left + 4: left + 4 + cw] = 2.5
    flat = ip.resample(big.cuda(), size, "nearest", crop=(left + 4, top + 4, cw, ch), antialias=True).cpu()
    assert float((flat - 2.5).abs().max()) <= 5e-7 * 2.5, float((flat - 2.5).abs().max())
    # a mask source is blurred as 0 / 1 floats, then thresholded (pixels the restatement puts within 1e-6 of 0.5 excluded)
    m = _mask(hw)
    mref = pr.resample(m.float()[None], size, "nearest", crop=crop, antialias=True)[0]
    bits = ip.resample(_packed(m).cuda(), size, "nearest", crop=crop, antialias=True, bits_shape=hw).cpu()
    sure = (mref - 0.5).abs() > 1e-6
    assert torch.equal(bits[sure], (mref > 0.5)[sure])


@pytest.mark.parametrize("hw,size,crop", pr.SHAPES, ids=IDS)
def test_area_is_the_box_mean(hw, size, crop):
    from glue_factory_colon_amd import image_preprocessor as ip

    x = _depth(hw, c=2)
    ref, n = pr.area_f64(x, size, crop)
    out = ip.resample(x.cuda(), size, "area", crop=crop).cpu()
    err, bound = float((out.double() - ref).abs().max()), (n + 2) * 2.0 ** -24 * float(x.abs().max())
    print(f"area {hw}->{size}: largest box {n}, max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    # the decoded uint8 image, C = 3: the /255 table of numpy_image_to_torch, then the same boxes
    g = torch.Generator().manual_seed(hw[0])
    u8 = torch.randint(0, 256, (*hw, 3), generator=g, dtype=torch.uint8)
    xf = opp.numpy_image_to_torch(u8.numpy())
    ref, n = pr.area_f64(xf, size, crop)
    out = ip.resample(u8.cuda(), size, "area", crop=crop).cpu()
    assert out.shape == (3, *size)
    err, bound = float((out.double() - ref).abs().max()), (n + 2) * 2.0 ** -24 * float(xf.max())
    print(f"area u8 {hw}->{size}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


def test_endomapper_crop_end_to_end():
    """540x720 image, depth and packed mask -> 512x672 through the window (36, 14), no resize: host slicing exactly."""
    from glue_factory_colon_amd import image_preprocessor as ip

    g = torch.Generator().manual_seed(9)
    u8 = torch.randint(0, 256, (540, 720, 3), generator=g, dtype=torch.uint8)
    depth, mask = _depth((540, 720))[0], _mask((540, 720))
    win = ip.endomapper_dense_window(540, 720)
    assert win == (36, 14, 672, 512)
    img = ip.resample(u8.cuda(), (512, 672), "nearest", crop=win).cpu()
    assert torch.equal(img, opp.numpy_image_to_torch(u8.numpy())[:, 14:526, 36:708])
    d, v = ip.resample(depth.cuda(), (512, 672), "nearest", crop=win, value_scale=0.37, want_valid=True)
    assert torch.equal(d.cpu(), (depth * 0.37)[14:526, 36:708]) and torch.equal(v.cpu(), (depth[14:526, 36:708] > 0).float())
    m = ip.resample(_packed(mask).cuda(), (512, 672), "nearest", crop=win, bits_shape=(540, 720)).cpu()
    assert torch.equal(m, mask[14:526, 36:708])


def test_error_returns():
    from glue_factory_colon_amd import _native as nat
    from glue_factory_colon_amd import image_preprocessor as ip

    lib = nat.lib()
    x = torch.zeros((1, 1, 256, 256), device="cuda")
    out = torch.zeros((1, 1, 16, 16), device="cuda")
    st = nat.stream_ptr(x.device)

    def call(src, dst, window=(0, 0, 256, 256), kind=0, mode=0, antialias=0, size=(16, 16), valid=None, c=1):
        return lib.gfc_preprocess_resample(nat.ptr(src), kind, 1, c, 256, 256, *window, mode, antialias, 1.0, nat.ptr(dst),
                                           nat.ptr(valid), size[0], size[1], st)

    assert nat.STATUS[call(x, out)] == "GFC_OK"
    for window in ((250, 0, 7, 256), (0, 250, 256, 7), (-1, 0, 16, 16), (0, 0, 0, 16), (0, 0, 257, 256)):
        assert nat.STATUS[call(x, out, window)] == "GFC_ERR_INVALID", window
    assert nat.STATUS[call(None, out)] == "GFC_ERR_INVALID" and nat.STATUS[call(x, None)] == "GFC_ERR_INVALID"
    assert nat.STATUS[call(x, out, kind=4)] == "GFC_ERR_INVALID" and nat.STATUS[call(x, out, mode=2)] == "GFC_ERR_INVALID"
    assert nat.STATUS[call(x, out, kind=3, c=2)] == "GFC_ERR_INVALID"  # a mask source has one channel
    one = torch.zeros((1, 1, 1, 1), device="cuda")
    assert nat.STATUS[call(x, one, antialias=1, size=(1, 1))] == "GFC_ERR_UNSUPPORTED"  # 256x: 511 taps > PP_MAX_KS
    assert nat.STATUS[call(x, one, antialias=0, size=(1, 1))] == "GFC_OK"
    assert nat.STATUS[call(x, out, mode=1, antialias=1)] == "GFC_ERR_UNSUPPORTED"  # area after a blur is not built
    assert nat.STATUS[call(x, out, (0, 0, 256, 1), antialias=1, size=(1, 16))] == "GFC_ERR_INVALID"  # reflect pad >= size
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        ip.resample(x, (16, 16), "nearest", crop=(250, 0, 7, 256))
    with pytest.raises(nat.NativeError, match="GFC_ERR_UNSUPPORTED"):
        ip.resample(x, (1, 1), "nearest", antialias=True)
    with pytest.raises(NotImplementedError, match="'area' with antialias=True on a down-scale"):
        ip.resample(x, (16, 16), "area", antialias=True)
    with pytest.raises(NotImplementedError):
        ip.resample(x, (16, 16), "bicubic")
    torch.cuda.synchronize()


def test_image_preprocessor_nearest_and_area():
    from glue_factory_colon_amd.image_preprocessor import ImagePreprocessor

    x = _depth((37, 53), c=3)
    for mode, antialias in (("nearest", False), ("area", False), ("nearest", True)):
        pre = ImagePreprocessor({"resize": 23, "side": "long", "interpolation": mode, "antialias": antialias})
        d = pre(x.cuda())
        ref = opp.preprocess(x, resize=23, side="long", antialias=False)  # (sizes, scales, transform; not its image)
        assert tuple(d["image"].shape) == (3, 16, 23) == tuple(ref["image"].shape)
        assert torch.equal(d["scales"].cpu(), ref["scales"]) and np.array_equal(d["image_size"], ref["image_size"])
        assert np.array_equal(d["original_image_size"], ref["original_image_size"])
        assert np.allclose(d["transform"], np.diag([23 / 53, 16 / 37, 1.0]), atol=1e-7)
        want = pr.resample(x, (16, 23), mode, antialias=antialias)
        if mode == "nearest" and not antialias:
            assert torch.equal(d["image"].cpu(), want)
        else:
            tol = 5e-7 * float(x.max()) if mode == "nearest" else (9 + 2) * 2.0 ** -24 * float(x.max())  # boxes <= 3x3 here
            assert float((d["image"].cpu() - want).abs().max()) <= tol
    # the call argument overrides the configuration, as the reader passes interpolation="nearest" for depth
    pre = ImagePreprocessor({"resize": 23, "side": "long", "antialias": False})
    assert torch.equal(pre(x.cuda(), interpolation="nearest")["image"].cpu(), pr.resample(x, (16, 23), "nearest"))
    # the size already matches: the input itself
    same = x.cuda()
    assert ImagePreprocessor({"resize": 53, "interpolation": "nearest"})(same)["image"] is same
    with pytest.raises(NotImplementedError):
        ImagePreprocessor({"resize": 23, "interpolation": "bicubic"})(x.cuda())
    with pytest.raises(NotImplementedError, match="'area' with antialias=True on a down-scale"):
        ImagePreprocessor({"resize": 23, "interpolation": "area"})(x.cuda())
    pre = ImagePreprocessor({"resize": 106, "interpolation": "area"})  # an up-scale: no blur, antialias or not
    up = pre(x.cuda())["image"].cpu()
    ref, n = pr.area_f64(x, tuple(pre.get_new_image_size(37, 53)))
    assert float((up.double() - ref).abs().max()) <= (n + 2) * 2.0 ** -24 * float(x.max())
    with pytest.raises(ValueError, match="align_corners"):
        ImagePreprocessor({"resize": 23, "interpolation": "nearest", "align_corners": True})(x.cuda())
