"""`gfc_warp_perspective` (csrc/warp.hip) against the float64 restatement of tests/warp_reference.py.

UNPINNED against OpenCV (absent): the kernel and the restatement both restate cv2.warpPerspective's INTER_LINEAR /
BORDER_CONSTANT 0 rule; what is held here is that the kernel computes THAT rule.

Bound (tests/warp_reference.bound): every compared pixel |out - ref64| <= 7 * 2^-24 * max|tap| (four product roundings
and three sums on magnitudes <= the largest tap, the exact weights summing to 1), + 5 * 2^-24 * max|tap| for `gray`;
max|tap| is taken per pixel.  A pixel is left out only when the restatement's fX or fY lies within 1e-7 of a
half-integer (another association of the float64 sum may then round the other way); at most 0.01 % of a case's pixels.

Small shapes: two sources of 29 x 37 (H x W), window (3, 2, 31, 24), output 21 x 33 (more than one 32 x 8 block in both
directions, neither a multiple of the block), the plane outside the window filled with 1.0 so that a tap leaking out of
the window shows.  Benchmark size: two 540 x 720 x 3 byte sources, the EndoPatches window and patch, ten fixture matrices.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "endopatches_homographies.npz")
H, W, WINDOW, SIZE = 29, 37, (3, 2, 31, 24), (21, 33)
_c, _s = np.cos(0.3), np.sin(0.3)
ITEMS = [  # (what, destination -> source matrix); item i warps source i % 2
    ("identity", np.eye(3)),
    ("integer shift", np.array([[1, 0, 2], [0, 1, -1], [0, 0, 1.0]])),
    ("shift by (0.5, 0.25)", np.array([[1, 0, 0.5], [0, 1, 0.25], [0, 0, 1.0]])),
    ("rotation with perspective", np.array([[_c, -_s, 4.3], [_s, _c, -3.1], [1e-3, -5e-4, 1.0]])),
    ("wholly outside", np.array([[1, 0, 1000], [0, 1, 1000], [0, 0, 1.0]])),
    ("W = 0 at x = 32", np.array([[1, 0, 0], [0, 1, 0], [0.125, 0, -4.0]])),
    ("one pixel past the window edge", np.array([[1, 0, -1], [0, 1, -1], [0, 0, 1.0]])),
    ("identity, the other source", np.eye(3)),
]


def _sources(kind, c):
    """Two sources: -> (device tensor for the kernel, [float32 CHW plane per source]).  fp32 sources hold multiples of
    1/64 below 4 (every product with an n/1024 weight and every sum is exact in fp32); outside the window: 1.0."""
    g = np.random.RandomState(100 * c + (kind == "u8"))
    left, top, cw, ch = WINDOW
    if kind == "u8":
        u8 = np.full((2, H, W, c), 255, np.uint8)
        u8[:, top: top + ch, left: left + cw] = g.randint(0, 256, (2, ch, cw, c))
        return torch.from_numpy(u8).cuda(), [wr.to_float(u) for u in u8]
    f = np.ones((2, c, H, W), np.float32)
    f[:, :, top: top + ch, left: left + cw] = g.randint(0, 256, (2, c, ch, cw)).astype(np.float32) / 64.0
    return torch.from_numpy(f).cuda(), [p for p in f]


def _window_image(plane, dy=0, dx=0):
    """The window shifted by whole pixels and cut / zero-padded to SIZE: out[y, x] = window[y + dy, x + dx]."""
    left, top, cw, ch = WINDOW
    win = plane[:, top: top + ch, left: left + cw]
    out = np.zeros((plane.shape[0], *SIZE), np.float32)
    for y in range(SIZE[0]):
        for x in range(SIZE[1]):
            if 0 <= y + dy < ch and 0 <= x + dx < cw:
                out[:, y, x] = win[:, y + dy, x + dx]
    return out


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_small_items_in_one_launch(kind, c):
    from glue_factory_colon_amd import homographies as hg

    src, planes = _sources(kind, c)
    index = torch.tensor([i % 2 for i in range(len(ITEMS))], dtype=torch.int32).cuda()
    mats = torch.from_numpy(np.stack([m for _, m in ITEMS])).cuda()
    out = hg.warp_perspective(src, index, mats, SIZE, crop=WINDOW).cpu().numpy()
    assert out.shape == (len(ITEMS), c, *SIZE) and out.dtype == np.float32
    refs = [wr.warp(planes[i % 2], m, SIZE, WINDOW) for i, (_, m) in enumerate(ITEMS)]
    left_out = sum(wr.check(out[i], refs[i], what=f"{kind} C={c} {what}") for i, (what, _) in enumerate(ITEMS))
    assert left_out == 0  # 0.01 % of 8 x 693 pixels
    # identity and whole-pixel shifts: the converted window itself, bit for bit
    assert np.array_equal(out[0], _window_image(planes[0]))
    assert np.array_equal(out[7], _window_image(planes[1]))
    assert np.array_equal(out[1], _window_image(planes[1], dy=-1, dx=2))
    # one pixel past the edge: row 0 / column 0 read window (-1, .) / (., -1), column 32 reads window column 31 + 1 --
    # all inside the plane (filled with 1.0 there), outside the window: 0
    assert np.array_equal(out[6], _window_image(planes[0], dy=-1, dx=-1))
    assert not out[6][:, 0].any() and not out[6][:, :, 0].any() and not out[6][:, :, 32].any() and out[6].any()
    assert not out[4].any()
    # W = 0 exactly at x = 32: source cell (0, 0), fractions 0
    assert np.array_equal(out[5][:, :, 32], np.repeat(planes[1][:, WINDOW[1], WINDOW[0]][:, None], SIZE[0], axis=1))
    if kind == "f32":  # dyadic taps: every product and sum is exact, so the fp32 result IS the float64 one
        for i in (2, 3, 5):
            assert np.array_equal(out[i].astype(np.float64), refs[i][0]), ITEMS[i][0]
    if c == 3:
        gray = hg.warp_perspective(src, index, mats, SIZE, crop=WINDOW, gray=True).cpu().numpy()
        assert gray.shape == (len(ITEMS), 1, *SIZE)
        assert sum(wr.check(gray[i], refs[i], gray=True, what=f"{kind} gray {what}") for i, (what, _) in enumerate(ITEMS)) == 0
    # no crop: the whole plane is the image, and a single source may come without the batch dimension
    whole = hg.warp_perspective(src[0], index[:1] * 0, mats[3:4], SIZE).cpu().numpy()
    assert wr.check(whole[0], wr.warp(planes[0], ITEMS[3][1], SIZE), what=f"{kind} C={c} whole plane") == 0


def test_benchmark_size_from_fixture_matrices():
    from glue_factory_colon_amd import homographies as hg

    fx = np.load(GOLDEN)
    window, size = (81, 55, 582, 429), (426, 580)
    assert tuple(fx["size"]) == window[2:] and tuple(fx["patch"]) == size[::-1]
    g = np.random.RandomState(5)
    u8 = g.randint(0, 256, (2, 540, 720, 3)).astype(np.uint8)
    planes = [wr.to_float(u) for u in u8]
    keys = [f"H_{li}_{s}" for li, s in ((0, 0), (1, 0), (1, 1), (2, 2), (2, 3), (3, 0), (3, 1), (3, 4), (3, 5), (1, 5))]
    mats = np.stack([np.linalg.inv(fx[k]) for k in keys])
    index = [i % 2 for i in range(len(keys))]
    refs = [wr.warp(planes[index[i]], mats[i], size, window) for i in range(len(keys))]
    src, dev_i, dev_m = torch.from_numpy(u8).cuda(), torch.tensor(index, dtype=torch.int32).cuda(), torch.from_numpy(mats).cuda()
    for gray in (False, True):
        out = hg.warp_perspective(src, dev_i, dev_m, size, crop=window, gray=gray).cpu().numpy()
        assert out.shape == (len(keys), 1 if gray else 3, *size)
        left_out = sum(wr.check(out[i], refs[i], gray=gray, what=f"{keys[i]}{' gray' if gray else ''}") for i in range(len(keys)))
        assert left_out <= 1e-4 * len(keys) * size[0] * size[1], left_out
        assert all(float(np.abs(o).max()) > 0.5 for o in out)  # (every fixture warp samples inside the source)


def test_refusals_launch_nothing():
    from glue_factory_colon_amd import _native as nat
    from glue_factory_colon_amd import homographies as hg

    lib = nat.lib()
    src = torch.zeros((1, 3, 16, 16), device="cuda")
    two = torch.zeros((1, 2, 16, 16), device="cuda")
    out = torch.full((1, 3, 8, 8), 7.0, device="cuda")
    index = torch.zeros(1, dtype=torch.int32, device="cuda")
    mats = torch.eye(3, dtype=torch.float64, device="cuda")[None].contiguous()
    st = nat.stream_ptr(src.device)

    def call(s=src, c=3, window=(0, 0, 16, 16), size=(8, 8), gray=0, kind=0, b=1, idx=index, m=mats, dst=out):
        return nat.STATUS[lib.gfc_warp_perspective(nat.ptr(s), kind, 1, c, 16, 16, *window, nat.ptr(idx), nat.ptr(m), b, gray,
                                                   nat.ptr(dst), size[0], size[1], st)]

    for window in ((10, 0, 7, 16), (0, 10, 16, 7), (-1, 0, 8, 8), (0, 0, 0, 8), (0, 0, 17, 16)):
        assert call(window=window) == "GFC_ERR_INVALID", window
    assert call(s=two, c=2) == "GFC_ERR_INVALID"
    assert call(size=(0, 8)) == "GFC_ERR_INVALID" and call(size=(8, -1)) == "GFC_ERR_INVALID"
    assert call(c=1, gray=1) == "GFC_ERR_INVALID"
    assert call(kind=2) == "GFC_ERR_INVALID" and call(b=0) == "GFC_ERR_INVALID"
    assert call(idx=None) == "GFC_ERR_INVALID" and call(m=None) == "GFC_ERR_INVALID" and call(dst=None) == "GFC_ERR_INVALID"
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    assert call() == "GFC_OK"
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    # a source index outside [0, S) is device data: no read, a zero image
    out.fill_(7.0)
    assert call(idx=torch.tensor([5], dtype=torch.int32, device="cuda")) == "GFC_OK"
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        hg.warp_perspective(src, index, mats, (8, 8), crop=(10, 0, 7, 16))
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        hg.warp_perspective(src[:, :1], index, mats, (8, 8), gray=True)
