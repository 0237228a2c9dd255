"""Float64 restatement of the perspective-warp rule of `gfc_warp_perspective` (include/gfc_amd.h), numpy only.

UNPINNED against OpenCV: the rule restates cv2.warpPerspective with INTER_LINEAR and BORDER_CONSTANT 0 (the function the
reference's pair generator calls, gluefactory/datasets/homographies.py:37-44), and OpenCV is not installed where this
suite runs.  THIS FILE is the pin of the kernel: the same source position arithmetic in float64 (same association), the
same 1/32-pixel grid, the same fp32 taps and exact weights -- but the four products and their sum in float64.

Per destination pixel (x, y): X = M0 x + (M1 y + M2), Y, W alike; W <- 32 / W when W != 0 else 0; fX = X W, fY = Y W
saturated to the int32 range, rounded half to even -> qx, qy; cell (qx >> 5, qy >> 5), fractions (q & 31) / 32; a tap
outside the WINDOW counts as 0.
"""
import numpy as np

INT_MIN, INT_MAX = -2147483648.0, 2147483647.0
GRAY = (np.float32(0.299), np.float32(0.587), np.float32(0.114))  # data["image"].new_tensor([...]): fp32 constants


def to_float(u8):
    """numpy_image_to_torch (gluefactory/utils/image.py:148-156): uint8 HxWxC / HxW -> float32 CxHxW, value / 255."""
    u8 = np.asarray(u8)
    chw = u8.transpose(2, 0, 1) if u8.ndim == 3 else u8[None]
    return (chw / 255.0).astype(np.float32)


def source_positions(M, size):
    """-> (fX, fY) float64 [OH,OW]: the saturated source positions in 1/32 pixels, before rounding."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    oh, ow = size
    x = np.arange(ow, dtype=np.float64)[None, :]
    y = np.arange(oh, dtype=np.float64)[:, None]
    X = M[0, 0] * x + (M[0, 1] * y + M[0, 2])
    Y = M[1, 0] * x + (M[1, 1] * y + M[1, 2])
    W = M[2, 0] * x + (M[2, 1] * y + M[2, 2])
    nz = W != 0
    W = np.where(nz, 32.0 / np.where(nz, W, 1.0), 0.0)
    return np.clip(X * W, INT_MIN, INT_MAX), np.clip(Y * W, INT_MIN, INT_MAX)


def warp(plane, M, size, window=None):
    """plane: float32 [C,H,W] (a converted source); window (left, top, cw, ch) or None for the whole plane; size (OH, OW).
    -> (out float64 [C,OH,OW], max_tap float64 [OH,OW] the largest |tap| a pixel used over all
    channels, unsure bool [OH,OW]: fX or fY within 1e-7 of a half-integer, where another association of the float64 sum
    may round to the other neighbour)."""
    plane = np.asarray(plane, dtype=np.float32)
    c, h, w = plane.shape
    left, top, cw, ch = (0, 0, w, h) if window is None else window
    assert 0 <= left and 0 <= top and cw > 0 and ch > 0 and left + cw <= w and top + ch <= h
    win = plane[:, top: top + ch, left: left + cw].astype(np.float64)
    fX, fY = source_positions(M, size)
    unsure = (np.abs(fX - np.floor(fX) - 0.5) <= 1e-7) | (np.abs(fY - np.floor(fY) - 0.5) <= 1e-7)
    qx, qy = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    sx, sy = qx >> 5, qy >> 5
    ax, ay = (qx & 31) / 32.0, (qy & 31) / 32.0

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < cw) & (yy >= 0) & (yy < ch)
        v = win[:, np.clip(yy, 0, ch - 1), np.clip(xx, 0, cw - 1)]
        return np.where(ok[None], v, 0.0)

    t00, t01, t10, t11 = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    out = t00 * ((1 - ax) * (1 - ay)) + t01 * (ax * (1 - ay)) + t10 * ((1 - ax) * ay) + t11 * (ax * ay)
    max_tap = np.max(np.abs(np.stack([t00, t01, t10, t11])), axis=(0, 1))
    return out, max_tap, unsure


def bound(max_tap, gray=False):
    """|out - ref64| allowed per pixel: four product roundings and three sums on magnitudes <= the largest tap (the
    weights are exact, non-negative and sum to 1) = 7 ulp-sized steps of 2^-24 max|tap|; the grey sum adds three products
    and two sums on magnitudes <= max|tap| (its weights sum to 1): 5 more."""
    return (12 if gray else 7) * 2.0 ** -24 * max_tap


def gray_of(ref):
    """The grey reference of a colour reference triple of `warp` (the sum is taken after the warp)."""
    out, max_tap, unsure = ref
    return (np.float64(GRAY[0]) * out[0] + np.float64(GRAY[1]) * out[1] + np.float64(GRAY[2]) * out[2])[None], max_tap, unsure


def check(out, ref, gray=False, what=""):
    """Assert one warped item against `ref` = warp(...) of the same item (colour; with gray the grey sum is derived
    here); prints the figures first.  -> number of pixels left out (the caller holds the case's total to 0.01 %)."""
    ref, max_tap, unsure = gray_of(ref) if gray else ref
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = np.abs(out - ref).max(axis=0)
    lim = bound(max_tap, gray)
    bad = (err > lim) & ~unsure
    worst = float((err - lim)[~unsure].max()) if (~unsure).any() else 0.0
    print(f"warp {what}: max err {float(err[~unsure].max() if (~unsure).any() else 0):.3e}, largest bound "
          f"{float(lim.max()):.3e}, worst margin {worst:.3e}, left out {int(unsure.sum())} of {unsure.size}")
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), np.argwhere(bad)[:5].tolist())
    return int(unsure.sum())
