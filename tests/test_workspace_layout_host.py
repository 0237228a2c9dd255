"""Workspace layouts, host side (no GPU, no HIP call).

Every `*_workspace_bytes` export returns the `total` of the one layout function its entry point carves pointers from
(csrc/common.h: gfc_slots).  Two things are pinned here:

1. the byte counts are those of the library before that refactor (source hash 94c8050853c2): the literal tables below
   were recorded from a build of it, over arguments that straddle every branch of the size functions;
2. every entry point that takes a workspace refuses one that is a byte short with GFC_ERR_WORKSPACE, behind its
   argument checks and before anything is launched -- the pointers passed are made up and never dereferenced.  No call
   here passes ws_bytes >= need.  (gfc_attention / gfc_attention_f16 never refuse: they lower their key split to what
   the scratch holds.)
"""
import ctypes

import pytest

from glue_factory_colon_amd import _native as nat

INVALID, WORKSPACE = 1, 2
ALT128_M, ALT128_N = [8 + i for i in range(128)], [9] * 128  # 128 pairs, no two neighbours equal: 128 groups

# fmt: off
# (arguments, bytes); 0 = refused.  What the cases straddle: attention -- ceil(max_nq / 128) * heads * n_problems
# reaching 256; layer -- 8192 / 8193 rows (the key-split scratch ends); assignment -- M around multiples of AS_RB = 64;
# SuperPoint -- C = 1 / 3 and sizes that are no multiple of 8; RANSAC -- rs_splits' limits ceil(512 / B) and
# floor(num_hypotheses / 256); sizes that are no multiple of 256 bytes throughout; every argument error.
SIZES = {
    "gfc_attention_workspace_bytes": [
        ((2, 1024, 4), 17301504), ((64, 2048, 4), 0), ((63, 128, 4), 68124672), ((64, 128, 4), 0), ((64, 129, 4), 0),
        ((1, 1, 1), 2304), ((2, 70, 4), 1182720), ((3, 333, 5), 10549504), ((1, 32640, 1), 68935680),
        ((1, 32641, 1), 0), ((51, 128, 5), 68935680), ((0, 10, 4), 0), ((2, 0, 4), 0), ((2, 10, 0), 0),
        ((-1, 10, 4), 0),
    ],
    "gfc_lg_layer_workspace_bytes": [
        ((2048,), 31981568), ((8192,), 127926272), ((8193,), 58727424), ((1,), 15616), ((7,), 109312),
        ((390,), 6090240), ((100000,), 716800000), ((0,), 0), ((-1,), 0),
    ],
    "gfc_lg_assign_workspace_bytes": [
        ((2, 65, 130), 416000), ((1, 1, 1), 3840), ((1, 63, 5), 72448), ((1, 64, 5), 73472), ((1, 65, 5), 74752),
        ((3, 128, 67), 617472), ((3, 129, 67), 623872), ((2, 1024, 1024), 4792320), ((1, 1500, 2100), 4557056),
        ((1, 40, 17), 60672), ((0, 4, 4), 0), ((1, 0, 4), 0), ((1, 4, 0), 0), ((-1, 4, 4), 0),
    ],
    "gfc_nn_workspace_bytes": [
        ((2, 65, 130), 7936), ((1, 1, 1), 256), ((1, 63, 5), 1536), ((1, 64, 5), 1536), ((1, 65, 5), 1536),
        ((3, 128, 67), 11776), ((3, 129, 67), 11776), ((2, 1024, 1024), 81920), ((1, 1500, 2100), 72192),
        ((1, 40, 17), 1280), ((0, 4, 4), 0), ((1, 0, 4), 0), ((1, 4, 0), 0), ((-1, 4, 4), 0),
    ],
    "gfc_sp_workspace_bytes": [
        ((2, 1, 480, 640), 78643200), ((2, 3, 480, 640), 81100800), ((1, 1, 8, 8), 8192), ((1, 3, 8, 8), 8448),
        ((2, 1, 64, 96), 1572864), ((2, 3, 64, 96), 1622016), ((1, 1, 100, 36), 460800), ((1, 3, 99, 37), 466432),
        ((3, 1, 17, 23), 135168), ((3, 3, 17, 23), 140032), ((0, 1, 64, 64), 0), ((1, 1, 7, 64), 0),
        ((1, 3, 64, 7), 0), ((-2, 1, 64, 64), 0),
    ],
    "gfc_sp_select_workspace_bytes": [
        ((2, 480, 640), 4915200), ((2, 40, 56), 35840), ((1, 1, 1), 256), ((3, 17, 23), 9472), ((1, 5, 3), 256),
        ((0, 4, 4), 0),
    ],
    "gfc_sp_nms_select_workspace_bytes": [
        ((2, 480, 640), 4915456), ((2, 40, 56), 36096), ((1, 1, 1), 512), ((3, 17, 23), 9728), ((65, 5, 3), 8448),
        ((0, 4, 4), 0),
    ],
    "gfc_disk_select_workspace_bytes": [
        ((2, 48, 64), 73728), ((2, 40, 56), 53760), ((1, 1, 1), 768), ((3, 17, 23), 14592), ((0, 4, 4), 0),
        ((1, 0, 4), 0), ((1, 4, 0), 0), ((-1, 4, 4), 0),
    ],
    "gfc_disk_instnorm_workspace_bytes": [
        ((2, 64), 131072), ((1, 4), 4096), ((3, 16), 49152), ((1, 5), 5120), ((0, 4), 0), ((2, 0), 0), ((-1, 4), 0),
    ],
    "gfc_lg_adaptive_step_workspace_bytes": [
        ((3, 1000), 4608), ((1, 1), 768), ((128, 5000), 24320), ((2, 63), 768), ((2, 64), 768), ((2, 65), 1024),
        ((17, 390), 2816), ((1, 2796202), 11185408), ((0, 10), 0), ((129, 10), 0), ((1, 0), 0), ((1, 2796203), 0),
    ],
    "gfc_eval_homography_ransac_workspace_bytes": [
        ((2, 1000, 3, 4096), 41728), ((2, 100, 3, 512), 5120), ((20, 100, 8, 255), 42496), ((20, 100, 8, 256), 42496),
        ((20, 100, 8, 511), 42496), ((20, 100, 8, 512), 44288), ((3, 100, 8, 43520), 55552),
        ((3, 100, 8, 43776), 56064), ((3, 100, 8, 44032), 56064), ((1, 100, 3, 1048576), 20992),
        ((511, 7, 1, 4096), 86016), ((512, 7, 1, 4096), 79872), ((513, 7, 1, 4096), 81152), ((3, 0, 2, 1000), 768),
        ((5, 33, 5, 1), 4352), ((0, 10, 3, 512), 0), ((2, -1, 3, 512), 0), ((2, 10, 0, 512), 0), ((2, 10, 9, 512), 0),
        ((2, 10, 3, 0), 0),
    ],
    # the homography estimator's arguments; recorded from a build of the commit before the two estimators shared one
    # layout function (the five slots above plus 3288 bytes of solver scratch per (pair, threshold))
    "gfc_eval_relative_pose_ransac_workspace_bytes": [
        ((2, 1000, 3, 4096), 61696), ((2, 100, 3, 512), 25088), ((20, 100, 8, 255), 568576),
        ((20, 100, 8, 256), 568576), ((20, 100, 8, 511), 568576), ((20, 100, 8, 512), 570368),
        ((3, 100, 8, 43520), 134656), ((3, 100, 8, 43776), 135168), ((3, 100, 8, 44032), 135168),
        ((1, 100, 3, 1048576), 30976), ((511, 7, 1, 4096), 1766400), ((512, 7, 1, 4096), 1763328),
        ((513, 7, 1, 4096), 1767936), ((3, 0, 2, 1000), 20736), ((5, 33, 5, 1), 86784), ((0, 10, 3, 512), 0),
        ((2, -1, 3, 512), 0), ((2, 10, 0, 512), 0), ((2, 10, 9, 512), 0), ((2, 10, 3, 0), 0),
    ],
    "gfc_lg_workspace_bytes": [
        ((2, 65, 130), 6796032), ((1, 1, 1), 35584), ((1, 63, 5), 1185536), ((1, 64, 5), 1202944),
        ((1, 65, 5), 1220352), ((3, 128, 67), 10193920), ((3, 129, 67), 10246144), ((2, 1024, 1024), 71369216),
        ((1, 1500, 2100), 62726912), ((1, 40, 17), 993792), ((1, 2796201, 1), 25098709760),
        ((7, 2048, 2048), 257360896), ((0, 4, 4), 0), ((1, 0, 4), 0), ((1, 4, 0), 0), ((-1, 4, 4), 0),
        ((1, 2796202, 1), 0),
    ],
    "gfc_lg_packed_workspace_bytes": [
        ((2, 65, 130), 6390272), ((1, 1, 1), 33280), ((1, 63, 5), 1114624), ((1, 64, 5), 1131008),
        ((1, 65, 5), 1147392), ((3, 128, 67), 9585408), ((3, 129, 67), 9634560), ((2, 1024, 1024), 67109376),
        ((1, 1500, 2100), 58982912), ((1, 40, 17), 934400), ((1, 2796201, 1), 22190659584),
        ((7, 2048, 2048), 227542016), ((0, 4, 4), 0), ((1, 0, 4), 0), ((1, 4, 0), 0), ((-1, 4, 4), 0),
        ((1, 2796202, 1), 0),
    ],
    # the two split ground-truth labellers; recorded from a build of the commit before they shared the head of their
    # layouts (csrc/gt_sweep.h; source hash dd50ec4fbcab).  Slots of B (M + N) * 4, B (M + N) and B M * 4 bytes that are
    # no multiple of 256, the evaluation size, an empty side, and every argument error (B, M, N <= 65535)
    "gfc_gt_matches_sparse_map_workspace_bytes": [
        ((1, 1, 1), 1792), ((2, 17, 255), 12544), ((3, 257, 16), 20992), ((2, 65, 130), 10240),
        ((32, 2048, 2048), 3014656), ((1, 65535, 65535), 3014656), ((1, 0, 4), 0), ((1, 4, 0), 0), ((0, 4, 4), 0),
        ((-1, 4, 4), 0), ((1, -1, 4), 0), ((1, 65536, 4), 0), ((1, 4, 65536), 0), ((65536, 4, 4), 0),
    ],
    "gfc_gt_matches_roma_workspace_bytes": [
        ((1, 1, 1), 1280), ((2, 17, 255), 7936), ((3, 257, 16), 14336), ((2, 65, 130), 6656),
        ((32, 2048, 2048), 1966080), ((1, 65535, 65535), 1966080), ((1, 0, 4), 0), ((1, 4, 0), 0), ((0, 4, 4), 0),
        ((-1, 4, 4), 0), ((1, -1, 4), 0), ((1, 65536, 4), 0), ((1, 4, 65536), 0), ((65536, 4, 4), 0),
    ],
}
RAGGED_SIZES = [
    (([65], [130]), 3195392),
    (([65, 65, 40], [130, 130, 17]), 7324416),
    (([65, 40], [130, 17]), 4129280),
    (([5, 5, 2048, 2048, 7], [300, 300, 1000, 1000, 7]), 110101248),
    ((ALT128_M, ALT128_N), 81785088),
    (([33] * 128, [65] * 128), 99561728),
    (([4, 0], [4, 4]), 0),
    (([4, 4], [4, -1]), 0),
    (([4] * 129, [4] * 129), 0),
]
# fmt: on

_CASES = [(fn, args, want) for fn, cases in SIZES.items() for args, want in cases]


@pytest.mark.parametrize("fn,args,want", _CASES, ids=[f"{fn[4:-16]}{list(args)}" for fn, args, _ in _CASES])
def test_workspace_bytes_are_the_recorded_ones(fn, args, want):
    assert getattr(nat.lib(), fn)(*args) == want


def _ragged_bytes(m, n):
    b = len(m)
    return nat.lib().gfc_lg_ragged_workspace_bytes(b, (ctypes.c_int32 * b)(*m), (ctypes.c_int32 * b)(*n))


def test_ragged_workspace_bytes_are_the_recorded_ones():
    """1, 2 and 128 groups, and the refusals."""
    for (m, n), want in RAGGED_SIZES:
        assert _ragged_bytes(m, n) == want, (m[:4], n[:4], len(m))
    assert nat.lib().gfc_lg_packed_workspace_bytes(1, 65, 130) == RAGGED_SIZES[0][1]  # one group = the uniform batch


def test_anchor_sizes():
    """The sizes the layouts are known by (evaluation shapes)."""
    lib = nat.lib()
    assert lib.gfc_lg_layer_workspace_bytes(2048) == 31981568 and lib.gfc_lg_layer_workspace_bytes(8193) == 58727424
    assert lib.gfc_lg_assign_workspace_bytes(2, 65, 130) == 416000 and lib.gfc_nn_workspace_bytes(2, 65, 130) == 7936
    assert lib.gfc_sp_workspace_bytes(2, 1, 480, 640) == 78643200 and lib.gfc_sp_workspace_bytes(2, 3, 480, 640) == 81100800
    assert lib.gfc_sp_select_workspace_bytes(2, 480, 640) == 4915200
    assert lib.gfc_sp_nms_select_workspace_bytes(2, 480, 640) == 4915456
    assert lib.gfc_disk_select_workspace_bytes(2, 48, 64) == 73728 and lib.gfc_disk_instnorm_workspace_bytes(2, 64) == 131072
    assert lib.gfc_lg_adaptive_step_workspace_bytes(3, 1000) == 4608
    assert lib.gfc_eval_homography_ransac_workspace_bytes(2, 1000, 3, 4096) == 41728
    assert lib.gfc_lg_workspace_bytes(2, 65, 130) == 6796032 and lib.gfc_lg_packed_workspace_bytes(2, 65, 130) == 6390272
    assert lib.gfc_attention_workspace_bytes(2, 1024, 4) == 17301504 and lib.gfc_attention_workspace_bytes(64, 2048, 4) == 0


# ---------------------------------------------------------------------------------------- one byte short is refused
def f(n):
    """A non-null, 16-byte aligned host address that is never dereferenced."""
    return ctypes.c_void_p(0x1000 * n)


B, M, N = 2, 65, 130
R = B * (M + N)


# every per-layer pointer array of gfc_lg_params, in the header's order
LG_ARRAYS = ["wqkv", "bqkv", "s_out_w", "s_out_b", "s_ffn0_w", "s_ffn0_b", "s_ln_g", "s_ln_b", "s_ffn3_w", "s_ffn3_b",
             "c_qkv_w", "c_qkv_b", "c_out_w", "c_out_b", "c_ffn0_w", "c_ffn0_b", "c_ln_g", "c_ln_b", "c_ffn3_w", "c_ffn3_b",
             "final_proj_w", "final_proj_b", "matchability_w", "matchability_b", "token_w", "token_b",
             "wqkv16", "s_out_w16", "s_ffn0_w16", "s_ffn3_w16", "c_qkv_w16", "c_out_w16", "c_ffn0_w16", "c_ffn3_w16",
             "final_proj_w16"]


def _pointer_arrays(struct):
    """The fields of a parameter struct that are arrays of pointers, as the header declares them."""
    return [name for name, t in struct._fields_ if issubclass(t, ctypes.Array) and t._type_ is ctypes.c_void_p]


def _lg_params(precision=nat.GFC_LG_FP32, input_dim=256):
    """2 layers, every matrix of either precision 'present' (folded out_proj), decision heads on every layer."""
    assert _pointer_arrays(nat.LgParams) == LG_ARRAYS
    p = nat.LgParams()
    p.n_layers, p.input_dim, p.posenc_dim, p.precision = 2, input_dim, 2, precision
    p.posenc_wr = 0x1000
    if input_dim != 256:
        p.input_proj_w = p.input_proj_b = p.input_proj_w16 = 0x3000
    for name in _pointer_arrays(nat.LgParams):
        if name not in ("s_out_w", "s_out_b", "c_out_w", "c_out_b", "s_out_w16", "c_out_w16"):
            for i in range(2):
                getattr(p, name)[i] = 0x2000
    return p


def _short_calls():
    """name -> callable(ws_bytes) for every entry point with a workspace, and the size it asks for."""
    lib = nat.lib()
    calls = {}
    sp = nat.SpParams()
    sp.desc_dim, sp.conv_mode = 256, 0
    for c in (1, 3):
        calls[f"sp_dense_c{c}"] = (lib.gfc_sp_workspace_bytes(2, c, 64, 96), lambda ws, c=c: lib.gfc_sp_dense(
            ctypes.byref(sp), f(1), 2, c, 64, 96, f(2), f(3), f(4), ws, None, None))
    calls["sp_select"] = (lib.gfc_sp_select_workspace_bytes(2, 40, 56), lambda ws: lib.gfc_sp_select(
        f(1), 2, 40, 56, 0.0, 50, 50, f(2), f(3), f(4), f(5), ws, None))
    calls["sp_nms_select"] = (lib.gfc_sp_nms_select_workspace_bytes(2, 40, 56), lambda ws: lib.gfc_sp_nms_select(
        f(1), 2, 40, 56, 3, 0, None, 0.0, 50, 50, None, f(2), f(3), f(4), f(5), ws, None))
    calls["disk_nms_select"] = (lib.gfc_disk_select_workspace_bytes(2, 40, 56), lambda ws: lib.gfc_disk_nms_select(
        f(1), 2, 40, 56, 5, 0.0, 50, 50, f(2), f(3), f(4), f(5), ws, None))
    calls["disk_instnorm_stats"] = (lib.gfc_disk_instnorm_workspace_bytes(2, 64), lambda ws: lib.gfc_disk_instnorm_stats(
        f(1), 2, 8, 8, 64, 1e-5, f(2), f(3), f(4), ws, None))
    th = (ctypes.c_float * 3)(1.0, 2.0, 3.0)  # read on the host
    calls["eval_homography_ransac"] = (
        lib.gfc_eval_homography_ransac_workspace_bytes(2, 100, 3, 512), lambda ws: lib.gfc_eval_homography_ransac(
            f(1), f(2), f(3), None, None, None, 2, 100, 100, th, 3, 512, 3, 0, f(4), f(5), f(6), f(7), f(8), f(9), None,
            f(10), ws, None))
    calls["eval_relative_pose_ransac"] = (
        lib.gfc_eval_relative_pose_ransac_workspace_bytes(2, 100, 3, 512), lambda ws: lib.gfc_eval_relative_pose_ransac(
            f(1), f(2), f(3), None, f(4), 0, f(5), 0, None, 2, 100, 100, th, 3, 512, 3, 0, 0.0, f(6), f(7), f(8), f(9),
            f(10), f(11), f(12), f(13), f(14), None, None, f(15), ws, None))
    calls["nn_match"] = (lib.gfc_nn_workspace_bytes(B, M, N), lambda ws: lib.gfc_nn_match(
        f(1), f(2), B, M, N, 64, 0.8, 0.0, 1, f(3), f(4), f(5), f(6), f(7), f(8), f(9), ws, None))
    # the two without a size export: the sizes include/gfc_amd.h documents
    calls["lg_log_assignment"] = (2 * B * (M + N) * 4, lambda ws: lib.gfc_lg_log_assignment(
        f(1), f(2), f(3), B, M, N, f(4), f(5), ws, None))
    calls["lg_filter_matches"] = (B * (M + N) * 8, lambda ws: lib.gfc_lg_filter_matches(
        f(1), B, M, N, 0.1, f(2), f(3), f(4), f(5), f(6), ws, None))
    calls["gt_matches_sparse_map"] = (
        lib.gfc_gt_matches_sparse_map_workspace_bytes(B, M, N), lambda ws: lib.gfc_gt_matches_sparse_map(
            f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), f(10), None, None, f(11), B, M, N, 3.0, 5.0, 5.0, f(12),
            f(13), None, None, None, None, None, None, f(14), ws, None))
    calls["gt_matches_roma"] = (
        lib.gfc_gt_matches_roma_workspace_bytes(B, M, N), lambda ws: lib.gfc_gt_matches_roma(
            f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), f(10), B, M, N, 3.0, 5.0, 0.05, 2.0, 5e-4, 20.0, f(11),
            f(12), f(13), f(14), None, None, None, None, f(15), ws, None))
    step = _lg_params()
    calls["lg_adaptive_step"] = (lib.gfc_lg_adaptive_step_workspace_bytes(B, R), lambda ws: lib.gfc_lg_adaptive_step(
        ctypes.byref(step), 0, f(1), f(2), f(3), f(4), R, f(5), f(6), f(7), B, B, N, 0.9, 0.05, 0.95, 1, 1,
        f(8), f(9), f(10), f(11), f(12), 4 * R, f(13), f(14), f(15), f(16), f(17), f(18), ws, None))
    m, n = (ctypes.c_int32 * 3)(65, 65, 40), (ctypes.c_int32 * 3)(130, 130, 17)
    for tag, prec in (("fp32", nat.GFC_LG_FP32), ("fp16", nat.GFC_LG_FP16)):
        p = _lg_params(prec)
        calls[f"lg_layer_{tag}"] = (lib.gfc_lg_layer_workspace_bytes(R), lambda ws, p=p: lib.gfc_lg_layer(
            ctypes.byref(p), 1, f(1), f(2), f(3), R, f(4), f(5), 2 * B, N, f(6), ws, None))
        calls[f"lg_assign_{tag}"] = (lib.gfc_lg_assign_workspace_bytes(B, M, N), lambda ws, p=p: lib.gfc_lg_assign(
            ctypes.byref(p), 1, f(1), f(2), B, M, N, 0.1, f(3), f(4), f(5), f(6), f(7), f(8), ws, None))
        calls[f"lg_forward_{tag}"] = (lib.gfc_lg_workspace_bytes(B, M, N), lambda ws, p=p: lib.gfc_lg_forward(
            ctypes.byref(p), f(1), f(12), f(2), f(13), f(3), f(4), None, None, B, M, N, 0.1, f(5), f(6), f(7), f(8), f(9),
            None, None, f(11), ws, None))
        calls[f"lg_forward_packed_{tag}"] = (
            lib.gfc_lg_packed_workspace_bytes(B, M, N), lambda ws, p=p: lib.gfc_lg_forward_packed(
                ctypes.byref(p), f(1), f(2), f(3), f(4), None, B, M, N, 0.1, f(5), f(6), f(7), f(8), f(9), f(10), f(11), ws,
                None, None))
        calls[f"lg_forward_ragged_{tag}"] = (
            lib.gfc_lg_ragged_workspace_bytes(3, m, n), lambda ws, p=p: lib.gfc_lg_forward_ragged(
                ctypes.byref(p), f(1), f(2), f(3), f(4), None, 3, m, n, 0.1, f(5), f(6), f(7), f(8), f(9), f(10), f(11), ws,
                None, None))
    return calls


_SHORT = ["sp_dense_c1", "sp_dense_c3", "sp_select", "sp_nms_select", "disk_nms_select", "disk_instnorm_stats",
          "eval_homography_ransac", "eval_relative_pose_ransac", "nn_match", "lg_log_assignment", "lg_filter_matches", "lg_adaptive_step",
          "gt_matches_sparse_map", "gt_matches_roma"] + [
    f"lg_{e}_{t}" for t in ("fp32", "fp16") for e in ("layer", "assign", "forward", "forward_packed", "forward_ragged")]


@pytest.mark.parametrize("name", _SHORT)
def test_one_byte_short_is_refused_before_any_launch(name):
    calls = _short_calls()
    assert sorted(calls) == sorted(_SHORT)
    need, call = calls[name]
    assert need > 1
    assert call(need - 1) == WORKSPACE
    assert call(0) == WORKSPACE


def test_lg_forward_refuses_descriptors_that_do_not_fit_the_staging_slot():
    """A model with an input projection whose two descriptor arrays are not adjacent has them packed into the layer
    scratch: 7168 bytes per row, plus the attention key-split scratch up to 8192 rows.  Beyond 8192 rows input_dim = 2048
    (8192 bytes per row) does not fit, which is an argument error, answered before the workspace is looked at."""
    lib = nat.lib()
    b, m, n = 2, 2100, 2100  # 8400 rows
    for prec in (nat.GFC_LG_FP32, nat.GFC_LG_FP16):
        p = _lg_params(prec, input_dim=2048)

        def call(desc1, ws, b=b, m=m, n=n, p=p):
            return lib.gfc_lg_forward(ctypes.byref(p), f(1), f(12), f(2), desc1, f(3), f(4), None, None, b, m, n, 0.1,
                                      f(5), f(6), f(7), f(8), f(9), None, None, f(11), ws, None)

        need = lib.gfc_lg_workspace_bytes(b, m, n)
        assert call(f(13), need - 1) == INVALID and call(f(13), 0) == INVALID
        # adjacent arrays are read in place: nothing is staged, and the short workspace is what is refused
        adjacent = ctypes.c_void_p(0x2000 + b * m * 2048 * 4)
        assert call(adjacent, need - 1) == WORKSPACE
        # with the key-split scratch (rows <= 8192) the same descriptors fit
        assert call(f(13), lib.gfc_lg_workspace_bytes(B, M, N) - 1, B, M, N) == WORKSPACE
        # input_dim = 1792 is the largest that fits at any row count
        p.input_dim = 1792
        assert call(f(13), need - 1) == WORKSPACE
