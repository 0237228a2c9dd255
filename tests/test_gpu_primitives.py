"""GPU parity of every exported kernel in isolation (through the C ABI), against the oracle /
plain torch fp32 on the same seeded inputs.  Integer / index outputs bit-exact; floating point
within 1e-4 (north-star tolerance), in practice ~1e-6."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from glue_factory_colon_amd import _native as nat  # noqa: E402
from oracle import lightglue as olg  # noqa: E402
from oracle import superpoint as osp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
_KEEP = []


def D(t):
    """Move to the device and keep the tensor alive until the end of the test: the library gets
    raw pointers, so a temporary `.to(DEV)` would be freed (and its block reused) too early."""
    if t is None:
        return None
    t = t.to(DEV).contiguous()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return nat.stream_ptr(torch.device(DEV))


def maxerr(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------- conv3x3
@pytest.mark.parametrize("cin,cout,h,w,pool,bn", [(64, 64, 32, 48, True, True), (64, 128, 30, 40, False, True),
                                                   (128, 128, 17, 23, True, False), (128, 512, 15, 20, False, True),
                                                   (1, 64, 21, 35, False, True), (64, 64, 33, 47, True, True)])
def test_conv3x3(cin, cout, h, w, pool, bn):
    lib = nat.lib()
    g = gen(cin + cout + h)
    b = 2
    x = torch.randn((b, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin ** 0.5)
    bias = torch.randn((cout,), generator=g) * 0.1
    scale = torch.rand((cout,), generator=g) + 0.5 if bn else None
    shift = torch.randn((cout,), generator=g) * 0.1 if bn else None
    scale_neg = scale
    if bn:
        scale_neg = scale.clone()
        scale_neg[::3] *= -1  # negative BN gains: pooling must come after the affine
    ref = F.relu(F.conv2d(x, wt, bias, padding=1))
    if bn:
        ref = ref * scale_neg[None, :, None, None] + shift[None, :, None, None]
    if pool:
        ref = F.max_pool2d(ref, 2, 2)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = wt.to(DEV).contiguous()
    wp = torch.empty((9, cout, cin), device=DEV)
    nat.check(lib.gfc_pack_conv3x3(nat.ptr(wd), nat.ptr(wp), cout, cin, st()), "pack")
    assert torch.equal(wp.cpu(), wt.permute(2, 3, 0, 1).reshape(9, cout, cin))
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    y = torch.full((b, ho, wo, cout), float("nan"), device=DEV)
    nat.check(lib.gfc_conv3x3(nat.ptr(xd), nat.ptr(wp), nat.ptr(D(bias)),
                              nat.ptr(D(scale_neg)) if bn else None, nat.ptr(D(shift)) if bn else None,
                              nat.ptr(y), b, h, w, cin, cout, 1, int(pool), st()), "conv")
    torch.cuda.synchronize()
    assert maxerr(y.permute(0, 3, 1, 2), ref) < 2e-5


@pytest.mark.parametrize("h,w,bn", [(48, 64, True), (37, 51, True), (32, 32, False)])
def test_stem_fused_conv1a_conv1b_pool(h, w, bn):
    lib = nat.lib()
    g = gen(h * w)
    b = 2
    img = torch.rand((b, 1, h, w), generator=g)
    w1 = torch.randn((64, 1, 3, 3), generator=g) / 3
    b1 = torch.randn((64,), generator=g) * 0.1
    w2 = torch.randn((64, 64, 3, 3), generator=g) / 24
    b2 = torch.randn((64,), generator=g) * 0.1
    s1 = s2 = t1 = t2 = None
    ref = F.relu(F.conv2d(img, w1, b1, padding=1))
    if bn:
        s1, t1 = torch.rand((64,), generator=g) + 0.5, torch.randn((64,), generator=g) * 0.1
        s2, t2 = torch.rand((64,), generator=g) + 0.5, torch.randn((64,), generator=g) * 0.1
        s2[::5] *= -1
        ref = ref * s1[None, :, None, None] + t1[None, :, None, None]
    ref = F.relu(F.conv2d(ref, w2, b2, padding=1))
    if bn:
        ref = ref * s2[None, :, None, None] + t2[None, :, None, None]
    ref = F.max_pool2d(ref, 2, 2)
    w2p = torch.empty((9, 64, 64), device=DEV)
    nat.check(lib.gfc_pack_conv3x3(nat.ptr(D(w2)), nat.ptr(w2p), 64, 64, st()), "pack")
    w1p = D(w1.reshape(64, 9).t().contiguous())  # [9][64]
    y = torch.full((b, h // 2, w // 2, 64), float("nan"), device=DEV)
    nat.check(lib.gfc_sp_stem(nat.ptr(D(img.reshape(b, h, w))), nat.ptr(w1p), nat.ptr(D(b1)), nat.ptr(D(s1)),
                              nat.ptr(D(t1)), nat.ptr(w2p), nat.ptr(D(b2)), nat.ptr(D(s2)), nat.ptr(D(t2)), nat.ptr(y),
                              b, h, w, st()), "stem")
    torch.cuda.synchronize()
    assert maxerr(y.permute(0, 3, 1, 2), ref) < 2e-5


@pytest.mark.parametrize("cin,cout,pool", [(64, 128, False), (64, 64, True), (128, 64, False)])
def test_conv3x3_many_items_persistent_handover(cin, cout, pool):
    """More work items than resident workgroups (512: two per CU): the un-pooled layers (630 and 1260 items) run
    persistent workgroups that hand over from item to item with the next halo tile / weight slice prefetched; the
    pooled layer runs one workgroup per item.  Partial border tiles included.  Checked against torch."""
    lib = nat.lib()
    g = gen(cin * 3 + cout)
    b, h, w = 9, 104, 152   # 7 x 10 tiles x 9 images x (cout/64) blocks = 630 / 1260 items
    x = torch.randn((b, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin ** 0.5)
    bias = torch.randn((cout,), generator=g) * 0.1
    scale = torch.rand((cout,), generator=g) + 0.5
    shift = torch.randn((cout,), generator=g) * 0.1
    ref = F.relu(F.conv2d(x, wt, bias, padding=1)) * scale[None, :, None, None] + shift[None, :, None, None]
    if pool:
        ref = F.max_pool2d(ref, 2, 2)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wp = torch.empty((9, cout, cin), device=DEV)
    nat.check(lib.gfc_pack_conv3x3(nat.ptr(D(wt)), nat.ptr(wp), cout, cin, st()), "pack")
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    y = torch.full((b, ho, wo, cout), float("nan"), device=DEV)
    nat.check(lib.gfc_conv3x3(nat.ptr(xd), nat.ptr(wp), nat.ptr(D(bias)), nat.ptr(D(scale)), nat.ptr(D(shift)),
                              nat.ptr(y), b, h, w, cin, cout, 1, int(pool), st()), "conv")
    torch.cuda.synchronize()
    assert maxerr(y.permute(0, 3, 1, 2), ref) < 2e-5


def test_abi_status_codes_for_bad_arguments():
    """The C ABI reports misuse through gfc_status, never by faulting: a sweep over the entry points."""
    lib = nat.lib()
    x = torch.zeros(4096, device=DEV)
    xi = torch.zeros(64, device=DEV, dtype=torch.int32)
    xl = torch.zeros(64, device=DEV, dtype=torch.long)
    P, s_ = nat.ptr, st()
    INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 3
    assert lib.gfc_linear(P(x), 250, 256, None, 0, 0, P(x), 256, None, None, None, 1.0, None, None, None, 0, P(x), 8, 4, 8,
                          s_) == INVALID                                    # lda not a multiple of 4
    assert lib.gfc_linear(P(x), 256, 250, None, 0, 0, P(x), 256, None, None, None, 1.0, None, None, None, 0, P(x), 8, 4, 8,
                          s_) == INVALID                                    # K not a multiple of 32
    assert lib.gfc_linear(P(x), 256, 256, None, 0, 0, P(x), 256, None, P(x), None, 1.0, None, None, None, 0, P(x), 8, 4, 8,
                          s_) == INVALID                                    # scale without shift
    assert lib.gfc_batched_nt(P(x), 64, 0, P(x), 64, 0, P(x), 8, 0, 4, 8, 48, 1, s_) == INVALID
    assert lib.gfc_attention(P(x), 64, P(x), 64, P(x), 64, P(x), 64, P(xi), 0, 64, 1, 0.125, None, 0, s_) == INVALID
    assert lib.gfc_layernorm_gelu(None, 512, 4, 512, P(x), P(x), s_) == INVALID
    assert lib.gfc_sp_nms(P(x), 1, 8, 8, 2, 0, None, None, s_) == INVALID
    assert lib.gfc_sp_nms(P(x), 1, 8, 8, 7, 0, None, P(x), s_) == UNSUPPORTED  # radius beyond the LDS halo
    assert lib.gfc_sp_select(P(x), 1, 8, 8, 0.0, 4, 2, P(x), P(x), P(xi), P(x), 1 << 20, s_) == INVALID   # cap < k
    assert lib.gfc_sp_select(P(x), 1, 8, 8, 0.0, 4, 4, P(x), P(x), P(xi), P(x), 8, s_) == WORKSPACE
    assert lib.gfc_sp_nms_select(P(x), 1, 16, 16, 0, 0, None, 0.0, 4, 4, None, P(x), P(x), P(xi), P(x), 1 << 20,
                                 s_) == UNSUPPORTED                         # radius 0: two-stage path
    assert lib.gfc_sp_nms_select(P(x), 1, 16, 16, 3, 0, None, 0.0, 9000, 9000, None, P(x), P(x), P(xi), P(x), 1 << 20,
                                 s_) == UNSUPPORTED                         # k > 8192
    assert lib.gfc_sp_sample(P(x), 1, 2, 2, 256, None, None, 4, 0, P(x), P(x), s_) == INVALID
    assert lib.gfc_sp_refine_keypoints(P(x), 1, 8, 8, P(x), None, 4, 0, s_) == INVALID         # radius < 1
    assert lib.gfc_sp_mask_scores(P(x), 1, 8, 8, None, 8, 8, None, s_) == INVALID
    assert lib.gfc_sp_filter_keypoints(P(x), P(x), P(xi), 1, 0, P(x), 8, 8, None, 0.0, s_) == INVALID
    assert lib.gfc_lg_posenc(P(x), None, P(x), P(xi), P(xi), 1, 4, P(x), 4, P(x), P(x), s_) == INVALID  # dim 4 w/o scale_ori
    assert lib.gfc_lg_posenc(P(x), P(x), P(x), P(xi), P(xi), 1, 4, P(x), 2, P(x), P(x), s_) == INVALID  # dim 2 with it
    assert lib.gfc_lg_posenc(P(x), None, P(x), P(xi), P(xi), 1, 4, P(x), 3, P(x), P(x), s_) == INVALID
    assert lib.gfc_lg_filter_matches(P(x), 1, 4, 4, 0.1, P(xl), P(xl), P(x), P(x), P(x), 4, s_) == WORKSPACE
    assert lib.gfc_nn_match(P(x), P(x), 1, 4, 4, 64, 0.0, 0.0, 1, P(xl), P(xl), P(x), P(x), None, None, P(x), 4,
                            s_) in (INVALID, WORKSPACE)
    assert lib.gfc_eval_matches_homography(P(x), P(x), P(xl), P(x), None, 1, 4, 4, 3.0, 3.0, P(x), None, s_) == INVALID
    assert lib.gfc_eval_homography_dlt(P(x), P(x), P(xl), P(x), P(x), P(x), 0, 4, 4, P(x), P(x), s_) == INVALID
    assert lib.gfc_preprocess_resize(P(x), 0, 0, 1, 1, 8, 8, P(x), 0, 4, 0, 1, s_) == INVALID
    assert lib.gfc_preprocess_resize(P(x), 0, 0, 1, 1, 4096, 8, P(x), 16, 8, 0, 1, s_) == UNSUPPORTED  # 256x down-scale
    torch.cuda.synchronize()  # nothing was launched, nothing faulted


@pytest.mark.parametrize("cin,cout,h,w,pool,bn", [(64, 64, 32, 48, True, True), (64, 128, 30, 40, False, True),
                                                   (128, 128, 17, 23, True, False), (128, 512, 15, 20, False, True),
                                                   (64, 64, 33, 47, True, True), (16, 64, 5, 3, False, False),
                                                   (128, 128, 60, 80, False, True), (64, 64, 240, 320, True, True),
                                                   (64, 128, 104, 152, False, True)])  # 780 items: persistent, 780 % 8 != 0
def test_conv3x3_winograd(cin, cout, h, w, pool, bn):
    """gfc_conv3x3_wino (Winograd F(2x2,3x3), fp32 MFMA, filters transformed in float64 at pack time) against a
    float64 convolution: the error must be of the order of the direct fp32-MFMA kernel's (both ~1e-6 here)."""
    lib = nat.lib()
    g = gen(cin + cout + h + 1)
    b = 3
    x = torch.randn((b, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin ** 0.5)
    bias = torch.randn((cout,), generator=g) * 0.1
    scale = torch.rand((cout,), generator=g) + 0.5 if bn else None
    shift = torch.randn((cout,), generator=g) * 0.1 if bn else None
    if bn:
        scale[::3] *= -1  # negative BN gains: pooling must come after the affine
    ref = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), padding=1))
    if bn:
        ref = ref * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    if pool:
        ref = F.max_pool2d(ref, 2, 2)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    errs = {}
    for name in ("direct", "winograd"):
        y = torch.full((b, ho, wo, cout), float("nan"), device=DEV)
        if name == "direct":
            if cin % 32:
                continue
            wp = torch.empty((9, cout, cin), device=DEV)
            nat.check(lib.gfc_pack_conv3x3(nat.ptr(D(wt)), nat.ptr(wp), cout, cin, st()), "pack")
            nat.check(lib.gfc_conv3x3(nat.ptr(xd), nat.ptr(wp), nat.ptr(D(bias)), nat.ptr(D(scale)), nat.ptr(D(shift)),
                                      nat.ptr(y), b, h, w, cin, cout, 1, int(pool), st()), "conv")
        else:
            ww = torch.empty((16 * cout * cin,), device=DEV)
            nat.check(lib.gfc_pack_conv3x3_wino(nat.ptr(D(wt)), nat.ptr(ww), cout, cin, st()), "pack_wino")
            nat.check(lib.gfc_conv3x3_wino(nat.ptr(xd), nat.ptr(ww), nat.ptr(D(bias)), nat.ptr(D(scale)),
                                           nat.ptr(D(shift)), nat.ptr(y), b, h, w, cin, cout, 1, int(pool), st()),
                      "conv_wino")
        torch.cuda.synchronize()
        errs[name] = (y.permute(0, 3, 1, 2).double().cpu() - ref).abs().max().item()
    assert errs["winograd"] < 2e-5, errs
    if "direct" in errs:
        assert errs["winograd"] < 3 * errs["direct"] + 1e-6, errs
    from parity_utils import record
    record(f"conv_wino_err_{cin}_{cout}_{h}x{w}_{'pool' if pool else 'nopool'}", winograd_max_abs_err=errs["winograd"],
           direct_fp32_mfma_max_abs_err=errs.get("direct", -1.0))


@pytest.mark.parametrize("variant", ["f23", "f43"])
@pytest.mark.parametrize("h,w,bn,b", [(48, 64, True, 2), (37, 51, True, 2), (32, 32, False, 2), (480, 640, True, 2),
                                      (2, 2, True, 1), (16, 33, False, 3), (100, 200, True, 20)])
def test_stem_winograd(h, w, bn, b, variant):
    """gfc_sp_stem_wino (conv1a direct on the halo patch + conv1b Winograd F(2x2,3x3) + pool) and gfc_sp_stem_wino43
    (conv1a on the matrix pipe + conv1b Winograd F(4x4,3x3) + pool; persistent workgroups: the b = 20 case gives every
    workgroup several items) against float64 torch.  superpoint_open.py:61-77,100-108."""
    lib = nat.lib()
    g = gen(h * w + 3)
    img = torch.rand((b, 1, h, w), generator=g)
    w1 = torch.randn((64, 1, 3, 3), generator=g) / 3
    b1 = torch.randn((64,), generator=g) * 0.1
    w2 = torch.randn((64, 64, 3, 3), generator=g) / 24
    b2 = torch.randn((64,), generator=g) * 0.1
    s1 = s2 = t1 = t2 = None
    ref = F.relu(F.conv2d(img.double(), w1.double(), b1.double(), padding=1))
    if bn:
        s1, t1 = torch.rand((64,), generator=g) + 0.5, torch.randn((64,), generator=g) * 0.1
        s2, t2 = torch.rand((64,), generator=g) + 0.5, torch.randn((64,), generator=g) * 0.1
        s2[::5] *= -1
        ref = ref * s1.double()[None, :, None, None] + t1.double()[None, :, None, None]
    ref = F.relu(F.conv2d(ref, w2.double(), b2.double(), padding=1))
    if bn:
        ref = ref * s2.double()[None, :, None, None] + t2.double()[None, :, None, None]
    ref = F.max_pool2d(ref, 2, 2)
    w1p = D(w1.reshape(64, 9).t().contiguous())  # [9][64]
    y = torch.full((b, h // 2, w // 2, 64), float("nan"), device=DEV)
    if variant == "f23":
        w2w = torch.empty((16 * 64 * 64,), device=DEV)
        nat.check(lib.gfc_pack_conv3x3_wino(nat.ptr(D(w2)), nat.ptr(w2w), 64, 64, st()), "pack_wino")
        fn = lib.gfc_sp_stem_wino
    else:
        w2w = torch.empty((36 * 64 * 64,), device=DEV)
        nat.check(lib.gfc_pack_conv3x3_wino43(nat.ptr(D(w2)), nat.ptr(w2w), 64, 64, st()), "pack_wino43")
        fn = lib.gfc_sp_stem_wino43
    nat.check(fn(nat.ptr(D(img.reshape(b, h, w))), nat.ptr(w1p), nat.ptr(D(b1)), nat.ptr(D(s1)), nat.ptr(D(t1)),
                 nat.ptr(w2w), nat.ptr(D(b2)), nat.ptr(D(s2)), nat.ptr(D(t2)), nat.ptr(y), b, h, w, st()), "stem")
    torch.cuda.synchronize()
    from parity_utils import record
    err = (y.permute(0, 3, 1, 2).double().cpu() - ref).abs().max().item()
    record(f"stem_{variant}_err_{h}x{w}_b{b}", err=err)
    # direct fp32: ~1.5e-6 on this data; F(2x2,3x3) the same; F(4x4,3x3) a few times that (larger transform constants)
    assert err < (2e-5 if variant == "f23" else 4e-5), err


def test_conv3x3_rejects_bad_shapes():
    lib = nat.lib()
    x = torch.zeros(16, device=DEV)
    assert lib.gfc_conv3x3(nat.ptr(x), nat.ptr(x), nat.ptr(x), None, None, nat.ptr(x), 1, 8, 8, 48, 64, 1, 0, st()) == 3
    assert lib.gfc_conv3x3(None, nat.ptr(x), nat.ptr(x), None, None, nat.ptr(x), 1, 8, 8, 64, 64, 1, 0, st()) == 1


# -------------------------------------------------------------------------------- linear
def run_linear(a0, w, bias=None, a1=None, scale=None, shift=None, alpha=1.0, residual=None, cos=None, sin=None,
               rot_cols=0, ldy=None):
    lib = nat.lib()
    m, n = a0.shape[0], w.shape[0]
    ldy = ldy or n
    y = torch.full((m, ldy), float("nan"), device=DEV)
    d = D
    a0d, a1d, wd, bd, scd, shd, rd, cd, sd = map(d, (a0, a1, w, bias, scale, shift, residual, cos, sin))
    if rd is not None:
        y[:, :n] = rd
        rd = y
    nat.check(lib.gfc_linear(nat.ptr(a0d), a0.shape[1], a0.shape[1], nat.ptr(a1d), 0 if a1 is None else a1.shape[1],
                             0 if a1 is None else a1.shape[1], nat.ptr(wd), w.shape[1], nat.ptr(bd), nat.ptr(scd),
                             nat.ptr(shd), alpha, nat.ptr(rd), nat.ptr(cd), nat.ptr(sd), rot_cols, nat.ptr(y), ldy, m,
                             n, st()), "linear")
    torch.cuda.synchronize()
    return y[:, :n].cpu()


@pytest.mark.parametrize("m,n,k", [(300, 256, 256), (129, 65, 256), (1000, 768, 256), (64, 512, 512), (5, 256, 128)])
def test_linear_plain(m, n, k):
    g = gen(m + n)
    a = torch.randn((m, k), generator=g)
    w = torch.randn((n, k), generator=g) / k ** 0.5
    b = torch.randn((n,), generator=g)
    assert maxerr(run_linear(a, w, b), F.linear(a, w, b)) < 2e-5
    assert maxerr(run_linear(a, w, b, alpha=0.25), F.linear(a, w, b) / 4) < 1e-5


def test_gemm_tile_variants_via_knob():
    """Both GEMM tiles of the library (GFC_GEMM_TILE = 4: 128x128 with a 16-deep K tile, 3: 64x64 with a 32-deep one),
    each forced for EVERY problem size, pass the linear / batched tests (by default the size decides); the knob is read
    once per process, hence child processes.  The other variants of rounds 2-5 were removed in round 6."""
    import subprocess
    import sys

    # 4 = gemm_nt_kernel<2,2,16>, the variant large batches (bench.py: 32 pairs) dispatch to by default
    for tile in (3, 4):
        env = dict(os.environ, GFC_GEMM_TILE=str(tile))
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                            "-k", "(linear_plain or linear_concat or linear_rotary or batched_nt) and not via_knob", "-p", "no:cacheprovider"],
                           capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (tile, r.stdout[-800:], r.stderr[-400:])


def test_mfma_peak_probe():
    """bench-only gfc_probe_mfma_peak: a plausible fp32-MFMA rate and shader clock for an MI355X."""
    import ctypes

    tf, ghz = ctypes.c_float(0), ctypes.c_float(0)
    nat.check(nat.lib().gfc_probe_mfma_peak(20000, ctypes.byref(tf), ctypes.byref(ghz), st()), "probe")
    assert 60.0 < tf.value < 165.0 and 1.0 < ghz.value < 2.6, (tf.value, ghz.value)
    assert nat.lib().gfc_probe_mfma_peak(2, ctypes.byref(tf), ctypes.byref(ghz), st()) != 0  # GFC_ERR_INVALID


def test_attention_variants_via_knob():
    """attention_kernel<2> (GFC_ATTN_CFG=1: two 32-query tiles per wave, 256 queries per workgroup -- what a
    32-pair batch dispatches to) on the ragged shapes of test_attention (n_q not a multiple of 256, n_q != n_kv,
    query tails) and on the spiked-key case; the knob is read once per process."""
    import subprocess
    import sys

    for cfg in (1,):
        env = dict(os.environ, GFC_ATTN_CFG=str(cfg))
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                            "-k", "((test_attention and not split and not variants and not natural) or cross_attention) and not via_knob",
                            "-p", "no:cacheprovider"],
                           capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (cfg, r.stdout[-800:], r.stderr[-400:])


def test_linear_concat_residual_affine():
    g = gen(5)
    m = 333
    x, msg = torch.randn((m, 256), generator=g), torch.randn((m, 256), generator=g)
    w = torch.randn((512, 512), generator=g) / 512 ** 0.5
    b = torch.randn((512,), generator=g)
    ref = F.linear(torch.cat([x, msg], -1), w, b)
    assert maxerr(run_linear(x, w, b, a1=msg), ref) < 2e-5
    w3 = torch.randn((256, 512), generator=g) / 512 ** 0.5
    h = torch.randn((m, 512), generator=g)
    assert maxerr(run_linear(h, w3, b[:256], residual=x), x + F.linear(h, w3, b[:256])) < 2e-5
    sc, sh = torch.rand((256,), generator=g) + 0.5, torch.randn((256,), generator=g)
    assert maxerr(run_linear(x, w3[:, :256].contiguous(), b[:256], scale=sc, shift=sh),
                  F.linear(x, w3[:, :256], b[:256]) * sc + sh) < 2e-5
    # non-multiple-of-4 output stride (the 65-logit detector head)
    w65 = torch.randn((65, 256), generator=g) / 16
    assert maxerr(run_linear(x, w65, b[:65], ldy=65), F.linear(x, w65, b[:65])) < 2e-5


def test_linear_rotary():
    g = gen(9)
    m = 200
    x = torch.randn((m, 256), generator=g)
    w = torch.randn((768, 256), generator=g) / 16
    b = torch.randn((768,), generator=g) * 0.1
    ang = torch.randn((m, 32), generator=g) * 2
    cos = ang.cos().repeat_interleave(2, -1)
    sin = ang.sin().repeat_interleave(2, -1)
    y = F.linear(x, w, b)
    qk = y[:, :512].view(m, 8, 64)
    enc = torch.stack([cos, sin], 0)[:, :, None]  # [2, m, 1, 64]
    ref = torch.cat([olg.rotary(enc, qk).reshape(m, 512), y[:, 512:]], -1)
    out = run_linear(x, w, b, cos=cos, sin=sin, rot_cols=512)
    assert maxerr(out, ref) < 2e-5


def test_batched_nt():
    lib = nat.lib()
    g = gen(3)
    b, m, n, k = 3, 150, 97, 256
    a = torch.randn((b, m, k), generator=g).to(DEV)
    c = torch.randn((b, n, k), generator=g).to(DEV)
    y = torch.full((b, m + 1, n + 1), 7.0, device=DEV)
    nat.check(lib.gfc_batched_nt(nat.ptr(a), k, m * k, nat.ptr(c), k, n * k, nat.ptr(y), n + 1, (m + 1) * (n + 1), m,
                                 n, k, b, st()), "batched_nt")
    torch.cuda.synchronize()
    ref = torch.einsum("bmd,bnd->bmn", a.cpu(), c.cpu())
    assert maxerr(y[:, :m, :n], ref) < 5e-5
    assert (y[:, m, :] == 7).all() and (y[:, :, n] == 7).all()  # border untouched


def _ref64(fn, *tensors):
    """Reference in float64 on the device (plain torch; rocBLAS dgemm), result rounded to fp32 on the host."""
    with torch.no_grad():
        return fn(*[t.to(DEV).double() for t in tensors]).float().cpu()


@pytest.mark.parametrize("n,k,epilogue", [(768, 256, "rotary"), (512, 256, "plain"), (512, 512, "concat"),
                                          (256, 512, "residual"), (256, 256, "alpha")])
@pytest.mark.parametrize("m", [65536, 65536 - 37])
def test_linear_natural_dispatch_batch32_shapes(m, n, k, epilogue):
    """The GEMMs of a 32-pair LightGlue layer at their real size (M = 32 * 2 * 1024 rows; also a ragged M): no
    knob, so launch_gemm picks gemm_nt_kernel<2,2,16> itself (tiles(128,128) >= 768) -- the variant bench.py
    times.  Every epilogue the layer uses, against float64."""
    g = gen(m + n + k)
    w = torch.randn((n, k), generator=g) / k ** 0.5
    b = torch.randn((n,), generator=g) * 0.3
    if epilogue == "concat":
        a0, a1 = torch.randn((m, k // 2), generator=g), torch.randn((m, k // 2), generator=g)
        out = run_linear(a0, w, b, a1=a1)
        ref = _ref64(lambda x, y, ww, bb: F.linear(torch.cat([x, y], 1), ww, bb), a0, a1, w, b)
    else:
        a = torch.randn((m, k), generator=g)
        if epilogue == "rotary":
            ang = torch.randn((m, 32), generator=g) * 2
            cos, sin = ang.cos().repeat_interleave(2, -1), ang.sin().repeat_interleave(2, -1)
            out = run_linear(a, w, b, cos=cos, sin=sin, rot_cols=512)

            def rot(x, ww, bb, c, s_):
                y = F.linear(x, ww, bb)
                t = y[:, :512].reshape(m, 8, 32, 2)
                r = torch.stack([-t[..., 1], t[..., 0]], -1).reshape(m, 8, 64)
                qk = y[:, :512].reshape(m, 8, 64) * c[:, None] + r * s_[:, None]
                return torch.cat([qk.reshape(m, 512), y[:, 512:]], 1)
            ref = _ref64(rot, a, w, b, cos, sin)
        elif epilogue == "residual":
            res = torch.randn((m, n), generator=g)
            out = run_linear(a, w, b, residual=res)
            ref = _ref64(lambda x, ww, bb, r: r + F.linear(x, ww, bb), a, w, b, res)
        elif epilogue == "alpha":
            out = run_linear(a, w, b, alpha=0.25)
            ref = _ref64(lambda x, ww, bb: F.linear(x, ww, bb) * 0.25, a, w, b)
        else:
            out = run_linear(a, w, b)
            ref = _ref64(lambda x, ww, bb: F.linear(x, ww, bb), a, w, b)
    assert maxerr(out, ref) < 2e-5


@pytest.mark.parametrize("m", [65536, 16384 + 77, 100])
def test_linear_layernorm_gelu_fused(m):
    """gfc_linear_layernorm_gelu (row-owning 128 x 512 tiles: ffn[0] -> LayerNorm -> GELU of lightglue.py:143-148 in one
    kernel, two-source A) against float64 torch: F.linear -> layer_norm(eps 1e-5) -> gelu(erf)."""
    lib = nat.lib()
    g = gen(m)
    x, msg = torch.randn((m, 256), generator=g), torch.randn((m, 256), generator=g) * 2 + 0.3
    w = torch.randn((512, 512), generator=g) / 512 ** 0.5
    b = torch.randn((512,), generator=g)
    gamma, beta = torch.rand((512,), generator=g) + 0.5, torch.randn((512,), generator=g) * 0.2
    y = torch.full((m, 512), float("nan"), device=DEV)
    nat.check(lib.gfc_linear_layernorm_gelu(nat.ptr(D(x)), 256, 256, nat.ptr(D(msg)), 256, 256, nat.ptr(D(w)), 512,
                                            nat.ptr(D(b)), nat.ptr(D(gamma)), nat.ptr(D(beta)), nat.ptr(y), 512, m, 512,
                                            st()), "linear_ln_gelu")
    torch.cuda.synchronize()
    ref = _ref64(lambda a, c, ww, bb, ga, be: F.gelu(F.layer_norm(F.linear(torch.cat([a, c], 1), ww, bb), (512,), ga, be,
                                                                     1e-5)), x, msg, w, b, gamma, beta)
    assert maxerr(y, ref) < 2e-5
    # the unfused pair of kernels agrees to rounding
    h = run_linear(x, w, b, a1=msg).to(DEV)
    nat.check(lib.gfc_layernorm_gelu(nat.ptr(h), 512, m, 512, nat.ptr(D(gamma)), nat.ptr(D(beta)), st()), "ln")
    assert maxerr(y, h) < 1e-5
    assert lib.gfc_linear_layernorm_gelu(nat.ptr(D(x)), 256, 256, None, 0, 0, nat.ptr(D(w)), 512, nat.ptr(D(b)),
                                         nat.ptr(D(gamma)), nat.ptr(D(beta)), nat.ptr(y), 256, m, 256, st()) == 3


@pytest.mark.parametrize("m", [65536, 16384 + 77, 100])
def test_ffn_fused_whole_mlp(m):
    """gfc_ffn_fused: the whole LightGlue FFN with its residual in ONE kernel -- Linear(512,512) -> LayerNorm -> GELU ->
    Linear(512,256), + x (lightglue.py:143-148,162-164) -- against float64 torch, bit-identical to the two-kernel path
    (gfc_linear_layernorm_gelu, then gfc_linear with the residual epilogue), in place (Y = residual = A0) as the cross
    block uses it, and row-batch invariant (a row's result does not depend on which other rows share its launch)."""
    lib = nat.lib()
    g = gen(m + 1)
    x, msg = torch.randn((m, 256), generator=g), torch.randn((m, 256), generator=g) * 2 + 0.3
    w0 = torch.randn((512, 512), generator=g) / 512 ** 0.5
    b0 = torch.randn((512,), generator=g)
    gamma, beta = torch.rand((512,), generator=g) + 0.5, torch.randn((512,), generator=g) * 0.2
    w3 = torch.randn((256, 512), generator=g) / 512 ** 0.5
    b3 = torch.randn((256,), generator=g)
    dx, dmsg, dw0, db0, dga, dbe, dw3, db3 = (D(t) for t in (x, msg, w0, b0, gamma, beta, w3, b3))

    def fused(a0, resid, y, rows=m, off=0):
        o = off * 256 * 4
        nat.check(lib.gfc_ffn_fused(nat.c_void_p(a0.data_ptr() + o), 256, 256, nat.c_void_p(dmsg.data_ptr() + o), 256, 256,
                                    nat.ptr(dw0), 512, nat.ptr(db0), nat.ptr(dga), nat.ptr(dbe), nat.ptr(dw3), 512,
                                    nat.ptr(db3), None if resid is None else nat.c_void_p(resid.data_ptr() + o),
                                    nat.c_void_p(y.data_ptr() + o), 256, rows, st()), "gfc_ffn_fused")

    y = torch.full((m, 256), float("nan"), device=DEV)
    fused(dx, dx, y)
    torch.cuda.synchronize()
    ref = _ref64(lambda a, c, ww, bb, ga, be, w3_, b3_: a + F.linear(
        F.gelu(F.layer_norm(F.linear(torch.cat([a, c], 1), ww, bb), (512,), ga, be, 1e-5)), w3_, b3_),
        x, msg, w0, b0, gamma, beta, w3, b3)
    assert maxerr(y, ref) < 3e-5
    # the two-kernel path: bit-identical
    hb = torch.empty((m, 512), device=DEV)
    nat.check(lib.gfc_linear_layernorm_gelu(nat.ptr(dx), 256, 256, nat.ptr(dmsg), 256, 256, nat.ptr(dw0), 512, nat.ptr(db0),
                                            nat.ptr(dga), nat.ptr(dbe), nat.ptr(hb), 512, m, 512, st()), "ln_gelu")
    y2 = torch.empty((m, 256), device=DEV)
    nat.check(lib.gfc_linear(nat.ptr(hb), 512, 512, None, 0, 0, nat.ptr(dw3), 512, nat.ptr(db3), None, None, 1.0,
                             nat.ptr(dx), None, None, 0, nat.ptr(y2), 256, m, 256, st()), "ffn3")
    assert torch.equal(y, y2)
    # in place: Y = residual = A0 (the cross block's call)
    xin = dx.clone()
    fused(xin, xin, xin)
    assert torch.equal(xin, y)
    # no residual / rows of a launch are independent: a sub-range of rows alone gives the same rows
    y3 = torch.empty((m, 256), device=DEV)
    fused(dx, None, y3)
    assert maxerr(y3 + dx, y) < 1e-5
    if m > 300:
        sub = torch.full((m, 256), float("nan"), device=DEV)
        fused(dx, dx, sub, rows=200, off=37)
        torch.cuda.synchronize()
        assert torch.equal(sub[37:237], y[37:237]) and torch.isnan(sub[237:]).all() and torch.isnan(sub[:37]).all()
    assert lib.gfc_ffn_fused(nat.ptr(dx), 256, 256, None, 0, 0, nat.ptr(dw0), 512, nat.ptr(db0), nat.ptr(dga), nat.ptr(dbe),
                             nat.ptr(dw3), 256, nat.ptr(db3), None, nat.ptr(y3), 256, m, st()) == 1  # ldw3 < 512


def test_attention_natural_dispatch_64_problems():
    """64 problems of 1024 x 1024 (the self attention of a 32-pair batch): gfc_attention picks attention_kernel<2>
    itself (wgs(256) >= 1024).  Against a float64 soft-max attention, every problem, every head."""
    lib = nat.lib()
    g = gen(64)
    nprob, n = 64, 1024
    rows = nprob * n
    qkv = torch.randn((rows, 768), generator=g)
    qkv[:, :512] *= 1.5
    probs = torch.tensor([[i * n, n, i * n, n] for i in range(nprob)], dtype=torch.int32)
    qd = D(qkv)
    o = torch.full((rows, 256), float("nan"), device=DEV)
    nat.check(lib.gfc_attention(nat.ptr(qd), 768, nat.c_void_p(qd.data_ptr() + 256 * 4), 768,
                                nat.c_void_p(qd.data_ptr() + 512 * 4), 768, nat.ptr(o), 256, nat.ptr(D(probs)), nprob, n,
                                4, 0.125, None, 0, st()), "attention")
    torch.cuda.synchronize()
    with torch.no_grad():
        x = qd.double().view(nprob, n, 3, 4, 64).permute(2, 0, 3, 1, 4)  # [3, P, H, n, 64]
        ref = (torch.softmax(x[0] @ x[1].transpose(-1, -2) * 0.125, -1) @ x[2]).permute(0, 2, 1, 3).reshape(rows, 256)
    assert (o.double() - ref).abs().max().item() < 2e-5


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("shapes", [[(128, 128)], [(100, 161), (161, 100)], [(1, 1), (300, 33), (64, 257)],
                                    [(1024, 1024)], [(1024, 1024), (1024, 1000)]])
def test_attention(shapes, use_ws):
    """use_ws: with scratch the small problem sets take the key-split path (partials + merge kernel)."""
    lib = nat.lib()
    g = gen(len(shapes) + shapes[0][0])
    rows = sum(max(nq, nk) for nq, nk in shapes)
    q = torch.randn((rows, 256), generator=g) * 1.5
    k = torch.randn((rows, 256), generator=g) * 1.5
    v = torch.randn((rows, 256), generator=g)
    probs, r0 = [], 0
    for nq, nk in shapes:
        probs.append([r0, nq, r0, nk])
        r0 += max(nq, nk)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o = torch.full((rows, 256), float("nan"), device=DEV)
    pt = torch.tensor(probs, dtype=torch.int32, device=DEV)
    max_nq = max(s[0] for s in shapes)
    ws = None
    if use_ws:
        nbytes = lib.gfc_attention_workspace_bytes(len(shapes), max_nq, 4)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    nat.check(lib.gfc_attention(nat.ptr(qd), 256, nat.ptr(kd), 256, nat.ptr(vd), 256, nat.ptr(o), 256, nat.ptr(pt),
                                len(shapes), max_nq, 4, 0.125, nat.ptr(ws), 0 if ws is None else ws.numel(), st()),
              "attention")
    torch.cuda.synchronize()
    o = o.cpu()
    for r, nq, _, nk in probs:
        qq = q[r:r + nq].view(nq, 4, 64).transpose(0, 1)
        kk = k[r:r + nk].view(nk, 4, 64).transpose(0, 1)
        vv = v[r:r + nk].view(nk, 4, 64).transpose(0, 1)
        ref = (torch.softmax(qq @ kk.transpose(1, 2) * 0.125, -1) @ vv).transpose(0, 1).reshape(nq, 256)
        assert maxerr(o[r:r + nq], ref) < 2e-5
        if nq < max(nq, nk):
            assert torch.isnan(o[r + nq:r + max(nq, nk)]).all()  # rows of other problems untouched


@pytest.mark.parametrize("shapes", [[(600, 600)] * 2, [(100, 161), (161, 100)]], ids=["2x600x600", "cross_100_161"])
def test_attention_scratch_smaller_than_the_full_split(shapes):
    """gfc_att_split shrinks the key split until its partials fit the scratch it is offered (the callers with M != N
    offer less than the full split: the kernel indexes n_problems * max_nq query slots, they have fewer rows).  Three
    offers from one buffer filled with 0xA5: the full size (split 8); exactly the partials of a 3-way split (600 keys:
    10 tiles shared 4 + 4 + 2; 161 / 100 keys: 3 and 2 tiles, the third share of the latter empty); 4 bytes short of a
    2-way split (no split: the scratch is not touched).  Each result against a float64 soft-max; nothing behind the
    offer is written.  Whether the three results agree among themselves is not asserted."""
    lib = nat.lib()
    g = gen(len(shapes) + shapes[0][0])
    heads, n_prob = 4, len(shapes)
    rows = sum(max(nq, nk) for nq, nk in shapes)
    q = torch.randn((rows, 256), generator=g) * 1.5
    k = torch.randn((rows, 256), generator=g) * 1.5
    v = torch.randn((rows, 256), generator=g)
    probs, r0 = [], 0
    for nq, nk in shapes:
        probs.append([r0, nq, r0, nk])
        r0 += max(nq, nk)
    qd, kd, vd = D(q), D(k), D(v)
    pt = D(torch.tensor(probs, dtype=torch.int32))
    max_nq = max(s[0] for s in shapes)
    refs = []
    for r, nq, _, nk in probs:
        qq, kk, vv = (t[r:r + n_].double().view(n_, heads, 64).transpose(0, 1) for t, n_ in ((q, nq), (k, nk), (v, nk)))
        refs.append((torch.softmax(qq @ kk.transpose(1, 2) * 0.125, -1) @ vv).transpose(0, 1).reshape(nq, 256))
    full = lib.gfc_attention_workspace_bytes(n_prob, max_nq, heads)
    part = lambda split: n_prob * max_nq * heads * split * 66 * 4  # noqa: E731
    assert full == (part(8) + 255) // 256 * 256  # the dispatch wants all 8 splits for both problem sets
    buf = torch.empty(full, dtype=torch.uint8, device=DEV)
    for offer, split in ((full, 8), (part(3), 3), (part(2) - 4, 1)):
        buf.fill_(0xA5)
        o = torch.full((rows, 256), float("nan"), device=DEV)
        nat.check(lib.gfc_attention(nat.ptr(qd), 256, nat.ptr(kd), 256, nat.ptr(vd), 256, nat.ptr(o), 256, nat.ptr(pt),
                                    n_prob, max_nq, heads, 0.125, nat.ptr(buf), offer, st()), "attention")
        torch.cuda.synchronize()
        oc = o.cpu()
        for (r, nq, _, nk), ref in zip(probs, refs):
            assert maxerr(oc[r:r + nq], ref) < 2e-5, (offer, split)
            if nq < max(nq, nk):
                assert torch.isnan(oc[r + nq:r + max(nq, nk)]).all()  # rows of other problems untouched
        assert bool((buf[offer:] == 0xA5).all()), f"wrote behind an offer of {offer} bytes"
        # the partials of `split` shares end exactly at part(split): the path the offer is meant to reach did run
        used = buf[:offer] != 0xA5
        if split == 1:
            assert not bool(used.any()), "no split fits: the scratch must stay untouched"
        else:
            assert bool(used[part(split) - 66 * 4:part(split)].any()) and not bool(used[part(split):].any())


def test_attention_peaky_rows():
    """A spiked key forces the running-max rescale branch at a chosen tile (online softmax)."""
    lib = nat.lib()
    g = gen(77)
    n = 320
    q = torch.randn((n, 256), generator=g)
    k = torch.randn((n, 256), generator=g)
    v = torch.randn((n, 256), generator=g)
    k[200] = q[5] * 6  # late, very large score for query 5
    k[3] = q[9] * 6    # early spike for query 9
    o = torch.empty((n, 256), device=DEV)
    pt = torch.tensor([[0, n, 0, n]], dtype=torch.int32, device=DEV)
    nat.check(lib.gfc_attention(nat.ptr(D(q)), 256, nat.ptr(D(k)), 256, nat.ptr(D(v)), 256, nat.ptr(o),
                                256, nat.ptr(pt), 1, n, 4, 0.125, None, 0, st()), "attention")
    qq, kk, vv = (t.double().view(n, 4, 64).transpose(0, 1) for t in (q, k, v))
    ref = (torch.softmax(qq @ kk.transpose(1, 2) * 0.125, -1) @ vv).transpose(0, 1).reshape(n, 256)
    assert maxerr(o, ref) < 2e-5


def test_layernorm_gelu():
    lib = nat.lib()
    g = gen(4)
    x = torch.randn((301, 512), generator=g) * 3 + 0.5
    gamma, beta = torch.rand((512,), generator=g) + 0.5, torch.randn((512,), generator=g)
    xd = x.to(DEV)
    nat.check(lib.gfc_layernorm_gelu(nat.ptr(xd), 512, 301, 512, nat.ptr(D(gamma)), nat.ptr(D(beta)), st()),
              "ln")
    ref = F.gelu(F.layer_norm(x, (512,), gamma, beta, 1e-5))
    assert maxerr(xd, ref) < 2e-5


# ---------------------------------------------------------------------------- detection
@pytest.mark.parametrize("b,h8,w8,bn", [(2, 60, 80, True), (3, 25, 41, False), (1, 1, 3, True)])
def test_detector_head_fused_softmax_d2s(b, h8, w8, bn):
    """gfc_sp_detector_head (1x1 conv 256 -> 65 [+ BN affine] + softmax over 65 + dustbin drop + depth-to-space in one
    launch; superpoint_open.py:111-114,138-144) against float64, and against the two-stage form it replaced in round 5
    restated here -- the logits gfc_linear (N = 65) writes, then expf of (logit - max) summed over c = 0..64 in order:
    within 1e-7, with the same winner in every cell (torch's device exp is not guaranteed to be the kernels' expf, so
    bit-equality of the values is not what is asserted).  Cell counts that are not multiples of the 128-cell workgroup
    tile and a hidden map with a row pitch of 512 (the merged head's output) are covered; operands that are not 16-byte
    aligned are refused (the kernel reads them with 128-bit loads)."""
    lib = nat.lib()
    g = gen(31 + h8)
    rows = b * h8 * w8
    hidden = torch.randn((rows, 512), generator=g).clamp_(min=0)  # ReLU output of the merged 3x3 head
    w = torch.randn((65, 256), generator=g) / 8
    bias = torch.randn((65,), generator=g)
    scale = (torch.rand((65,), generator=g) + 0.5) if bn else None
    shift = torch.randn((65,), generator=g) if bn else None
    hd, wd, bd, scd, shd = D(hidden), D(w), D(bias), D(scale), D(shift)
    heat = torch.empty((b, h8 * 8, w8 * 8), device=DEV)
    nat.check(lib.gfc_sp_detector_head(nat.ptr(hd), 512, nat.ptr(wd), nat.ptr(bd), nat.ptr(scd), nat.ptr(shd), b, h8, w8,
                                       nat.ptr(heat), st()), "gfc_sp_detector_head")
    # float64 reference
    logits = hidden[:, :256].double() @ w.double().T + bias.double()
    if bn:
        logits = logits * scale.double() + shift.double()
    p = torch.softmax(logits, 1)[:, :64].reshape(b, h8, w8, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h8 * 8, w8 * 8)
    assert maxerr(heat, p) < 2e-6
    # the two-stage form: logits by the GEMM entry point, then the soft-max arithmetic of the kernel it replaced
    lg = torch.empty((rows, 65), device=DEV)
    nat.check(lib.gfc_linear(nat.ptr(hd), 512, 256, None, 0, 0, nat.ptr(wd), 256, nat.ptr(bd), nat.ptr(scd), nat.ptr(shd), 1.0,
                             None, None, None, 0, nat.ptr(lg), 65, rows, 65, st()), "gfc_linear")
    m = lg.max(1, keepdim=True).values
    e = torch.exp(lg - m)
    ssum = torch.zeros((rows,), device=DEV)
    for c in range(65):  # sequential fp32 sum over the channels, as the kernel sums
        ssum = ssum + e[:, c]
    two = (e[:, :64] / ssum[:, None]).reshape(b, h8, w8, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h8 * 8, w8 * 8)
    # torch.exp on the device is not guaranteed to be the expf the kernels call: equality is demanded of the LOGIT side
    # (max and arg-max of every cell, i.e. the winner of each cell's soft-max) and 1e-7 of the values
    assert maxerr(heat, two) < 1e-7
    cells_f = heat.reshape(b, h8, 8, w8, 8).permute(0, 1, 3, 2, 4).reshape(rows, 64)
    assert torch.equal(cells_f.argmax(1), lg[:, :64].argmax(1))
    # misaligned operands: GFC_ERR_INVALID (1), not a memory fault
    for hp, wp in ((hd.data_ptr() + 4, wd.data_ptr()), (hd.data_ptr(), wd.data_ptr() + 8)):
        assert lib.gfc_sp_detector_head(hp, 512, wp, nat.ptr(bd), nat.ptr(scd), nat.ptr(shd), b, h8, w8, nat.ptr(heat), st()) == 1


@pytest.mark.parametrize("r", [0, 1, 3, 4])
def test_nms_golden_bit_exact(golden, r):
    lib = nat.lib()
    gd = golden("nms")
    s = gd[f"in_r{r}"].to(DEV)
    out = torch.empty_like(s)
    nat.check(lib.gfc_sp_nms(nat.ptr(s), s.shape[0], s.shape[1], s.shape[2], r, 0, None, nat.ptr(out), st()), "nms")
    assert torch.equal(out.cpu(), gd[f"out_r{r}"])


@pytest.mark.parametrize("r,h,w", [(3, 480, 640), (4, 100, 77), (2, 33, 200), (1, 5, 3), (3, 1, 300), (4, 130, 24),
                                   (3, 65, 35), (1, 64, 108), (2, 200, 45)])
def test_nms_large_vs_oracle(r, h, w):
    lib = nat.lib()
    g = gen(r * 100 + h)
    s = torch.rand((2, h, w), generator=g)
    s[1] = (s[1] * 16).round() / 16  # many exact ties / plateaus
    s[0, 50:60, 20:60] = 0.5
    sd = s.to(DEV)
    out = torch.empty_like(sd)
    wh = torch.tensor([[w - 5, h - 9], [w, h]], dtype=torch.int32, device=DEV)
    nat.check(lib.gfc_sp_nms(nat.ptr(sd), 2, h, w, r, 4, nat.ptr(wh), nat.ptr(out), st()), "nms")
    ref = osp.kill_borders(osp.nms(s, r), 4, wh.cpu().float())
    assert torch.equal(out.cpu(), ref)


def run_select(scores, th, k):
    from glue_factory_colon_amd._superpoint_common import SuperPointRunner

    kp, sc, cnt = SuperPointRunner().select(scores.to(DEV).contiguous(), th, k)
    torch.cuda.synchronize()
    return kp.cpu(), sc.cpu(), cnt.cpu()


@pytest.mark.parametrize("k", [50, 1024, 5000, None])
def test_select_bit_exact(k):
    g = gen(12)
    h, w = 120, 160
    s = torch.rand((3, h, w), generator=g)
    s = osp.kill_borders(osp.nms(s, 3), 4)
    s[2] = -1.0
    s[2, 40, 50] = 0.25  # a single candidate
    kp, sc, cnt = run_select(s, 0.0, k)
    for i in range(3):
        xy, val = osp.select_keypoints(s[i], 0.0, k)
        n = int(cnt[i])
        assert n == len(val)
        assert torch.equal(kp[i, :n], xy) and torch.equal(sc[i, :n], val)


@pytest.mark.parametrize("k,r", [(50, 3), (1024, 3), (5000, 4), (300, 1)])
def test_fused_nms_select_equals_separate_stages(k, r):
    """gfc_sp_nms_select (candidates emitted by the NMS kernel, unordered) == gfc_sp_nms + gfc_sp_select, bit for bit,
    in both branches (more than k candidates: top-k sorted; fewer: all, row-major)."""
    from glue_factory_colon_amd._superpoint_common import SuperPointRunner

    g = gen(k + r)
    h, w = 150, 200
    s = torch.rand((3, h, w), generator=g)
    s[1] = (s[1] * 64).round() / 64  # ties
    s[2, :, :] = 0.0
    s[2, 40:44, 50:60] = 0.3
    run = SuperPointRunner()
    sd = D(s)
    wh = D(torch.tensor([[w, h], [w - 7, h - 3], [w, h]], dtype=torch.int32))
    nms = run.nms(sd, r, 4, wh)
    kp_a, sc_a, cnt_a = run.select(nms, 0.0, k)
    kp_b, sc_b, cnt_b = run.nms_select(sd, r, 4, wh, 0.0, k)
    torch.cuda.synchronize()
    assert torch.equal(cnt_a, cnt_b) and torch.equal(kp_a, kp_b) and torch.equal(sc_a, sc_b)
    assert int(cnt_a[2]) < k


def test_fused_nms_select_candidate_overflow_paths():
    """The streaming NMS buffers its candidates per wave (256 slots) and reserves list space with one atomic per flush: a
    NEGATIVE detection threshold makes every pixel a candidate (zeros included), so every wave flushes several times, and
    the result must still equal the separate stages.  Also k larger than the number of candidates and a 1-row image."""
    from glue_factory_colon_amd._superpoint_common import SuperPointRunner

    g = gen(91)
    run = SuperPointRunner()
    for (h, w, r, th, k) in ((96, 130, 3, -0.5, 4000), (70, 64, 2, -2.0, 8192), (1, 500, 1, 0.0, 100), (40, 40, 4, 0.0, 8192)):
        s = torch.rand((2, h, w), generator=g)
        s[1] = (s[1] * 8).round() / 8
        sd = D(s)
        nms = run.nms(sd, r, 2, None)
        kp_a, sc_a, cnt_a = run.select(nms, th, k)
        kp_b, sc_b, cnt_b = run.nms_select(sd, r, 2, None, th, k)
        torch.cuda.synchronize()
        assert torch.equal(cnt_a, cnt_b), (h, w, r, cnt_a, cnt_b)
        for i in range(2):
            n = int(cnt_a[i])
            assert torch.equal(kp_a[i, :n], kp_b[i, :n]) and torch.equal(sc_a[i, :n], sc_b[i, :n]), (h, w, r, i)


@pytest.mark.parametrize("mode", ["1", "2"])
def test_nms_kernel_variants_via_knob(mode):
    """The default picks the NMS kernel by problem size (few images: 64 x 64 tiles on an LDS image, ten passes; many:
    the streaming kernel -- waves walk column bands with the pool windows in registers).  GFC_NMS_MODE=1 / 2 force one
    of them for every size: both pass the same bit-exact tests."""
    import subprocess
    import sys

    env = dict(os.environ, GFC_NMS_MODE=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                        "(test_nms_golden or test_nms_large or test_fused_nms_select or test_select_bit_exact) and not via_knob",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-400:])


def test_select_ties_and_empty():
    """Equal scores: lower linear index first (what torch.topk on CPU returns for these inputs is
    not contractual; the HIP rule is documented in the header) -- here checked against a stable sort."""
    h, w = 64, 96
    s = torch.full((2, h, w), -1.0)
    s[0, 8:56:4, 8:88:4] = 0.5
    s[0, 20, 20] = 0.9
    kp, sc, cnt = run_select(s, 0.0, 40)
    assert cnt.tolist() == [40, 0]
    ys, xs = torch.where(s[0] > 0)
    order = torch.argsort(-s[0][ys, xs], stable=True)[:40]
    assert torch.equal(kp[0, :40], torch.stack([xs[order], ys[order]], -1).float())
    assert (sc[1] == 0).all()


PLANT_H = PLANT_W = 132  # 66 x 66 sites two pixels apart: isolated under a radius-1 NMS, room for 4097 candidates


def planted_scores(values, seed):
    """[PLANT_H, PLANT_W] map, -1 except len(values) seeded sites (even rows and columns), which hold `values` in
    row-major order of the sites."""
    sites = torch.randperm(66 * 66, generator=gen(seed))[: len(values)].sort().values
    s = torch.full((PLANT_H, PLANT_W), -1.0)
    s[2 * (sites // 66), 2 * (sites % 66)] = values
    return s


def expected_selection(s, k):
    """The rule of test_select_ties_and_empty: all candidates row-major when there are at most k, else a stable
    descending sort (equal scores: lower linear index first) cut at k."""
    ys, xs = torch.where(s > 0)
    v = s[ys, xs]
    if len(v) > k:
        order = torch.argsort(-v, stable=True)[:k]
        ys, xs, v = ys[order], xs[order], v[order]
    return torch.stack([xs, ys], -1).float(), v


def check_selection(s, k):
    """gfc_sp_select on the planted maps and gfc_sp_nms_select (radius 1, which keeps every isolated site and hands the
    candidates over unordered) against expected_selection; rows beyond the count are zero."""
    from glue_factory_colon_amd._superpoint_common import SuperPointRunner

    run = SuperPointRunner()
    sd = D(s)
    results = {"select": run.select(sd, 0.0, k), "nms_select": run.nms_select(sd, 1, 0, None, 0.0, k)}
    torch.cuda.synchronize()
    for name, (kp, sc, cnt) in results.items():
        for i in range(s.shape[0]):
            xy, v = expected_selection(s[i], k)
            c = int(cnt[i])
            assert c == len(v), (name, i, k, c, len(v))
            assert torch.equal(kp[i, :c].cpu(), xy) and torch.equal(sc[i, :c].cpu(), v), (name, i, k)
            assert not kp[i, c:].any() and not sc[i, c:].any(), (name, i, k)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_select_counts_at_wave_and_chunk_boundaries(n):
    """Exactly n candidates, k = n - 1, n, n + 1: image 0 with n distinct scores (the radix select stops as soon as a
    bin holds exactly what is wanted), image 1 with n equal scores (n > k sends it through all eight passes, into the
    index word).  n <= k returns all candidates row-major: through the scan of the dense map in gfc_sp_select, through
    the second sort in gfc_sp_nms_select."""
    distinct = (torch.randperm(n, generator=gen(n)) + 1).float() / 8192  # exact in fp32, all different, in (0, 1)
    s = torch.stack([planted_scores(distinct, n), planted_scores(torch.full((n,), 0.5), n + 1)])
    for k in (n - 1, n, n + 1):
        if 1 <= k <= 8192:
            check_selection(s, k)


def test_select_tie_group_that_straddles_k():
    """k - 3 distinct higher scores, then ten equal ones: the three with the lowest linear index complete the k."""
    k = 100
    values = torch.cat([0.5 + torch.arange(1, k - 2).float() / 1024, torch.full((10,), 0.25)])
    values = values[torch.randperm(len(values), generator=gen(5))]
    check_selection(planted_scores(values, 6)[None], k)


def test_specular_filter_kernels_vs_oracle():
    """gfc_sp_filter_keypoints (stable compaction over several 1024-chunks, counts on both sides of a wave and of a
    chunk, fractional key points with the reference's default offset 0.5, image_size crop) and gfc_sp_mask_scores
    against extractors/utils.py restated."""
    lib = nat.lib()
    g = gen(91)
    b, cap, hm, wm = 8, 2500, 70, 90
    mask = torch.rand((b, hm, wm), generator=g) > 0.3
    kp = torch.rand((b, cap, 2), generator=g) * torch.tensor([wm + 4.0, hm + 4.0]) - 2.0  # some outside
    kp[:, ::3] = kp[:, ::3].round() + 0.5                                              # exact pixel centres too
    sc = torch.rand((b, cap), generator=g)
    counts = torch.tensor([cap, 1700, 0, 1, 64, 65, 1024, 1025], dtype=torch.int32)
    wh = torch.tensor([[90, 70], [80, 60], [90, 70], [90, 70], [90, 70], [85, 66], [90, 70], [80, 60]], dtype=torch.int32)
    kd, sd_, cd = kp.clone().to(DEV), sc.clone().to(DEV), counts.clone().to(DEV)
    nat.check(lib.gfc_sp_filter_keypoints(nat.ptr(kd), nat.ptr(sd_), nat.ptr(cd), b, cap, nat.ptr(D(mask.to(torch.uint8))),
                                          hm, wm, nat.ptr(D(wh)), 0.5, st()), "filter")
    torch.cuda.synchronize()
    for i in range(b):
        n = int(counts[i])
        k_ref, s_ref = osp.filter_keypoints_by_specular_mask(kp[i, :n], mask[i], sc[i, :n],
                                                             image_size=wh[i].float(), keypoint_offset=0.5)
        assert int(cd[i]) == k_ref.shape[0]
        assert torch.equal(kd[i, : k_ref.shape[0]].cpu(), k_ref) and torch.equal(sd_[i, : k_ref.shape[0]].cpu(), s_ref)
    # score-map form: exactly the pixels inside the (cropped) mask keep their score
    h, w = 64, 88
    scores = torch.rand((b, h, w), generator=g)
    sdev = scores.clone().to(DEV)
    nat.check(lib.gfc_sp_mask_scores(nat.ptr(sdev), b, h, w, nat.ptr(D(mask.to(torch.uint8))), hm, wm, nat.ptr(D(wh)),
                                     st()), "mask")
    torch.cuda.synchronize()
    for i in range(b):
        keep = torch.zeros((h, w), dtype=torch.bool)
        eh, ew = min(hm, int(wh[i, 1]), h), min(wm, int(wh[i, 0]), w)
        keep[:eh, :ew] = mask[i, :eh, :ew]
        out = sdev[i].cpu()
        assert torch.equal(out[keep], scores[i][keep]) and torch.isinf(out[~keep]).all() and (out[~keep] < 0).all()


@pytest.mark.parametrize("mode,name", [(0, "open"), (1, "legacy"), (2, "fixed")])
def test_sample_descriptors(mode, name):
    lib = nat.lib()
    g = gen(21 + mode)
    b, h8, w8, n = 2, 15, 20, 300
    dense = torch.randn((b, 256, h8, w8), generator=g)
    kp = torch.stack([torch.randint(0, w8 * 8, (b, n), generator=g), torch.randint(0, h8 * 8, (b, n), generator=g)],
                     -1).float()
    kp[0, 0] = torch.tensor([0.0, 0.0])
    kp[0, 1] = torch.tensor([w8 * 8 - 1.0, h8 * 8 - 1.0])
    ref = osp.sample_descriptors(kp, F.normalize(dense, dim=1), 8, name)
    raw = dense.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.empty((b, n, 256), device=DEV)
    kout = torch.empty((b, n, 2), device=DEV)
    nat.check(lib.gfc_sp_sample(nat.ptr(raw), b, h8, w8, 256, nat.ptr(D(kp)), None, n, mode, nat.ptr(out),
                                nat.ptr(kout), st()), "sample")
    assert maxerr(out, ref) < 1e-5
    assert torch.equal(kout.cpu(), kp + 0.5)


# ---------------------------------------------------------------------------- assignment
def test_log_assignment_and_filter_golden(golden):
    lib = nat.lib()
    gd = golden("assignment")
    sim, z0, z1 = gd["sim"], gd["z0"], gd["z1"]
    b, m, n = sim.shape
    out = torch.empty((b, m + 1, n + 1), device=DEV)
    ws = torch.empty(2 * b * (m + n) * 4, dtype=torch.uint8, device=DEV)
    nat.check(lib.gfc_lg_log_assignment(nat.ptr(D(sim)), nat.ptr(D(z0.reshape(b, m).contiguous())),
                                        nat.ptr(D(z1.reshape(b, n).contiguous())), b, m, n, nat.ptr(out),
                                        nat.ptr(ws), ws.numel(), st()), "log_assignment")
    assert maxerr(out, gd["log_assignment"]) < 1e-5
    for th, tag in ((0.0, "0p0"), (0.1, "0p1"), (0.5, "0p5")):
        m0, m1, s0, s1 = run_filter(gd["log_assignment"], th)
        assert torch.equal(m0, gd[f"m0_{tag}"]) and torch.equal(m1, gd[f"m1_{tag}"])
        assert maxerr(s0, gd[f"s0_{tag}"]) < 1e-6 and maxerr(s1, gd[f"s1_{tag}"]) < 1e-6
    m0, m1, _, _ = run_filter(gd["perm_log_assignment"], 0.1)
    assert torch.equal(m0, gd["perm_m0"]) and torch.equal(m1, gd["perm_m1"])


def run_filter(scores, th):
    lib = nat.lib()
    b, m, n = scores.shape[0], scores.shape[1] - 1, scores.shape[2] - 1
    m0 = torch.empty((b, m), dtype=torch.long, device=DEV)
    m1 = torch.empty((b, n), dtype=torch.long, device=DEV)
    s0, s1 = torch.empty((b, m), device=DEV), torch.empty((b, n), device=DEV)
    ws = torch.empty(b * (m + n) * 8, dtype=torch.uint8, device=DEV)
    nat.check(lib.gfc_lg_filter_matches(nat.ptr(D(scores)), b, m, n, th, nat.ptr(m0), nat.ptr(m1),
                                        nat.ptr(s0), nat.ptr(s1), nat.ptr(ws), ws.numel(), st()), "filter")
    torch.cuda.synchronize()
    return m0.cpu(), m1.cpu(), s0.cpu(), s1.cpu()


def test_filter_matches_large_random_bit_exact():
    g = gen(31)
    sc = torch.randn((2, 1025, 1025), generator=g)
    sc = (sc * 8).round() / 8  # heavy ties: first-index arg-max must match torch CPU
    m0, m1, s0, s1 = run_filter(sc, 0.2)
    r0, r1, rs0, rs1 = olg.filter_matches(sc, 0.2)
    assert torch.equal(m0, r0) and torch.equal(m1, r1)
    assert maxerr(s0, rs0) < 1e-6 and maxerr(s1, rs1) < 1e-6


def test_posenc(golden):
    lib = nat.lib()
    gd = golden("lightglue")
    kp = gd["keypoints0"]  # [2,160,2]
    b, n, _ = kp.shape
    from glue_factory_colon_amd import weights

    wr = weights.lightglue_state_dict(0)["posenc.Wr.weight"]
    cos = torch.empty((b * n, 64), device=DEV)
    sin = torch.empty((b * n, 64), device=DEV)
    row0 = torch.arange(b, dtype=torch.int32, device=DEV) * n
    cnt = torch.full((b,), n, dtype=torch.int32, device=DEV)
    nat.check(lib.gfc_lg_posenc(nat.ptr(D(kp.reshape(-1, 2).contiguous())), None, nat.ptr(D(gd["image_size"])),
                                nat.ptr(row0), nat.ptr(cnt), b, n, nat.ptr(D(wr)), 2, nat.ptr(cos),
                                nat.ptr(sin), st()), "posenc")
    enc = gd["enc0"]  # [2,B,1,N,64]
    assert maxerr(cos.view(b, n, 64), enc[0, :, 0]) < 1e-5
    assert maxerr(sin.view(b, n, 64), enc[1, :, 0]) < 1e-5


@pytest.mark.parametrize("b,m,n", [(2, 1024, 1024), (1, 1500, 2100), (3, 130, 67), (1, 1, 5), (2, 64, 1025)])
def test_assignment_head_two_pass_tail_vs_oracle(b, m, n):
    """gfc_lg_assign = final_proj + matchability + sim GEMM + the two-pass tail (row / column statistics in one sweep;
    final scores, dustbin row / column and both arg-maxes in the second) + mutual check, against the oracle's
    match_assignment + filter_matches (lightglue.py:257-319): log-assignment within 1e-4 relative, matches bit-exact.
    Ragged sizes: several 1024-column chunks, partial bands, N+1 row pitch that is not a multiple of 4."""
    import ctypes

    lib = nat.lib()
    g = gen(b * 1000 + m + n)
    x0 = torch.randn((b, m, 256), generator=g)
    x1 = torch.randn((b, n, 256), generator=g)
    x1[:, : min(m, n)] += 2.5 * x0[:, : min(m, n)].flip(1)  # structure: peaky rows / columns, many mutual matches
    sd = {"log_assignment.0.final_proj.weight": torch.randn((256, 256), generator=g) / 8,
          "log_assignment.0.final_proj.bias": torch.randn((256,), generator=g) * 0.1,
          "log_assignment.0.matchability.weight": torch.randn((1, 256), generator=g) / 16,
          "log_assignment.0.matchability.bias": torch.randn((1,), generator=g)}
    ref = olg.match_assignment(sd, "log_assignment.0", x0, x1)
    r0, r1, rs0, rs1 = olg.filter_matches(ref, 0.1)
    p = nat.LgParams()
    p.n_layers = 1
    p.input_dim = 256
    p.final_proj_w[0] = D(sd["log_assignment.0.final_proj.weight"]).data_ptr()
    p.final_proj_b[0] = D(sd["log_assignment.0.final_proj.bias"]).data_ptr()
    p.matchability_w[0] = D(sd["log_assignment.0.matchability.weight"].reshape(-1)).data_ptr()
    p.matchability_b[0] = D(sd["log_assignment.0.matchability.bias"]).data_ptr()
    m0 = torch.empty((b, m), dtype=torch.long, device=DEV)
    m1 = torch.empty((b, n), dtype=torch.long, device=DEV)
    s0, s1 = torch.empty((b, m), device=DEV), torch.empty((b, n), device=DEV)
    la = torch.full((b, m + 1, n + 1), float("nan"), device=DEV)
    ws = torch.full((lib.gfc_lg_assign_workspace_bytes(b, m, n),), 0xFF, dtype=torch.uint8, device=DEV)
    x0d, x1d = D(x0.reshape(b * m, 256)), D(x1.reshape(b * n, 256))
    nat.check(lib.gfc_lg_assign(ctypes.byref(p), 0, nat.ptr(x0d), nat.ptr(x1d), b, m, n, 0.1, nat.ptr(m0), nat.ptr(m1),
                                nat.ptr(s0), nat.ptr(s1), nat.ptr(la), nat.ptr(ws), ws.numel(), st()), "gfc_lg_assign")
    torch.cuda.synchronize()
    err = ((la.cpu() - ref).abs() / (1 + ref.abs())).max().item()
    assert err < 1e-4, err
    assert torch.equal(m0.cpu(), r0) and torch.equal(m1.cpu(), r1)
    assert maxerr(s0, rs0) < 1e-5 and maxerr(s1, rs1) < 1e-5
    if min(m, n) > 60:
        assert int((r0 >= 0).sum()) > 0.3 * min(m, n) * b  # the case is not degenerate
    # stage-isolated: the arg-maxes the fused pass produced equal the standalone filter on the SAME finished matrix
    f0, f1, _, _ = run_filter(la, 0.1)
    assert torch.equal(m0.cpu(), f0) and torch.equal(m1.cpu(), f1)


def test_pad_keypoints_random_c():
    """gfc_sp_pad_keypoints = pad_and_stack(mode="random_c") + zero scores in one launch (models/utils/misc.py:19-62):
    valid entries untouched, padded coordinates inside [min, max] of the image's own key points per column (fallback
    bounds for an empty image), padded scores 0, reproducible under torch.manual_seed."""
    from glue_factory_colon_amd._superpoint_common import pad_keypoints_native

    g = gen(8)
    b, k = 4, 300
    kp = torch.rand((b, k, 2), generator=g) * torch.tensor([600.0, 400.0]) + 20
    sc = torch.rand((b, k), generator=g) + 0.1
    counts = torch.tensor([k, 120, 0, 1], dtype=torch.int32)
    img = torch.zeros((b, 1, 480, 640), device=DEV)
    data = {"image_size": torch.tensor([[640.0, 480.0], [500.0, 470.0], [640.0, 333.0], [640.0, 480.0]], device=DEV)}

    def run(seed):
        torch.manual_seed(seed)
        a, s_ = pad_keypoints_native(kp.clone().to(DEV), sc.clone().to(DEV), counts.to(DEV), k, 0, data, img)
        torch.cuda.synchronize()
        return a.cpu(), s_.cpu()

    a, s_ = run(3)
    assert torch.equal(a[0], kp[0]) and torch.equal(s_[0], sc[0])                       # full image: untouched
    assert torch.equal(a[1, :120], kp[1, :120]) and torch.equal(s_[1, :120], sc[1, :120])
    lo, hi = kp[1, :120].amin(0), kp[1, :120].amax(0)
    assert (a[1, 120:] >= lo).all() and (a[1, 120:] <= hi).all() and (s_[1, 120:] == 0).all()
    assert a[1, 120:].std(0).min() > 10                                                # spread over the range, not constant
    assert (a[2] >= 0).all() and (a[2] <= 333).all() and (s_[2] == 0).all()            # empty: bounds (0, image_size.min())
    assert a[2].max() > 250
    assert torch.equal(a[3, 1:], kp[3, :1].expand(k - 1, 2)) and (s_[3, 1:] == 0).all()  # one point: min == max
    b2, _ = run(3)
    c2, _ = run(4)
    assert torch.equal(a, b2) and not torch.equal(a, c2)
