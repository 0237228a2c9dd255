"""The opt-in fp16 matcher's host side (no GPU): the `matmul_precision` key, the C ABI fields appended to
gfc_lg_params, the exported kernels, and argument checks that refuse before anything reaches a device."""
import ctypes
import os
import re

import pytest

from glue_factory_colon_amd import _native as nat
from glue_factory_colon_amd import lightglue, lightglue_pretrained

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.mark.parametrize("bad", ["fp64", "bf16", "FP16", "", None, 16, True])
def test_bad_matmul_precision_raises(bad):
    with pytest.raises(ValueError, match="matmul_precision"):
        lightglue.LightGlue({"matmul_precision": bad})
    with pytest.raises(ValueError, match="matmul_precision"):
        lightglue_pretrained.LightGlue({"matmul_precision": bad})


def test_matmul_precision_default_and_forwarding():
    assert lightglue.LightGlue({}).conf.matmul_precision == "fp32"
    assert lightglue.LightGlue({"matmul_precision": "fp16"}).conf.matmul_precision == "fp16"
    net = lightglue_pretrained.LightGlue({"matmul_precision": "fp16"}).net
    assert net.conf.matmul_precision == "fp16"
    # `mp` keeps the reference class's meaning (none): it does not select the fp16 matcher
    assert lightglue.LightGlue({"mp": True}).conf.matmul_precision == "fp32"


def test_lg_params_fp16_fields_are_appended_last():
    names = [f[0] for f in nat.LgParams._fields_]
    tail = ["precision", "input_proj_w16", "wqkv16", "s_out_w16", "s_ffn0_w16", "s_ffn3_w16", "c_qkv_w16", "c_out_w16",
            "c_ffn0_w16", "c_ffn3_w16", "final_proj_w16"]
    assert names[-len(tail):] == tail
    assert names.index("token_b") == len(names) - len(tail) - 1
    assert nat.LgParams().precision == nat.GFC_LG_FP32 == 0 and nat.GFC_LG_FP16 == 1
    # the header declares the same fields in the same order, after token_b
    header = open(os.path.join(ROOT, "include", "gfc_amd.h")).read()
    body = header[header.index("token_b[GFC_LG_MAX_LAYERS]"):header.index("} gfc_lg_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"\b(\w+)(?:\[GFC_LG_MAX_LAYERS\])?;", body)
    assert declared[1:] == tail, declared
    assert re.search(r"#define GFC_LG_FP32 0\b", header) and re.search(r"#define GFC_LG_FP16 1\b", header)


def test_fp16_kernels_exported():
    lib = nat.lib()
    for name in ("gfc_linear_f16", "gfc_batched_nt_f16", "gfc_attention_f16"):
        assert name in nat.SIGNATURES and hasattr(lib, name), name


def _fake(n=1):
    """Host addresses that are never dereferenced: every call below is refused by its argument checks first."""
    return ctypes.c_void_p(0x1000 * n)


def test_linear_f16_refuses_invalid_arguments():
    lib = nat.lib()
    a, w, y = _fake(1), _fake(2), _fake(3)

    def call(A0=a, a0f=0, lda0=256, K0=256, A1=None, a1f=1, lda1=0, K1=0, W=w, ldw=256, rcs=None, rc=None, rs=None,
             rot=0, Y=y, ldy=256, M=10, N=256):
        return lib.gfc_linear_f16(A0, a0f, lda0, K0, A1, a1f, lda1, K1, W, ldw, None, 1.0, None, rcs, rc, rs, rot, Y, 0,
                                  ldy, M, N, None)

    for kw in ({"A0": None}, {"W": None}, {"Y": None}, {"M": 0}, {"N": -1}, {"K0": 48}, {"K0": 0},
               {"K1": 32}, {"A1": _fake(4), "K1": 0}, {"a0f": 1, "lda0": 260}, {"lda0": 258}, {"ldw": 260},
               {"ldw": 128}, {"ldy": 100}, {"rc": _fake(5)}, {"rcs": _fake(5), "rc": _fake(6), "rs": _fake(7), "rot": 64},
               {"rcs": _fake(5), "rot": 96}, {"rcs": _fake(5), "rot": 0}, {"rcs": _fake(5), "rot": 512}):
        assert call(**kw) == INVALID, kw


def test_batched_nt_f16_refuses_invalid_arguments():
    lib = nat.lib()

    def call(A=_fake(1), lda=256, sa=256 * 4, B=_fake(2), ldb=256, sb=256 * 4, Y=_fake(3), ldy=5, M=4, N=4, K=256,
             batch=2):
        return lib.gfc_batched_nt_f16(A, lda, sa, B, ldb, sb, Y, ldy, sa, M, N, K, batch, None)

    for kw in ({"A": None}, {"B": None}, {"Y": None}, {"M": 0}, {"N": 0}, {"K": 40}, {"batch": 0}, {"lda": 252},
               {"ldb": 100}, {"ldy": 3}, {"sa": 1027}):
        assert call(**kw) == INVALID, kw


def test_attention_f16_refuses_invalid_arguments():
    lib = nat.lib()

    def call(Q=_fake(1), ldq=768, K=_fake(2), ldk=768, V=_fake(3), ldv=768, O=_fake(4), ldo=256, pt=_fake(5), npb=2,
             maxn=8, heads=4):
        return lib.gfc_attention_f16(Q, ldq, K, ldk, V, ldv, O, ldo, pt, npb, maxn, heads, 0.125, None, 0, None)

    for kw in ({"Q": None}, {"K": None}, {"V": None}, {"O": None}, {"pt": None}, {"npb": 0}, {"maxn": 0},
               {"heads": 0}, {"ldq": 772}, {"ldk": 252}, {"ldv": 770}, {"ldo": 250}, {"ldo": 128}):
        assert call(**kw) == INVALID, kw


LG_ARRAYS = ["wqkv", "bqkv", "s_out_w", "s_out_b", "s_ffn0_w", "s_ffn0_b", "s_ln_g", "s_ln_b", "s_ffn3_w", "s_ffn3_b",
             "c_qkv_w", "c_qkv_b", "c_out_w", "c_out_b", "c_ffn0_w", "c_ffn0_b", "c_ln_g", "c_ln_b", "c_ffn3_w", "c_ffn3_b"]
LG_ARRAYS_F16 = ["wqkv16", "s_out_w16", "s_ffn0_w16", "s_ffn3_w16", "c_qkv_w16", "c_out_w16", "c_ffn0_w16", "c_ffn3_w16",
                 "final_proj_w16"]
LG_HEADS = ["final_proj_w", "final_proj_b", "matchability_w", "matchability_b", "token_w", "token_b"]


def _pointer_arrays(struct):
    """The fields of a parameter struct that are arrays of pointers, as the header declares them."""
    return [name for name, t in struct._fields_ if issubclass(t, ctypes.Array) and t._type_ is ctypes.c_void_p]


def _fp16_params(drop=None):
    """A params struct that asks for fp16 with every matrix present (never-dereferenced addresses), minus `drop`."""
    assert _pointer_arrays(nat.LgParams) == LG_ARRAYS + LG_HEADS + LG_ARRAYS_F16
    p = nat.LgParams()
    p.n_layers, p.input_dim, p.posenc_dim, p.precision = 2, 256, 2, nat.GFC_LG_FP16
    p.posenc_wr = 0x1000
    for name in _pointer_arrays(nat.LgParams):
        if name not in ("token_w", "token_b"):
            if name in ("s_out_w", "s_out_b", "c_out_w", "c_out_b", "s_out_w16", "c_out_w16"):
                continue  # folded
            arr = getattr(p, name)
            for i in range(2):
                arr[i] = 0x2000
    if drop:
        getattr(p, drop[0])[drop[1]] = None
    return p


@pytest.mark.parametrize("drop", [("wqkv16", 0), ("s_ffn0_w16", 1), ("s_ffn3_w16", 0), ("c_qkv_w16", 1),
                                  ("c_ffn0_w16", 0), ("c_ffn3_w16", 1), ("final_proj_w16", 1)])
def test_fp16_matcher_with_a_missing_matrix_is_invalid(drop):
    """precision = GFC_LG_FP16 with one fp16 matrix missing: the whole-matcher entry points, gfc_lg_layer and
    gfc_lg_assign refuse it (GFC_ERR_INVALID) before any launch."""
    lib = nat.lib()
    p = _fp16_params(drop)
    f = _fake
    m = (ctypes.c_int32 * 1)(4)
    n = (ctypes.c_int32 * 1)(4)
    ws = 1 << 30
    assert lib.gfc_lg_forward_packed(ctypes.byref(p), f(1), f(2), f(3), f(4), None, 1, 4, 4, 0.1, f(5), f(6), f(7), f(8),
                                     f(9), f(10), f(11), ws, None, None) == INVALID
    assert lib.gfc_lg_forward_ragged(ctypes.byref(p), f(1), f(2), f(3), f(4), None, 1, m, n, 0.1, f(5), f(6), f(7), f(8),
                                     f(9), f(10), f(11), ws, None, None) == INVALID
    assert lib.gfc_lg_forward(ctypes.byref(p), f(1), f(12), f(2), f(13), f(3), f(4), None, None, 1, 4, 4, 0.1, f(5),
                              f(6), f(7), f(8), f(9), None, None, f(11), ws, None) == INVALID
    layer, _ = drop[1], None
    if drop[0] != "final_proj_w16":
        assert lib.gfc_lg_layer(ctypes.byref(p), layer, f(1), f(2), f(3), 8, f(4), f(5), 2, 4, f(6), ws, None) == INVALID
    else:
        assert lib.gfc_lg_assign(ctypes.byref(p), layer, f(1), f(2), 1, 4, 4, 0.1, f(3), f(4), f(5), f(6), f(7), f(8),
                                 ws, None) == INVALID


def test_unknown_precision_is_invalid():
    lib = nat.lib()
    p = _fp16_params()
    p.precision = 2
    f = _fake
    ws = 1 << 30
    assert lib.gfc_lg_forward_packed(ctypes.byref(p), f(1), f(2), f(3), f(4), None, 1, 4, 4, 0.1, f(5), f(6), f(7), f(8),
                                     f(9), f(10), f(11), ws, None, None) == INVALID
    assert lib.gfc_lg_layer(ctypes.byref(p), 0, f(1), f(2), f(3), 8, f(4), f(5), 2, 4, f(6), ws, None) == INVALID
    assert lib.gfc_lg_assign(ctypes.byref(p), 0, f(1), f(2), 1, 4, 4, 0.1, f(3), f(4), f(5), f(6), f(7), f(8), ws,
                             None) == INVALID
