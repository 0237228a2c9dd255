"""The Python binding is derived from include/gfc_amd.h (no GPU, nothing launched).

Pinned here: the declaration parser against hand-written answers for one function of every scalar kind and pointer
form; the four structure layouts against what a C++ compiler makes of the same header; what `nat.call` refuses before
the library is entered; and that host-arithmetic functions give the same values through `call` as through `lib()`.
"""
import ctypes
import importlib.util
import os
import subprocess
from unittest import mock

import pytest
import torch

from glue_factory_colon_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = {
    "gfc_version": ("const char*", []),
    "gfc_event_create": ("int", [("event", "void**")]),
    "gfc_batched_nt": ("int", [
        ("A", "const float*"), ("lda", "int"), ("strideA", "long long"), ("Bm", "const float*"), ("ldb", "int"),
        ("strideB", "long long"), ("Y", "float*"), ("ldy", "int"), ("strideY", "long long"), ("M", "int"), ("N", "int"),
        ("K", "int"), ("batch", "int"), ("stream", "void*")]),
    "gfc_nn_match": ("int", [
        ("desc0", "const float*"), ("desc1", "const float*"), ("B", "int"), ("M", "int"), ("N", "int"), ("D", "int"),
        ("ratio_thresh", "double"), ("distance_thresh", "double"), ("mutual", "int"), ("m0", "int64_t*"),
        ("m1", "int64_t*"), ("ms0", "float*"), ("ms1", "float*"), ("sim", "float*"), ("log_assignment", "float*"),
        ("ws", "void*"), ("ws_bytes", "size_t"), ("stream", "void*")]),
    "gfc_sp_pad_keypoints": ("int", [
        ("kpts", "float*"), ("kscores", "float*"), ("counts", "const int32_t*"), ("B", "int"), ("cap", "int"),
        ("k", "int"), ("low", "float"), ("sizes", "const float*"), ("n_sizes", "int"), ("high_fallback", "float"),
        ("seed", "unsigned int"), ("stream", "void*")]),
    "gfc_eval_homography_ransac": ("int", [
        ("kp0", "const float*"), ("kp1", "const float*"), ("m0", "const int64_t*"), ("stream_id", "const int64_t*"),
        ("H_gt", "const float*"), ("image_size0", "const float*"), ("B", "int"), ("M", "int"), ("N", "int"),
        ("thresholds", "const float*"), ("T", "int"), ("num_hypotheses", "int"), ("lo_iters", "int"),
        ("seed", "uint64_t"), ("H_out", "double*"), ("inliers", "uint8_t*"), ("num_inliers", "int32_t*"),
        ("success", "uint8_t*"), ("best_hypothesis", "int32_t*"), ("H_minimal", "double*"), ("err_out", "float*"),
        ("ws", "void*"), ("ws_bytes", "size_t"), ("stream", "void*")]),
    "gfc_lg_forward_ragged": ("int", [
        ("p", "const gfc_lg_params*"), ("kpts", "const float*"), ("desc", "const float*"), ("size0", "const float*"),
        ("size1", "const float*"), ("scale_ori", "const float*"), ("B", "int"), ("m", "const int32_t*"),
        ("n", "const int32_t*"), ("threshold", "float"), ("m0", "int64_t*"), ("m1", "int64_t*"), ("ms0", "float*"),
        ("ms1", "float*"), ("log_assignment", "float*"), ("rows", "float*"), ("ws", "void*"), ("ws_bytes", "size_t"),
        ("attention_trace", "gfc_trace*"), ("stream", "void*")]),
    "gfc_sift_extract": ("int", [
        ("image", "const float*"), ("B", "int"), ("H", "int"), ("W", "int"), ("valid_wh", "const int32_t*"),
        ("specular", "const unsigned char*"), ("first_octave", "int"), ("num_octaves", "int"),
        ("detection_threshold", "double"), ("edge_threshold", "double"), ("cap", "int"), ("ocap", "int"),
        ("nms_radius", "int"), ("scale_weighting", "int"), ("k", "int"), ("rootsift", "int"), ("out_cap", "int"),
        ("kpts", "float*"), ("scales", "float*"), ("oris", "float*"), ("scores", "float*"), ("desc_out", "float*"),
        ("index", "int32_t*"), ("counts_out", "int32_t*"), ("counts", "int32_t*"), ("ocounts", "int32_t*"),
        ("ws", "void*"), ("ws_bytes", "size_t"), ("stream", "void*")]),
}
KNOWN_CTYPES = {
    "gfc_version": (ctypes.c_char_p, []),
    "gfc_event_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p)]),
    "gfc_batched_nt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong] * 3 + [ctypes.c_int] * 4
                       + [ctypes.c_void_p]),
    "gfc_sp_pad_keypoints": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [
        ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint, ctypes.c_void_p]),
}


def test_parser_known_answers():
    assert len(nat.FUNCTIONS) == len(nat.SIGNATURES) == 101 and len(KNOWN["gfc_sift_extract"][1]) == 29
    for name, expected in KNOWN.items():
        assert nat.FUNCTIONS[name] == expected, name
    for name, expected in KNOWN_CTYPES.items():
        assert nat.SIGNATURES[name] == expected, name
    rag = nat.SIGNATURES["gfc_lg_forward_ragged"][1]
    assert rag[0] == ctypes.POINTER(nat.LgParams) and rag[-2] == ctypes.POINTER(nat.Trace)
    assert rag[7] is ctypes.c_void_p and nat.SIGNATURES["gfc_nn_match"][1][6] is ctypes.c_double
    ransac = nat.SIGNATURES["gfc_eval_homography_ransac"]
    assert ransac[1][13] is ctypes.c_uint64 and ransac[1][9] is ctypes.c_void_p and ransac[1][22] is ctypes.c_size_t
    assert nat.SIGNATURES["gfc_sp_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)


def test_parser_constants_and_structs():
    assert len(nat.CONSTANTS) == 26 and all(getattr(nat, k) == v for k, v in nat.CONSTANTS.items())
    assert nat.STATUS == {0: "GFC_OK", 1: "GFC_ERR_INVALID", 2: "GFC_ERR_WORKSPACE", 3: "GFC_ERR_UNSUPPORTED",
                          4: "GFC_ERR_LAUNCH"}
    assert (nat.GFC_LG_MAX_LAYERS, nat.GFC_SG_MAX_LAYERS, nat.GFC_LG_MAX_RAGGED_PAIRS) == (16, 32, 128)
    assert (nat.GFC_SAMPLE_OPEN, nat.GFC_SAMPLE_LEGACY, nat.GFC_SAMPLE_FIXED) == (0, 1, 2)
    assert (nat.GFC_CAM_PINHOLE, nat.GFC_CAM_RADIAL, nat.GFC_CAM_OPENCV, nat.GFC_CAM_OPENCV_FISHEYE) == (0, 1, 2, 3)
    assert (nat.GFC_RS_F32_CHW, nat.GFC_RS_U8_HWC, nat.GFC_RS_U8_PLANE, nat.GFC_RS_BITS) == (0, 1, 2, 3)
    assert (nat.GFC_RS_NEAREST, nat.GFC_RS_AREA, nat.GFC_LG_FP32, nat.GFC_LG_FP16) == (0, 1, 0, 1)
    assert (nat.GFC_LG_ADAPTIVE_LIVE, nat.GFC_LG_ADAPTIVE_STOPPED, nat.GFC_LG_ADAPTIVE_EMPTIED) == (0, 1, 2)
    assert nat.STRUCTS["gfc_trace"] == [("start", "void**", None), ("stop", "void**", None), ("capacity", "int", None),
                                        ("count", "int", None)]
    sg = dict((f, (t, n)) for f, t, n in nat.STRUCTS["gfc_sg_params"])
    assert sg["cross"] == ("int", 32) and sg["kenc_scale"] == ("const float*", 4) and sg["bin_score"] == ("float", None)
    assert dict(nat.SgParams._fields_)["cross"] is ctypes.c_int * 32
    assert dict(nat.LgParams._fields_)["wqkv16"] is ctypes.c_void_p * 16
    assert dict(nat.Trace._fields_)["start"] is ctypes.POINTER(ctypes.c_void_p)
    # the per-layer name lists, by declared type: 20 block arrays + 6 head arrays in fp32, the 9 fp16 copies
    assert nat._LG_ARRAYS[0] == "wqkv" and nat._LG_ARRAYS[19] == "c_ffn3_b" and nat._LG_ARRAYS[20:] == [
        "final_proj_w", "final_proj_b", "matchability_w", "matchability_b", "token_w", "token_b"]
    assert nat._LG_ARRAYS_F16 == ["wqkv16", "s_out_w16", "s_ffn0_w16", "s_ffn3_w16", "c_qkv_w16", "c_out_w16",
                                  "c_ffn0_w16", "c_ffn3_w16", "final_proj_w16"]
    assert nat._SG_ARRAYS == ["wqkv", "bqkv", "merge_w", "merge_b", "mlp0_w", "mlp0_b", "mlp_scale", "mlp_shift",
                              "mlp1_w", "mlp1_b"]


@pytest.mark.parametrize("snippet", [
    "int gfc_f(int (*callback)(int), void* stream);",      # function pointer
    "int gfc_f(int a, ...);",                               # variadic
    "struct gfc_s { int a; };",                             # struct without typedef
    "typedef struct { int a : 3; } gfc_s;",                 # bit field
    "typedef struct { struct { int a; } in; } gfc_s;",      # nested struct
    "#define GFC_X (1 << 4)",                               # constant expression
    "typedef enum { GFC_A, GFC_B } gfc_e;",                 # implicit enum values
    "static inline int gfc_f(int a) { return a; }",         # definition
    "int gfc_f(int);",                                      # unnamed parameter
    "extern int gfc_global;",                               # variable
    "// a line comment\nint gfc_f(int a);",                 # comment form the header does not use
    "}",                                                    # a brace outside the extern "C" guard
    "#ifdef GFC_EXTRA\nint gfc_g(int a);\n#endif",          # a conditional declaration
    "typedef struct { const float* w[GFC_UNKNOWN]; } gfc_s;",  # an array length that is not defined
])
def test_parser_raises_outside_its_grammar(snippet):
    with pytest.raises(nat.NativeError, match="cannot parse"):
        nat.parse_header("int gfc_ok(int a);\n" + snippet + "\nint gfc_after(int b);\n")


def test_parser_accepts_the_forms_of_the_header():
    funcs, structs, enums, consts = nat.parse_header(
        '#ifndef GFC_AMD_H\n#define GFC_AMD_H\n#include <stddef.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
        "/* a comment; with int f(void); inside */\n#define GFC_N 3\n"
        "typedef enum { GFC_A = 0, GFC_B = 5 /* five */ } gfc_e;\nenum { GFC_C = 7 };\n"
        "typedef struct {\n  const float* w[GFC_N]; /* [3] */\n  int n;\n} gfc_s;\n"
        "size_t gfc_bytes(const gfc_s* p,\n                 unsigned int seed);\n"
        "#ifdef __cplusplus\n}\n#endif\n#endif /* GFC_AMD_H */\n")
    assert funcs == {"gfc_bytes": ("size_t", [("p", "const gfc_s*"), ("seed", "unsigned int")])}
    assert structs == {"gfc_s": [("w", "const float*", 3), ("n", "int", None)]}
    assert enums == {"gfc_e": {"GFC_A": 0, "GFC_B": 5}, "": {"GFC_C": 7}}
    assert consts == {"GFC_N": 3, "GFC_A": 0, "GFC_B": 5, "GFC_C": 7}


def test_missing_header_raises(monkeypatch):
    monkeypatch.setattr(nat, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(nat.NativeError, match="no_such_header.h not found"):
        nat._load_header()


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof / offsetof of every field, from a host-only program compiled against the header."""
    spec = importlib.util.spec_from_file_location("gfc_build", os.path.join(ROOT, "glue-factory-colon_amd", "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "gfc_amd.h"', "int main() {"]
    for cname, fields in nat.STRUCTS.items():
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  std::printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));'
                  for f, _, _ in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([build._hipcc(), "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    compiled = {k: tuple(int(x) for x in v.split()) for k, v in
                (line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
                 .stdout.splitlines())}
    classes = {"gfc_sp_params": nat.SpParams, "gfc_lg_params": nat.LgParams, "gfc_sg_params": nat.SgParams,
               "gfc_trace": nat.Trace}
    assert set(classes) == set(nat.STRUCTS)
    mine = {}
    for cname, cls in classes.items():
        mine[cname] = (ctypes.sizeof(cls),)
        assert [f for f, _ in cls._fields_] == [f for f, _, _ in nat.STRUCTS[cname]]
        for f, _ in cls._fields_:
            mine[f"{cname}.{f}"] = (getattr(cls, f).offset, getattr(cls, f).size)
    assert mine == compiled
    assert [mine[c][0] for c in ("gfc_sp_params", "gfc_lg_params", "gfc_sg_params", "gfc_trace")] == [440, 4536, 2864, 24]


# ---------------------------------------------------------------------------------------------- nat.call refusals
def _tensor(dtype=torch.float32, device="cuda:0", contiguous=True):
    """Stands in for a device tensor, which a host without a GPU cannot make: `convert` reads only device, dtype,
    contiguity and address, and those are set by hand here.  So these tests pin which refusal `convert` raises and
    its wording, not how a real tensor reports itself; real CPU and meta tensors are used where they can be, and real
    device tensors pass through `convert` at every call site in the GPU suite."""
    t = mock.MagicMock(spec=torch.Tensor)
    t.device, t.dtype = torch.device(device), dtype
    t.is_contiguous.return_value = contiguous
    t.stride.return_value = (2, 1) if contiguous else (1, 7)
    t.data_ptr.return_value = 0x1000
    return t


@pytest.fixture()
def no_library(monkeypatch):
    """Entering the library fails the test: every refusal below has to come first."""
    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(nat, "lib", entered)


def _nms_args(**kw):
    args = dict(heatmap=_tensor(), B=1, H=8, W=8, radius=3, border=0, valid_wh=_tensor(torch.int32), out=_tensor())
    args.update(kw)
    return list(args.values())


def test_call_refuses_a_wrong_dtype(no_library):
    with pytest.raises(nat.NativeError, match=r"gfc_sp_nms: 'valid_wh' is declared const int32_t\* and needs "
                                              r"torch.int32, got torch.int64"):
        nat.call("gfc_sp_nms", *_nms_args(valid_wh=_tensor(torch.int64)))
    with pytest.raises(nat.NativeError, match=r"'heatmap' is declared const float\* and needs torch.float32, got "
                                              r"torch.float16"):
        nat.call("gfc_sp_nms", *_nms_args(heatmap=_tensor(torch.float16)))
    with pytest.raises(nat.NativeError, match=r"'H_out' is declared double\* and needs torch.float64"):
        nat.convert("gfc_eval_homography_ransac", [None] * 14 + [_tensor()] + [None] * 8)
    with pytest.raises(nat.NativeError, match=r"'m0' is declared const int64_t\* and needs torch.int64"):
        nat.convert("gfc_eval_homography_ransac", [None, None, _tensor(torch.int32)] + [None] * 20)
    with pytest.raises(nat.NativeError, match="'B' is declared int, got a tensor"):
        nat.call("gfc_sp_nms", *_nms_args(B=_tensor(torch.int32)))
    with pytest.raises(nat.NativeError, match=r"'p' is declared const gfc_sp_params\*, got a tensor"):
        nat.convert("gfc_sp_dense", [_tensor()] + [None] * 10)


def test_call_accepts_what_the_pointee_names():
    mask = dict(scores=_tensor(), B=1, H=8, W=8, mask=_tensor(torch.bool), Hm=8, Wm=8, image_wh=None)
    assert nat.convert("gfc_sp_mask_scores", list(mask.values())) == ([0x1000, 1, 8, 8, 0x1000, 8, 8, None],
                                                                      torch.device("cuda:0"))
    mask["mask"] = _tensor(torch.uint8)
    nat.convert("gfc_sp_mask_scores", list(mask.values()))
    for dtype in (torch.float16, torch.float32, torch.uint8, torch.bool):  # const void* src: any dtype
        nat.convert("gfc_preprocess_resize", [_tensor(dtype), 0, 0, 1, 1, 8, 8, _tensor(), 4, 4, 0, 1])
    host = (ctypes.c_int32 * 2)(4, 5)  # host arrays, byref and raw addresses pass through
    out, device = nat.convert("gfc_lg_ragged_workspace_bytes", [2, host, host])
    assert out[1] is host and device is None


def test_call_refuses_layout_and_device(no_library):
    with pytest.raises(nat.NativeError, match=r"gfc_sp_nms: 'out' \(float\*\) must be contiguous"):
        nat.call("gfc_sp_nms", *_nms_args(out=_tensor(contiguous=False)))
    with pytest.raises(nat.NativeError, match=r"gfc_sp_nms: 'heatmap' \(const float\*\) is on cpu"):
        nat.call("gfc_sp_nms", *_nms_args(heatmap=torch.zeros(1, 8, 8)))
    with pytest.raises(nat.NativeError, match=r"'out' \(float\*\) is on meta"):
        nat.call("gfc_sp_nms", *_nms_args(out=torch.zeros(1, 8, 8, device="meta")))
    with pytest.raises(nat.NativeError, match=r"gfc_sp_nms: 'out' \(float\*\) is on cuda:1, earlier tensors are on "
                                              r"cuda:0"):
        nat.call("gfc_sp_nms", *_nms_args(out=_tensor(device="cuda:1")))


def test_call_refuses_a_wrong_argument_count(no_library):
    args = _nms_args()
    with pytest.raises(nat.NativeError, match=r"gfc_sp_nms takes 8 arguments \(heatmap, B, H, W, radius, border, "
                                              r"valid_wh, out\), got 7"):
        nat.call("gfc_sp_nms", *args[:-1])
    with pytest.raises(nat.NativeError, match="takes 8 arguments .* got 9"):  # the stream is not the caller's to pass
        nat.call("gfc_sp_nms", *args, None)
    with pytest.raises(nat.NativeError, match="gfc_version takes 0 arguments"):
        nat.call("gfc_version", 1)


def test_call_equals_lib_on_host_arithmetic():
    lib = nat.lib()
    assert nat.call("gfc_version") == lib.gfc_version() and b"gfx950" in nat.call("gfc_version")
    for args in ((2, 65, 130), (1, 1, 1), (0, 4, 4)):
        assert nat.call("gfc_lg_packed_workspace_bytes", *args) == lib.gfc_lg_packed_workspace_bytes(*args)
    assert nat.call("gfc_lg_packed_workspace_bytes", 2, 65, 130) > 0
    m, n = (ctypes.c_int32 * 2)(4, 5), (ctypes.c_int32 * 2)(6, 7)
    assert nat.call("gfc_lg_ragged_workspace_bytes", 2, m, n) == lib.gfc_lg_ragged_workspace_bytes(2, m, n) > 0
    out = (ctypes.c_int64 * 35)()
    assert nat.call("gfc_sift_pyramid_layout", 64, 64, 0, 2, out) is None and out[0] == 2
    with pytest.raises(nat.NativeError, match="gfc_sift_pyramid_layout failed: GFC_ERR_UNSUPPORTED"):
        nat.call("gfc_sift_pyramid_layout", 64, 64, 3, 2, out)
    ms = ctypes.c_float()  # byref where the header says float*: as bench.py calls gfc_probe_mfma_peak
    with pytest.raises(nat.NativeError, match="gfc_event_elapsed_ms failed: GFC_ERR_INVALID"):
        nat.call("gfc_event_elapsed_ms", None, None, ctypes.byref(ms))
