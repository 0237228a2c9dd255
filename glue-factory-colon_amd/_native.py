"""ctypes binding of libgfc_amd.so (the C ABI declared in include/gfc_amd.h and, for the validation pass,
include/gfc_amd_validation.h, include/gfc_amd_sparse_map.h and include/gfc_amd_dense_warp.h; for the cross attention with
the score matrix evaluated once, include/gfc_amd_cross_attention.h; for the per-layer scores of the deep-supervision loss,
include/gfc_amd_layer_scores.h; for the head and exit-token gradients, include/gfc_amd_head_backward.h; for the FFN-block
backward and the last layer's kept tensors, include/gfc_amd_ffn_backward.h; for the cross-attention backward,
include/gfc_amd_cross_attn_backward.h; for the self-attention backward and the layer that keeps the self attention's
context, include/gfc_amd_self_attn_backward.h).

The library is the product: if it is missing or a call fails, this module raises --
there is no PyTorch / CPU fallback for any arithmetic on the path.
"""
import ctypes
import os
import re
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_uint64,
                    c_void_p)

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# GFC_AMD_LIB: another build of the same library (same-box A/B of kernel variants: tools/ab_build.sh)
LIB_PATH = os.environ.get("GFC_AMD_LIB") or os.path.join(_PKG, "libgfc_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd.h")
VALIDATION_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_validation.h")
SPARSE_MAP_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_sparse_map.h")
DENSE_WARP_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_dense_warp.h")
CROSS_ATTENTION_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_cross_attention.h")
LAYER_SCORES_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_layer_scores.h")
HEAD_BACKWARD_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_head_backward.h")
FFN_BACKWARD_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_ffn_backward.h")
CROSS_ATTN_BACKWARD_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_cross_attn_backward.h")
SELF_ATTN_BACKWARD_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "gfc_amd_self_attn_backward.h")


class NativeError(RuntimeError):
    pass


# ---- the header is the single source: functions, structs and constants are parsed from it ----
_TYPE = r"(?:const\s+)?(?:unsigned\s+int|unsigned\s+char|long\s+long|\w+)\s*\**"
_DECL = re.compile(r"""\s*(?:
      \#\s*define\s+(?P<def>GFC_\w+)[ \t]+(?P<defval>-?\d+)[ \t]*$
    | \#\s*ifdef\s+__cplusplus\s+(?:extern\s+"C"\s*\{|\})\s+\#\s*endif\b[^\n]*$
    | \#\s*(?:ifndef|endif|include|define\s+GFC_AMD(?:_\w+)?_H\b)[^\n]*$
    | (?:typedef\s+)?enum\s*\{(?P<enum>[^{}]*)\}\s*(?P<ename>\w*)\s*;
    | typedef\s+struct\s*\{(?P<fields>[^{}]*)\}\s*(?P<sname>\w+)\s*;
    | (?P<ret>%s)\s*\b(?P<fname>gfc_\w+)\s*\((?P<params>[^()]*)\)\s*;
    )""" % _TYPE, re.X | re.M)
_VAR = re.compile(r"\s*(?P<type>%s)\s*\b(?P<name>\w+)\s*(?:\[\s*(?P<len>\w+)\s*\])?\s*$" % _TYPE)


def _var(text, consts, what):
    m = _VAR.match(text)
    if m is None:
        raise NativeError(f"{HEADER_PATH}: cannot parse {what} '{text.strip()}'")
    ctype = re.sub(r"\s*\*", "*", " ".join(m["type"].split()))
    n = m["len"]
    if n is not None and not n.isdigit() and n not in consts:
        raise NativeError(f"{HEADER_PATH}: cannot parse {what} '{text.strip()}': {n} is not defined before it")
    return m["name"], ctype, (None if n is None else int(n) if n.isdigit() else consts[n])


def parse_header(text):
    """The declarations of include/gfc_amd.h: functions {name: (return type, [(parameter, C type)])}, structs
    {name: [(field, C type, array length or None)]}, enums {typedef name: {member: value}} and every integer constant
    (#define and enum member).  Only the forms that header uses; anything else raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    funcs, structs, enums, consts, pos = {}, {}, {}, {}, 0
    while text[pos:].strip():
        m = _DECL.match(text, pos)
        if m is None:
            raise NativeError(f"{HEADER_PATH}: cannot parse the declaration at '{text[pos:].strip()[:80]}'")
        pos = m.end()
        if m["def"]:
            consts[m["def"]] = int(m["defval"])
        elif m["enum"] is not None:
            members = {}
            for item in m["enum"].split(","):
                k = re.fullmatch(r"\s*(GFC_\w+)\s*=\s*(-?\d+)\s*", item)
                if k is None:
                    raise NativeError(f"{HEADER_PATH}: cannot parse the enum member '{item.strip()}'")
                members[k[1]] = int(k[2])
            enums[m["ename"]] = members
            consts.update(members)
        elif m["sname"]:
            structs[m["sname"]] = [_var(f, consts, "the field") for f in m["fields"].split(";") if f.strip()]
        elif m["fname"]:
            params = [] if m["params"].strip() == "void" else [_var(p, consts, "the parameter")[:2]
                                                               for p in m["params"].split(",")]
            funcs[m["fname"]] = (_var(m["ret"] + " _", consts, "the return type")[1], params)
    return funcs, structs, enums, consts


def _load_header():
    if not os.path.exists(HEADER_PATH):
        raise NativeError(f"{HEADER_PATH} not found: the binding is derived from the C header")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


FUNCTIONS, STRUCTS, ENUMS, CONSTANTS = _load_header()


def _load_functions_header(path, known):
    """The functions of a header that declares functions only and takes its types from gfc_amd.h (same library, same
    grammar); `known`: the functions declared before it."""
    if not os.path.exists(path):
        raise NativeError(f"{path} not found: the binding is derived from the C headers")
    with open(path) as f:
        funcs, structs, enums, consts = parse_header(f.read())
    if structs or enums or consts or set(funcs) & set(known):
        raise NativeError(f"{path}: only new function declarations belong there")
    return funcs


def _load_validation_header():
    """include/gfc_amd_validation.h: the validation pass."""
    return _load_functions_header(VALIDATION_HEADER_PATH, FUNCTIONS)


VALIDATION_FUNCTIONS = _load_validation_header()
# include/gfc_amd_sparse_map.h: ground-truth labels from Endomapper sparse maps
SPARSE_MAP_FUNCTIONS = _load_functions_header(SPARSE_MAP_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS})
# include/gfc_amd_dense_warp.h: ground-truth labels from dense warps (RoMa)
DENSE_WARP_FUNCTIONS = _load_functions_header(DENSE_WARP_HEADER_PATH,
                                              {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS})
# include/gfc_amd_cross_attention.h: cross attention with the score matrix evaluated once
CROSS_ATTENTION_FUNCTIONS = _load_functions_header(
    CROSS_ATTENTION_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS})
# include/gfc_amd_layer_scores.h: per-layer agreement, token BCE and confident counts
LAYER_SCORES_FUNCTIONS = _load_functions_header(
    LAYER_SCORES_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS,
                               **CROSS_ATTENTION_FUNCTIONS})
# include/gfc_amd_head_backward.h: gradients of the assignment heads and exit tokens
HEAD_BACKWARD_FUNCTIONS = _load_functions_header(
    HEAD_BACKWARD_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS,
                                **CROSS_ATTENTION_FUNCTIONS, **LAYER_SCORES_FUNCTIONS})
# include/gfc_amd_ffn_backward.h: the FFN-block backward and the layer that keeps what it starts from
FFN_BACKWARD_FUNCTIONS = _load_functions_header(
    FFN_BACKWARD_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS,
                               **CROSS_ATTENTION_FUNCTIONS, **LAYER_SCORES_FUNCTIONS, **HEAD_BACKWARD_FUNCTIONS})
# include/gfc_amd_cross_attn_backward.h: the cross-attention backward and the to_qk / to_v gradients around it
CROSS_ATTN_BACKWARD_FUNCTIONS = _load_functions_header(
    CROSS_ATTN_BACKWARD_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS,
                                      **CROSS_ATTENTION_FUNCTIONS, **LAYER_SCORES_FUNCTIONS, **HEAD_BACKWARD_FUNCTIONS,
                                      **FFN_BACKWARD_FUNCTIONS})
# include/gfc_amd_self_attn_backward.h: the self-attention backward, the Wqkv gradients around it, the kept self context
SELF_ATTN_BACKWARD_FUNCTIONS = _load_functions_header(
    SELF_ATTN_BACKWARD_HEADER_PATH, {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS,
                                     **CROSS_ATTENTION_FUNCTIONS, **LAYER_SCORES_FUNCTIONS, **HEAD_BACKWARD_FUNCTIONS,
                                     **FFN_BACKWARD_FUNCTIONS, **CROSS_ATTN_BACKWARD_FUNCTIONS})
globals().update(CONSTANTS)  # GFC_LG_MAX_LAYERS, GFC_LG_FP16, GFC_CAM_RADIAL, GFC_RS_AREA, ...
STATUS = {v: k for k, v in ENUMS["gfc_status"].items()}

_SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "long long": c_longlong,
            "unsigned int": c_uint, "uint64_t": c_uint64}
_CLASSES = {}  # C struct name -> ctypes.Structure


def _ctype(ctype):
    """Scalars as themselves, struct pointers and void** typed, every data pointer a c_void_p."""
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if not ctype.endswith("*"):
        raise NativeError(f"{HEADER_PATH}: no ctypes mapping for '{ctype}'")
    pointee = ctype[:-1].replace("const ", "")
    if pointee in _CLASSES:
        return POINTER(_CLASSES[pointee])
    return POINTER(c_void_p) if pointee == "void*" else c_void_p


def _structure(cname):
    fields = [(f, _ctype(t) if n is None else _ctype(t) * n) for f, t, n in STRUCTS[cname]]
    _CLASSES[cname] = type("".join(w.capitalize() for w in cname[4:].split("_")), (Structure,), {"_fields_": fields})
    return _CLASSES[cname]


SpParams, Trace, LgParams, SgParams = map(_structure, ("gfc_sp_params", "gfc_trace", "gfc_lg_params", "gfc_sg_params"))
assert set(_CLASSES) == set(STRUCTS), "a struct of the header has no class here"


def _layer_arrays(cname, length, ctype):
    """The fields of a parameter struct that hold one `ctype` per layer, in the header's order."""
    return [f for f, t, n in STRUCTS[cname] if n == length and t == ctype]


# For code outside the package that fills a parameter struct field by field: the per-layer fp32 arrays of LightGlue,
# its fp16 copies (declared const void*) and SuperGlue's per-layer arrays, by declared type -- no list is kept here.
_LG_ARRAYS = _layer_arrays("gfc_lg_params", GFC_LG_MAX_LAYERS, "const float*")  # noqa: F821
_LG_ARRAYS_F16 = _layer_arrays("gfc_lg_params", GFC_LG_MAX_LAYERS, "const void*")  # noqa: F821
_SG_ARRAYS = _layer_arrays("gfc_sg_params", GFC_SG_MAX_LAYERS, "const float*")  # noqa: F821

def _signatures(functions):
    return {name: (c_char_p if ret == "const char*" else _ctype(ret), [_ctype(t) for _, t in params])
            for name, (ret, params) in functions.items()}


# name -> (restype, argtypes); every symbol declared in include/gfc_amd.h
SIGNATURES = _signatures(FUNCTIONS)
VALIDATION_SIGNATURES = _signatures(VALIDATION_FUNCTIONS)  # include/gfc_amd_validation.h
SPARSE_MAP_SIGNATURES = _signatures(SPARSE_MAP_FUNCTIONS)  # include/gfc_amd_sparse_map.h
DENSE_WARP_SIGNATURES = _signatures(DENSE_WARP_FUNCTIONS)  # include/gfc_amd_dense_warp.h
CROSS_ATTENTION_SIGNATURES = _signatures(CROSS_ATTENTION_FUNCTIONS)  # include/gfc_amd_cross_attention.h
LAYER_SCORES_SIGNATURES = _signatures(LAYER_SCORES_FUNCTIONS)  # include/gfc_amd_layer_scores.h
HEAD_BACKWARD_SIGNATURES = _signatures(HEAD_BACKWARD_FUNCTIONS)  # include/gfc_amd_head_backward.h
FFN_BACKWARD_SIGNATURES = _signatures(FFN_BACKWARD_FUNCTIONS)  # include/gfc_amd_ffn_backward.h
CROSS_ATTN_BACKWARD_SIGNATURES = _signatures(CROSS_ATTN_BACKWARD_FUNCTIONS)  # include/gfc_amd_cross_attn_backward.h
SELF_ATTN_BACKWARD_SIGNATURES = _signatures(SELF_ATTN_BACKWARD_FUNCTIONS)  # include/gfc_amd_self_attn_backward.h
_ALL_FUNCTIONS = {**FUNCTIONS, **VALIDATION_FUNCTIONS, **SPARSE_MAP_FUNCTIONS, **DENSE_WARP_FUNCTIONS,
                  **CROSS_ATTENTION_FUNCTIONS, **LAYER_SCORES_FUNCTIONS, **HEAD_BACKWARD_FUNCTIONS,
                  **FFN_BACKWARD_FUNCTIONS, **CROSS_ATTN_BACKWARD_FUNCTIONS, **SELF_ATTN_BACKWARD_FUNCTIONS}

_DTYPES = {"float": (torch.float32,), "int32_t": (torch.int32,), "int": (torch.int32,), "int64_t": (torch.int64,),
           "double": (torch.float64,), "uint8_t": (torch.uint8, torch.bool), "unsigned char": (torch.uint8, torch.bool),
           "void": None}


def _call_spec(params):
    """([(parameter, C type, dtypes a tensor may have there)] without a trailing `void* stream`, whether there is one).
    The dtypes: () = no tensor (scalar, struct pointer, void**), None = any (void*), else those of the pointee."""
    has_stream = params[-1:] == [("stream", "void*")]
    return [(p, t, _DTYPES.get(t[:-1].replace("const ", ""), ()) if t.endswith("*") else ())
            for p, t in (params[:-1] if has_stream else params)], has_stream


_CALLS = {name: _call_spec(params) for name, (_, params) in _ALL_FUNCTIONS.items()}

_lib = None


def convert(name, args):
    """Check `args` against the header's parameters of `name` (the stream left out) and turn tensors into device
    addresses.  Returns (arguments, device of the tensors or None).  No library call: a violation raises first."""
    params, _ = _CALLS[name]
    if len(args) != len(params):
        raise NativeError(f"{name} takes {len(params)} arguments ({', '.join(p for p, _, _ in params)}), got {len(args)}")
    out, device = [], None
    for a, (pname, ctype, rule) in zip(args, params):
        if isinstance(a, torch.Tensor):
            if rule == ():
                raise NativeError(f"{name}: '{pname}' is declared {ctype}, got a tensor")
            d = a.device
            if d.type != "cuda":
                raise NativeError(f"{name}: '{pname}' ({ctype}) is on {d}; it must be on a 'cuda' (ROCm) device")
            if device is None:
                device = d
            elif d != device:
                raise NativeError(f"{name}: '{pname}' ({ctype}) is on {d}, earlier tensors are on {device}")
            if rule is not None and a.dtype not in rule:
                raise NativeError(f"{name}: '{pname}' is declared {ctype} and needs {' or '.join(map(str, rule))}, "
                                  f"got {a.dtype}")
            if not a.is_contiguous():
                raise NativeError(f"{name}: '{pname}' ({ctype}) must be contiguous, got strides {tuple(a.stride())}")
            a = a.data_ptr()
        out.append(a)
    return out, device


def call(name, *args, device=None):
    """One checked native call: tensors are verified against the header (device, dtype, contiguity), a trailing
    `void* stream` is filled in with the current stream of their device (of `device` without tensors), a non-zero
    gfc_status raises; size_t and const char* results are returned."""
    converted, dev = convert(name, args)
    if _CALLS[name][1]:
        converted.append(torch.cuda.current_stream(dev if dev is not None else device).cuda_stream)
    result = getattr(lib(), name)(*converted)
    if _ALL_FUNCTIONS[name][0] != "int":
        return result
    if result != 0:
        raise NativeError(f"{name} failed: {STATUS.get(result, result)}")


def lib():
    """Load libgfc_amd.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} not found: build it with `python glue-factory-colon_amd/csrc/build.py` "
                "(or __graft_entry__.build()).  There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **VALIDATION_SIGNATURES, **SPARSE_MAP_SIGNATURES,
                                  **DENSE_WARP_SIGNATURES, **CROSS_ATTENTION_SIGNATURES,
                                  **LAYER_SCORES_SIGNATURES, **HEAD_BACKWARD_SIGNATURES,
                                  **FFN_BACKWARD_SIGNATURES, **CROSS_ATTN_BACKWARD_SIGNATURES,
                                  **SELF_ATTN_BACKWARD_SIGNATURES}.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status: int, what: str):
    if status != 0:
        raise NativeError(f"{what} failed: {STATUS.get(status, status)}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor must be contiguous fp32/int32/int64."""
    if t is None:
        return None
    assert t.is_contiguous(), "native calls need contiguous tensors"
    return c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_cuda(t: torch.Tensor, name: str):
    if t.device.type != "cuda":
        raise NativeError(f"{name} is on {t.device}: the MI355X path needs tensors on a 'cuda' (ROCm) device; "
                          "there is no CPU implementation in this package")


class Workspace:
    """Grow-only device scratch buffer (torch-allocated, passed to the library as void*)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes: int, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf


class KernelTrace:
    """Host-side owner of a gfc_trace: `capacity` hipEvent pairs recorded by the library around
    the launches of the dominant kernel (see include/gfc_amd.h)."""

    def __init__(self, capacity: int):
        l = lib()
        self.capacity = capacity
        self.starts = (c_void_p * capacity)()
        self.stops = (c_void_p * capacity)()
        for arr in (self.starts, self.stops):
            for i in range(capacity):
                ev = c_void_p()
                check(l.gfc_event_create(ctypes.byref(ev)), "gfc_event_create")
                arr[i] = ev
        self.c = Trace(ctypes.cast(self.starts, POINTER(c_void_p)), ctypes.cast(self.stops, POINTER(c_void_p)),
                       capacity, 0)

    def reset(self):
        self.c.count = 0

    def durations_ms(self):
        """Call after a device synchronisation."""
        l = lib()
        out = []
        for i in range(self.c.count):
            ms = c_float()
            check(l.gfc_event_elapsed_ms(self.starts[i], self.stops[i], ctypes.byref(ms)), "gfc_event_elapsed_ms")
            out.append(ms.value)
        return out

    def close(self):
        l = lib()
        for arr in (self.starts, self.stops):
            for i in range(self.capacity):
                if arr[i]:
                    l.gfc_event_destroy(arr[i])
                    arr[i] = None
