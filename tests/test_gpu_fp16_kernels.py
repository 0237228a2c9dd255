"""gfc_linear_f16, gfc_batched_nt_f16 and gfc_attention_f16 on the MI355X against the cases of
tests/fp16_kernel_cases.py, through the C ABI, in the call forms the fp16 matcher makes.

Exact cases are equality assertions (output and NaN canaries); bounded cases use only the per-element formulas of
fp16_kernel_cases and record their worst error / tolerance ratio with parity_utils.record.
tests/test_fp16_kernel_cases_host.py shows on the CPU that these predicates reject wrong kernels."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp16_kernel_cases as K  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402
from parity_utils import record  # noqa: E402

DEV = "cuda"
_KEEP = []


def D(t):
    """Move to the device and keep the tensor alive until the end of the test (the library gets raw pointers)."""
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


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def st():
    return nat.stream_ptr(torch.device(DEV))


# ------------------------------------------------------------------------------------------------ GEMM
def run_gemm(c, a0=None, a0_f16=None):
    a0 = c.a0 if a0 is None else a0
    a0_f16 = c.a0_f16 if a0_f16 is None else a0_f16
    y = D(c.y_init)
    resid = y if c.resid == "inplace" else D(c.resid_buf)
    nat.check(nat.lib().gfc_linear_f16(
        P(D(a0)), a0_f16, c.lda0, c.K0, P(D(c.a1)), c.a1_f16, c.lda1, c.K1, P(D(c.w)), c.ldw, P(D(c.bias)), c.alpha,
        P(resid), P(D(c.cs)) if c.rot == "packed" else None, P(D(c.cos64)) if c.rot == "tables" else None,
        P(D(c.sin64)) if c.rot == "tables" else None, c.rot_cols, P(y), c.y_f16, c.ldy, c.M, c.N, st()), "gfc_linear_f16")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("form,m", K.GEMM_EXACT)
def test_linear_f16_exact(form, m):
    """Small-integer operands, 0 / +-1 rotary tables: the output equals the integer reference and every canary
    (the row below M, the columns right of N) is still NaN."""
    c = K.gemm_case(form, m, "int")
    y = run_gemm(c)
    ok, _ = c.accept(y)
    assert ok, (c.name, int((y[:m, :c.N] != c.expected[:m, :c.N]).sum()), int(torch.isnan(y[:m, :c.N]).sum()))


@pytest.mark.parametrize("form,m", K.GEMM_RANDOM)
def test_linear_f16_random_vs_float64(form, m):
    """1e-5 * sum|a||w| + 1e-6 |ref| (+ the fp16 output's own rounding) per element, every form."""
    c = K.gemm_case(form, m, "rand")
    ok, ratio = c.accept(run_gemm(c))
    record(f"fp16_linear_{form}", worst_err_over_tol=ratio)
    print(c.name, "worst error / tolerance", ratio)
    assert ok, (c.name, ratio)


@pytest.mark.parametrize("k0", K.STAGING)
def test_linear_f16_staging_rounds_to_nearest_even(k0):
    """fp32 A on every rounding edge of fp16: staged by the kernel == rounded by A.half(), bit for bit."""
    c = K.staging_case(k0)
    y32 = run_gemm(c)
    y16 = run_gemm(c, a0=c.a0.half(), a0_f16=1)
    assert not torch.isnan(y32[:c.M]).any() and torch.isnan(y32[c.M]).all() and torch.isnan(y16[c.M]).all()
    ok, _ = c.accept(y32, y16)
    assert ok, int((y32.view(torch.int32) != y16.view(torch.int32)).sum())


# ------------------------------------------------------------------------------------------------ batched NT
@pytest.mark.parametrize("args", K.NT_CASES, ids=lambda a: "-".join(map(str, a)))
def test_batched_nt_f16(args):
    c = K.nt_case(*args)
    y = D(c.y_init)
    nat.check(nat.lib().gfc_batched_nt_f16(P(D(c.a)), c.K, c.strideA, P(D(c.b)), c.K, c.strideB, P(y), c.N + 1,
                                           (c.M + 1) * (c.N + 1), c.M, c.N, c.K, c.B, st()), "gfc_batched_nt_f16")
    torch.cuda.synchronize()
    ok, ratio = c.accept(y.cpu())
    if not c.exact:
        record(f"fp16_{c.name}", worst_err_over_tol=ratio)
    assert ok, (c.name, ratio)


# ------------------------------------------------------------------------------------------------ attention
ATT_PART, ATT_MAX_SPLIT = 66, 8


def att_scratch_bytes(queries, heads, split):
    """gfc_att_scratch_bytes (csrc/common.h), restated."""
    return queries * heads * split * ATT_PART * 4


def att_split(c, ws_bytes):
    """gfc_att_split (csrc/common.h) as gfc_attention_f16 calls it, restated -- used only to assert that a case
    reaches the split it was chosen for.  If this fails after a policy change, re-pick the shapes."""
    wgs = (c.max_nq + 127) // 128 * K.HEADS * len(c.problems)
    if ws_bytes is None or wgs >= 256:
        return 1
    want = min((511 + wgs) // wgs, ATT_MAX_SPLIT)
    while want > 1 and ws_bytes < att_scratch_bytes(len(c.problems) * c.max_nq, K.HEADS, want):
        want -= 1
    return want


def run_attention(c, ws):
    """ws: "none", "full" (what gfc_attention_workspace_bytes gives) or "three" (scratch for exactly three splits)."""
    x = D(c.x)
    o = D(K.o_blank(c))
    pt = D(torch.tensor(c.problems, dtype=torch.int32))
    n = len(c.problems)
    nbytes = {"none": None, "full": int(nat.lib().gfc_attention_workspace_bytes(n, c.max_nq, K.HEADS)),
              "three": att_scratch_bytes(n * c.max_nq, K.HEADS, 3)}[ws]
    wsb = None if nbytes is None else D(torch.empty(max(nbytes, 256), dtype=torch.uint8))
    q, k, v = x[:, c.qcol:], x[:, c.kcol:], x[:, c.vcol:]
    nat.check(nat.lib().gfc_attention_f16(P(q), c.ld, P(k), c.ld, P(v), c.ld, P(o), c.ldo, P(pt), n, c.max_nq, K.HEADS,
                                          K.SCALE, P(wsb), nbytes or 0, st()), "gfc_attention_f16")
    torch.cuda.synchronize()
    return o.cpu(), att_split(c, nbytes)


# what each named case was chosen for: (case, ws) -> (split, tiles per split of problem 0 or None)
SPLIT_EXPECTED = {
    ("onehot-self-1", "full"): (8, [1, 1, 0, 0, 0, 0, 0, 0]),   # nk = 65: six splits without a tile
    ("onehot-cross-1", "full"): (8, [1, 1, 0, 0, 0, 0, 0, 0]),
    ("onehot-self-2", "full"): (8, [2, 2, 2, 2, 1, 0, 0, 0]),   # nk = 576
    ("onehot-cross-2", "full"): (8, [2, 2, 2, 2, 1, 0, 0, 0]),
    ("onehot-self-2", "three"): (3, [3, 3, 3]),                 # not a power of two
    ("onehot-cross-2", "three"): (3, [3, 3, 3]),
    ("onehot-self-6", "full"): (1, None),                       # the ragged table of all six: 384 workgroups
    ("uniform-self-single65", "full"): (8, [1, 1, 0, 0, 0, 0, 0, 0]),
    ("uniform-cross-single65", "full"): (8, [1, 1, 0, 0, 0, 0, 0, 0]),
    ("many", "full"): (1, None),                                # 64 x 1024 x 1024: no split even with scratch
}
ATT_RUNS = [(n, ws) for n in K.ATT_EXACT + K.ATT_BOUNDED for ws in ("none", "full")] + \
           [("onehot-self-2", "three"), ("onehot-cross-2", "three")]


def _check_split(c, name, ws, split):
    if ws == "none":
        assert split == 1
    if (name, ws) in SPLIT_EXPECTED:
        want, tiles = SPLIT_EXPECTED[(name, ws)]
        assert split == want, (name, ws, split, want)
        if tiles is not None:
            assert K.tiles_per_split(c.problems[0][3], split) == tiles


_REF = {}


def _reference(c, name):
    """Computed once per case and shared by its runs; the 64-problem case on the device, as _ref64 of
    test_gpu_primitives.py does."""
    if name not in _REF:
        with torch.no_grad():
            _REF[name] = K.attention_reference(c, device=DEV if name == "many" else "cpu")
    return _REF[name]


@pytest.mark.parametrize("name,ws", ATT_RUNS)
def test_attention_f16(name, ws):
    """One-hot and uniform cases: O equals the expected tensor exactly.  Random cases: per element within
    2^-11 (sum p|v| + |O|) + 2^-24 sum|v| / l + 1e-5 sum p|v| of float64 on the fp16 operands.  Rows and columns
    outside every problem stay NaN.  With and without the key split."""
    c = K.att_case(name)
    o, split = run_attention(c, ws)
    _check_split(c, name, ws, split)
    if c.exact:
        ok, _ = c.accept(o)
        valid = ~torch.isnan(c.expected)
        assert ok, (name, ws, int((o[valid] != c.expected[valid]).sum()), int((torch.isnan(o) != ~valid).sum()))
    else:
        ok, ratio = K.bounded_accept(c, *_reference(c, name))(o)
        record(f"fp16_attention_{name}_ws_{ws}", worst_err_over_tol=ratio, split=split)
        print(name, ws, "split", split, "worst error / tolerance", ratio)
        assert ok, (name, ws, ratio)
