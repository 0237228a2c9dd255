"""The fp32 LayerNorm and soft-max kernels on the MI355X against the ill-conditioned cases of tests/conditioning_cases.py,
through the C ABI: gfc_layernorm_gelu, gfc_linear_layernorm_gelu, gfc_ffn_fused, gfc_attention (both query-tile
configurations, with and without the key split) and gfc_sp_detector_head.

Every comparison is against float64 on exactly representable pre-activations / logits, under the per-element bounds
the cases carry; tests/test_conditioning_cases_host.py shows on the CPU that these bounds reject the one-pass variance,
a missing or misplaced eps, a missing running maximum, a missing rescale and the wrong merges by a factor of 100 or
more.  Each test records its worst error / bound ratio (parity_utils.record, keys conditioning_*)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import conditioning_cases as C  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402
from parity_utils import record  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
CFG = os.environ.get("GFC_ATTN_CFG", "")  # the child process of test_attention_two_query_tiles_per_wave sets it
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


# ------------------------------------------------------------------------------------------------ LayerNorm
def _cases_of(launch):
    return [case for case, (ln, _) in C.LN_CASES.items() if ln == launch]


@pytest.mark.parametrize("launch", ["offset", "tiny"])
def test_layernorm_gelu_conditioning(launch):
    """gfc_layernorm_gelu, gfc_linear_layernorm_gelu and gfc_ffn_fused on one launch of 133 rows: the row statistics at
    mean 4096 / sigma 8, at zero variance, under one element 20 sigma out, and at a variance of the order of eps."""
    lib = nat.lib()
    c = C.ln_launch(launch)
    m = c.M
    a0, a1 = D(c.a[:, :256]), D(c.a[:, 256:])
    w0, b0, ga, be, w3, b3 = (D(t) for t in (c.w0, c.b0, c.gamma, c.beta, c.w3, c.b3))
    # the stand-alone kernel on the exact pre-activation, in place
    x = D(c.pre.clone())
    nat.check(lib.gfc_layernorm_gelu(P(x), 512, m, 512, P(ga), P(be), st()), "gfc_layernorm_gelu")
    # the GEMM with the LayerNorm + GELU epilogue
    h = torch.full((m + 1, 512), C.NAN, device=DEV)
    nat.check(lib.gfc_linear_layernorm_gelu(P(a0), 256, 256, P(a1), 256, 256, P(w0), 512, P(b0), P(ga), P(be), P(h), 512, m,
                                            512, st()), "gfc_linear_layernorm_gelu")
    # the whole FFN in one kernel, and the two-kernel path
    y = torch.full((m + 1, 256), C.NAN, device=DEV)
    nat.check(lib.gfc_ffn_fused(P(a0), 256, 256, P(a1), 256, 256, P(w0), 512, P(b0), P(ga), P(be), P(w3), 512, P(b3), P(a0),
                                P(y), 256, m, st()), "gfc_ffn_fused")
    y2 = torch.empty((m, 256), device=DEV)
    nat.check(lib.gfc_linear(P(h), 512, 512, None, 0, 0, P(w3), 512, P(b3), None, None, 1.0, P(a0), None, None, 0, P(y2),
                             256, m, 256, st()), "gfc_linear")
    torch.cuda.synchronize()
    assert torch.isnan(h[m]).all() and torch.isnan(y[m]).all()  # the row below the launch
    assert torch.equal(y[:m], y2)  # bit for bit: the fused kernel's statistics are those of the two-kernel path
    xc, hc, yc = x.cpu(), h[:m].cpu(), y[:m].cpu()
    for case in _cases_of(launch):
        for name, out, which in (("layernorm_gelu", xc, "h"), ("linear_layernorm_gelu", hc, "h"), ("ffn_fused", yc, "y")):
            ratio = C.ln_ratio(case, out, which)
            record(f"conditioning_{name}_{case}", worst_err_over_tol=ratio)
            print(name, case, "worst error / bound", ratio)
            assert ratio <= 1.0, (name, case, ratio)
    assert torch.isfinite(xc).all() and torch.isfinite(hc).all() and torch.isfinite(yc).all()
    if launch == "offset":  # zero variance: gelu(beta), the same in every such row
        rows = C.ln_rows("const")
        for out in (xc, hc):
            assert all(torch.equal(out[r], out[rows[0]]) for r in rows)


# ------------------------------------------------------------------------------------------------ attention
ATT_PART, ATT_MAX_SPLIT = 66, 8


def att_scratch_bytes(queries, split):
    """gfc_att_scratch_bytes (csrc/common.h), restated."""
    return queries * C.HEADS * split * ATT_PART * 4


def att_split(c, ws_bytes):
    """gfc_att_split (csrc/common.h) as gfc_attention calls it, restated -- used only to assert that a launch reaches
    the split it was built for.  If this fails after a policy change, re-pick the shapes."""
    wgs = (c.max_nq + 127) // 128 * C.HEADS * len(c.problems)
    if not ws_bytes or wgs >= 256 or CFG == "1":
        return 1
    want = min((511 + wgs) // wgs, ATT_MAX_SPLIT)
    while want > 1 and ws_bytes < att_scratch_bytes(len(c.problems) * c.max_nq, want):
        want -= 1
    return want


def run_attention(c):
    """The scratch offers of test_attention_scratch_smaller_than_the_full_split: the full size (split 8), exactly the
    partials of a 3-way split, 4 bytes short of a 2-way split (no split); none for the launches without a split."""
    lib = nat.lib()
    n = len(c.problems)
    queries = n * c.max_nq
    full = int(lib.gfc_attention_workspace_bytes(n, c.max_nq, C.HEADS))
    offer = {"single": 0, "pair": 0, "split8": full, "split3": att_scratch_bytes(queries, 3),
             "nosplit": att_scratch_bytes(queries, 2) - 4}[c.run]
    ws = D(torch.empty(max(full, 256), dtype=torch.uint8)) if offer else None
    o = torch.full((c.rows, 256), C.NAN, device=DEV)
    nat.check(lib.gfc_attention(P(D(c.q)), 256, P(D(c.k)), 256, P(D(c.v)), 256, P(o), 256,
                                P(D(torch.tensor(c.problems, dtype=torch.int32))), n, c.max_nq, C.HEADS, C.SCALE, P(ws), offer,
                                st()), "gfc_attention")
    torch.cuda.synchronize()
    return o.cpu(), att_split(c, offer)


ATT_LAUNCHES = [(case, run) for case in C.ATT_CASES for run in C.ATT_RUNS]


@pytest.mark.parametrize("case,run", ATT_LAUNCHES, ids=[f"{a}-{b}" for a, b in ATT_LAUNCHES])
def test_attention_conditioning(case, run):
    """gfc_attention on logits of +-145, on a maximum that rises in every half tile, never, or for a few lanes of a wave
    only, on rows of -190 and of +190 and on identical keys: per problem and head within the case's bound of float64,
    every output finite, rows beyond nq untouched.  As one problem, as two with a masked key tail, and through the key
    split by 8 (merge weights that underflow to 0), by 3 (an empty share) and with scratch too small for any split."""
    c = C.att_case(case, run)
    o, split = run_attention(c)
    if CFG != "1":
        assert split == c.split, (split, c.split)
    ratio, untouched = C.att_ratio(c, o)
    record(f"conditioning_attention{'_cfg' + CFG if CFG else ''}_{case}_{run}", worst_err_over_tol=ratio, split=split)
    print(case, run, "split", split, "worst error / bound", ratio)
    assert untouched, "rows outside every problem's queries were written"
    valid = ~torch.isnan(c.ref)
    assert torch.isfinite(o[valid]).all()
    assert ratio <= 1.0, (case, run, ratio)


def test_attention_two_query_tiles_per_wave():
    """attention_kernel<2> (GFC_ATTN_CFG=1: two 32-query tiles per wave, what a 32-pair batch dispatches to) on the
    launches without a key split; the knob is read once per process, so they run in one child pytest process."""
    env = dict(os.environ, GFC_ATTN_CFG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-k", "test_attention_conditioning and (single or pair)", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-400:])
    assert f"{2 * len(C.ATT_CASES)} passed" in r.stdout, r.stdout[-400:]


# ------------------------------------------------------------------------------------------------ detector head
@pytest.mark.parametrize("mode", C.DH_MODES)
@pytest.mark.parametrize("shape", C.DH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_detector_head_conditioning(shape, mode):
    """gfc_sp_detector_head on integer logits spanning more than +-100 (the affine of the open variant) and without the
    affine: the dustbin far above and far below the heat-map channels, 96 above them (heat values in the subnormal
    range), two channels tied for the maximum, all 65 logits equal."""
    c = C.dh_case(shape, mode)
    b, h8, w8 = shape
    heat = torch.full((b, h8 * 8, w8 * 8), C.NAN, device=DEV)
    nat.check(nat.lib().gfc_sp_detector_head(P(D(c.hidden)), 512, P(D(c.w)), P(D(c.bias)), P(D(c.scale)), P(D(c.shift)), b, h8,
                                             w8, P(heat), st()), "gfc_sp_detector_head")
    torch.cuda.synchronize()
    out = C.dh_from_heat(c, heat.cpu())
    assert torch.isfinite(out).all()
    ratio = C.dh_ratio(c, out)
    record(f"conditioning_detector_head_{c.name}", worst_err_over_tol=ratio)
    print(c.name, "worst error / bound", ratio)
    assert ratio <= 1.0, (c.name, ratio)
    # the winner of every cell whose two largest heat-map logits differ (and whose winner is a normal fp32 number: below
    # 2^-126 the outputs of different logits may round to the same subnormal); exact ties give equal values
    top = c.logits[:, :64].topk(2, 1)
    decided = (top.values[:, 0] > top.values[:, 1]) & (c.ref.max(1).values >= 2.0 ** -126)
    assert c.cells < 16 or int(decided.sum()) > 100
    assert torch.equal(out.argmax(1)[decided], top.indices[decided, 0])
    lg = c.logits[:, :64]
    order = lg.argsort(1)
    same = lg.gather(1, order)[:, 1:] == lg.gather(1, order)[:, :-1]
    vals = out.gather(1, order)
    assert torch.equal(vals[:, 1:][same], vals[:, :-1][same])
    for cell in c.kind["tie"]:
        assert out[cell, C.DH_TIE[0]] == out[cell, C.DH_TIE[1]] == out[cell].max()
