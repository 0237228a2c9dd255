"""gfc_attention_self_backward, gfc_lg_self_attn_backward and gfc_lg_layer_pairs_keep_self alone on the GPU, against the
float64 closed form of tests/self_block_grad_reference.py evaluated on the SAME bits: every output element within 2^-23
times its error sum (derived there from the shape alone; the closed form runs in float64 torch on the device, so that the
largest shape stays a matter of seconds).

Shapes (B, M, N) at the edges of the kernel's plan -- a wave owns 32 rows, a workgroup 128, the side is streamed in tiles
of 32 rows, once as keys and once as queries: single rows; 4 / 5 rows (the second lane half of the log-sum-exp sees no key
of a side of fewer than five); 31..33 and 63..65 (a wave, a tile, two of them); 127..130 (a workgroup); 257, 300 (several
workgroups, a ragged last tile); 1024 (many pairs' worth of workgroups) and 2048 with one pair (few workgroups, long
streams).
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import self_block_grad_reference as sbr  # noqa: E402
import test_gpu_output_stage as tos  # noqa: E402  (model, layer_call: one layer's call as forward_layers builds it)

from glue_factory_colon_amd import _native as nat  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
D = sbr.D
Q = 3 * D
SHAPES = ((1, 1, 1), (1, 1, 65), (2, 3, 2), (1, 5, 4), (1, 31, 33), (1, 32, 32), (2, 63, 64), (1, 64, 65), (1, 127, 129),
          (1, 128, 128), (3, 130, 65), (2, 129, 257), (1, 300, 257), (2, 1024, 1024), (1, 2048, 2048))
WORST = {}


def strided(t, ld):
    """A view with leading dimension ld of a NaN-filled buffer, holding t."""
    buf = torch.full((t.shape[0], max(ld, t.shape[1])), NAN, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf


def run_core(qkv, ctx, dctx, cos, sin, shape, lds=(Q, D, D, Q), heads=4, scale=sbr.SCALE, ws_bytes=None, ws_offset=0,
             out=None):
    """One call on device tensors; every operand is placed in a buffer of its leading dimension; the workspace and the
    output are filled with NaNs on entry.  -> dqkv as a [R,768] view."""
    b, m, n = shape
    rows = qkv.shape[0]
    ins = [strided(t, ld) for t, ld in zip((qkv, ctx, dctx), lds)]
    out = torch.full((rows, max(lds[3], Q)), NAN, device=DEV) if out is None else out
    need = nat.call("gfc_attention_self_backward_workspace_bytes", max(b, 1), max(m, 1), max(n, 1), 4)
    ws = torch.full(((need if ws_bytes is None else ws_bytes) + ws_offset,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[ws_offset:]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    try:
        status = nat.lib().gfc_attention_self_backward(
            ins[0].data_ptr(), lds[0], ins[1].data_ptr(), lds[1], ins[2].data_ptr(), lds[2], ptr(cos), ptr(sin), b, m, n,
            heads, scale, out.data_ptr(), lds[3], ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    nat.check(status, "gfc_attention_self_backward")
    assert lds[3] == Q or bool(torch.isnan(out[:, Q:]).all())  # nothing is written outside the 768 columns
    return out[:, :Q]


def check_core(tag, qkv, ctx, dctx, cos, sin, shape, lds=(Q, D, D, Q)):
    """Float32 host tensors (cos, sin may be None).  Two calls agree bit for bit; every element inside its bound."""
    dev = [None if t is None else t.to(DEV).contiguous() for t in (qkv, ctx, dctx, cos, sin)]
    got, again = run_core(*dev, shape, lds), run_core(*dev, shape, lds)
    assert torch.equal(got, again), f"{tag}: two calls differ"
    want, errs = sbr.attention_backward(*(None if t is None else t.double() for t in dev), *shape)
    tol = sbr.U * errs
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    report = {}
    for k, c0 in (("dq", 0), ("dk", D), ("dv", 2 * D)):
        report[k] = sbr.worst_ratio(got[:, c0:c0 + D], want[:, c0:c0 + D], tol[:, c0:c0 + D])
        WORST[k] = max(WORST.get(k, 0.0), report[k])
    print(f"{tag}: fraction of the bound used: " + ", ".join(f"{k} {r:.3f}" for k, r in report.items()))
    assert max(report.values()) <= 1.0, (tag, report)
    return got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_core_matches_closed_form(shape):
    check_core(f"core {shape}", *sbr.random_core(*shape, seed=sum(shape)), shape)


def test_core_general_tables():
    """Tables with unequal entries within a pair pin the general transpose."""
    shape = (2, 70, 45)
    check_core("general tables", *sbr.random_core(*shape, seed=21, equal_pairs=False), shape)


def test_core_null_tables_signed_permutation():
    """cos / sin NULL equals cos = 1, sin = 0 bit for bit; cos = 0, sin = 1 is a signed permutation of the columns of dq
    and dk: dt[2i] = do[2i+1], dt[2i+1] = -do[2i], the same bits permuted.  The core reads q' and k' ALREADY rotated, so its
    tables act in the epilogue only: "the run on pre-permuted inputs with cos = 1, sin = 0, permuted back" is, for the
    core, the plain run's output permuted, which is what is compared here.  The form with pre-permuted inputs proper is
    test_block_signed_permutation, where the forward's rotation is part of the call."""
    shape = (2, 70, 45)
    qkv, ctx, dctx, cos, _ = sbr.random_core(*shape, seed=22)
    dev = [t.to(DEV) for t in (qkv, ctx, dctx)]
    one, zero = torch.ones_like(cos, device=DEV), torch.zeros_like(cos, device=DEV)
    plain = run_core(*dev, None, None, shape)
    assert torch.equal(run_core(*dev, one, zero, shape), plain)
    perm = run_core(*dev, zero, one, shape)
    want = torch.cat([-sbr._sign(plain[:, :2 * D]) * sbr._swap(plain[:, :2 * D]), plain[:, 2 * D:]], 1)
    assert torch.equal(perm, want)
    check_core("no tables", qkv, ctx, dctx, None, None, shape)


def test_core_negative_and_zero_dctx():
    shape = (2, 70, 45)
    qkv, ctx, dctx, cos, sin = sbr.random_core(*shape, seed=5, dctx_sign=-1.0)
    check_core("negative dctx", qkv, ctx, dctx, cos, sin, shape)
    got = run_core(qkv.to(DEV), ctx.to(DEV), torch.zeros_like(dctx, device=DEV), cos.to(DEV), sin.to(DEV), shape)
    assert bool((got == 0).all())


def test_core_dctx_zero_on_one_side():
    """dctx = 0 on side 0: a side's outputs depend on that side alone, so side 0's are exact zeros."""
    b, m, n = shape = (2, 50, 77)
    qkv, ctx, dctx, cos, sin = sbr.random_core(*shape, seed=9)
    dctx[:b * m] = 0
    got, _ = check_core("dctx zero on side 0", qkv, ctx, dctx, cos, sin, shape)
    assert bool((got[:b * m] == 0).all()) and bool((got[b * m:] != 0).any())


def test_core_identical_keys():
    qkv, ctx, dctx, shape = sbr.identical_keys_case()
    got, _ = check_core("64 identical keys", qkv, ctx, dctx, None, None, shape)
    m = shape[1]
    # side 1's rows are indistinguishable: the same S, the same lse, the same sums
    assert torch.equal(got[m:], got[m:m + 1].expand(64, Q))


def test_core_dominant_key():
    qkv, ctx, dctx, shape, key = sbr.dominant_key_case()
    got, _ = check_core("dominant key", qkv, ctx, dctx, None, None, shape)
    m = shape[1]
    want = torch.zeros_like(got)
    want[key, 2 * D:] = dctx[:m].to(DEV).sum(0)      # exact: integers over 1024
    want[m + key, 2 * D:] = dctx[m:].to(DEV).sum(0)
    assert torch.equal(got, want)


def test_core_leading_dimensions():
    shape = (2, 40, 67)
    t = sbr.random_core(*shape, seed=12)
    plain, _ = check_core("contiguous", *t, shape)
    wide, _ = check_core("leading dimensions", *t, shape, lds=(772, 264, 300, 1024))
    assert torch.equal(plain, wide)


def test_core_refusals_leave_outputs_untouched():
    shape = (1, 40, 33)
    dev = [t.to(DEV) for t in sbr.random_core(*shape, seed=2)]
    wsb = lambda *a: nat.call("gfc_attention_self_backward_workspace_bytes", *a)  # noqa: E731
    need = wsb(*shape, 4)
    assert need == 2 * 1280  # lse 73 * 4 floats | D 73 * 4 floats, each slot rounded up to 256 bytes
    assert wsb(0, 40, 33, 4) == 0 and wsb(1, 0, 33, 4) == 0 and wsb(1, 40, 0, 4) == 0 and wsb(1, 40, 33, 8) == 0
    assert wsb(1, 2796201, 1, 4) > 0 and wsb(1, 2796202, 1, 4) == 0
    cases = (({"ws_bytes": need - 1}, "GFC_ERR_WORKSPACE"), ({"ws_offset": 4}, "GFC_ERR_WORKSPACE"),
             ({"heads": 8}, "GFC_ERR_INVALID"), ({"lds": (Q, D, D, 764)}, "GFC_ERR_INVALID"),
             ({"lds": (770, D, D, Q)}, "GFC_ERR_INVALID"), ({"lds": (Q, 252, D, Q)}, "GFC_ERR_INVALID"),
             ({"sin": None}, "GFC_ERR_INVALID"), ({"cos": None}, "GFC_ERR_INVALID"))
    for kwargs, status in cases:
        kwargs = dict(kwargs)
        args = list(dev)
        for i, k in ((3, "cos"), (4, "sin")):
            if k in kwargs:
                args[i] = kwargs.pop(k)
        out = torch.full((73, 1024), NAN, device=DEV)
        with pytest.raises(nat.NativeError, match=status):
            run_core(*args, shape, out=out, **kwargs)
        assert bool(torch.isnan(out).all()), (kwargs, status)
    for bad in ((0, 40, 33), (1, 0, 33), (1, 40, 0)):
        out = torch.full((73, Q), NAN, device=DEV)
        with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
            run_core(*dev, bad, out=out)
        assert bool(torch.isnan(out).all())


# ---- the block entry --------------------------------------------------------------------------------------------------
def fresh(rows, want_dx=True):
    return {"dWqkv": torch.full((Q, D), NAN, device=DEV), "dbqkv": torch.full((Q,), NAN, device=DEV),
            "dx": torch.full((rows, D), NAN, device=DEV) if want_dx else None}


def run_block(x, cos, sin, ctx, dctx, dx_in, w, bias, shape, want_dx=True, ws_bytes=None, ws_offset=0, out=None):
    out = fresh(x.shape[0], want_dx) if out is None else out
    need = nat.call("gfc_lg_self_attn_backward_workspace_bytes", *(max(s, 1) for s in shape))
    ws = torch.full(((need if ws_bytes is None else ws_bytes) + ws_offset,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[ws_offset:]
    try:
        nat.call("gfc_lg_self_attn_backward", x, cos, sin, ctx, dctx, dx_in, w, bias, *shape, out["dWqkv"], out["dbqkv"],
                 out["dx"], ws, ws.numel())
    finally:
        torch.cuda.synchronize()
    return out


def autograd64(x, cos, sin, dctx, w_sd, b_sd, shape):
    """torch float64 autograd of Wqkv (state-dict order) + rotary + attention on the device: dWqkv, dbqkv, dx_att."""
    b, m, n = shape
    leaf = lambda t: t.detach().double().requires_grad_()  # noqa: E731
    w, bias, xl = leaf(w_sd), leaf(b_sd), leaf(x)
    loss = 0.0
    for rows, cnt in ((slice(0, b * m), m), (slice(b * m, None), n)):
        c, s = (t[rows].double().reshape(b, 1, cnt, 64) for t in (cos, sin))
        qkv = (xl[rows].reshape(b, cnt, D) @ w.t() + bias).unflatten(-1, (4, -1, 3)).transpose(1, 2)
        q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
        half = lambda t: torch.stack((-t[..., 1::2], t[..., 0::2]), -1).flatten(-2)  # noqa: E731  rotate_half
        q, k = q * c + half(q) * s, k * c + half(k) * s
        ctx = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v
        loss = loss + (ctx.transpose(1, 2).reshape(b * cnt, D) * dctx[rows].double()).sum()
    loss.backward()
    return {"dWqkv": w.grad, "dbqkv": bias.grad, "dx_att": xl.grad}


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 700, 1400)),
                         ids=lambda s: "x".join(map(str, s)))
def test_block_matches_closed_form(shape):
    host = sbr.random_block(*shape, seed=40 + sum(shape))
    x, cos, sin, ctx, dctx, dx_in, w, bias = (t.to(DEV) for t in host)
    args = (x, cos, sin, ctx, dctx)
    full, again = run_block(*args, dx_in, w, bias, shape), run_block(*args, dx_in, w, bias, shape)
    att, bare = run_block(*args, None, w, bias, shape), run_block(*args, None, w, bias, shape, want_dx=False)
    for k in ("dWqkv", "dbqkv", "dx"):
        assert torch.equal(full[k], again[k]), k
    for k in ("dWqkv", "dbqkv"):  # the parameter gradients do not depend on the row outputs asked for
        assert torch.equal(full[k], att[k]) and torch.equal(full[k], bare[k]), k
    d = lambda t: t.double()  # noqa: E731
    want, errs = sbr.backward(d(x), d(cos), d(sin), d(ctx), d(dctx), d(dx_in), d(w), d(bias), *shape)
    tol = sbr.bounds(errs)
    got = dict(full, dx_att=att["dx"])
    report = {k: sbr.worst_ratio(got[k], want[k], tol[k]) for k in sbr.OUTPUTS}
    for k, r in report.items():
        WORST[k] = max(WORST.get(k, 0.0), r)
    print(f"block {shape}: fraction of the bound used: " + ", ".join(f"{k} {r:.3f}" for k, r in report.items()))
    assert max(report.values()) <= 1.0, report
    # the attention's share is tested on its own: the summed dx is 200 times larger and blind to it
    assert float(want["dx_att"].abs().max()) < 0.05 * float(want["dx"].abs().max())
    # mapped to state-dict order, against torch's float64 autograd of the block as the reference writes it
    ref = autograd64(x, cos, sin, dctx, sbr.to_state_dict(w), sbr.to_state_dict(bias), shape)
    for k, mine, bound in (("dWqkv", sbr.to_state_dict(full["dWqkv"]), sbr.to_state_dict(tol["dWqkv"])),
                           ("dbqkv", sbr.to_state_dict(full["dbqkv"]), sbr.to_state_dict(tol["dbqkv"])),
                           ("dx_att", att["dx"], tol["dx_att"])):
        # ctx is the float32 rounding of the forward: the closed form reads it in D, autograd its own float64 one
        assert sbr.worst_ratio(mine, ref[k], bound) <= 1.0, k


def test_block_signed_permutation():
    """cos = 0, sin = 1 makes q' and k' signed permutations of the GEMM's columns.  The same call on PRE-PERMUTED Wqkv /
    bqkv rows with cos = 1, sin = 0 forms the same q', k' bits, so its dWqkv / dbqkv, permuted back, are the same bits."""
    shape = (2, 63, 64)
    x, cos, sin, ctx, dctx, dx_in, w, bias = (t.to(DEV) for t in sbr.random_block(*shape, seed=7))
    one, zero = torch.ones_like(cos), torch.zeros_like(cos)
    # q'[2i] = -t[2i+1], q'[2i+1] = t[2i]: rows of the q and k thirds swapped within pairs, the first negated
    fwd = lambda t: torch.cat([sbr._sign(t[:2 * D].t()).t() * sbr._swap(t[:2 * D].t()).t(), t[2 * D:]], 0)  # noqa: E731
    back = lambda t: torch.cat([-sbr._sign(t[:2 * D].t()).t() * sbr._swap(t[:2 * D].t()).t(), t[2 * D:]], 0)  # noqa: E731
    assert torch.equal(back(fwd(w)), w)
    got = run_block(x, zero, one, ctx, dctx, dx_in, w, bias, shape)
    pre = run_block(x, one, zero, ctx, dctx, dx_in, fwd(w), fwd(bias[:, None])[:, 0].contiguous(), shape)
    assert torch.equal(got["dWqkv"], back(pre["dWqkv"]))
    assert torch.equal(got["dbqkv"], back(pre["dbqkv"][:, None])[:, 0])
    assert bool(torch.isfinite(got["dx"]).all())


def test_block_refusals_leave_outputs_untouched():
    shape = (1, 40, 33)
    x, cos, sin, ctx, dctx, dx_in, w, bias = (t.to(DEV) for t in sbr.random_block(*shape, seed=3))
    args = (x, cos, sin, ctx, dctx, dx_in, w, bias)
    need = nat.call("gfc_lg_self_attn_backward_workspace_bytes", *shape)
    assert need > 0 and nat.call("gfc_lg_self_attn_backward_workspace_bytes", 0, 40, 33) == 0
    untouched = lambda out: all(bool(torch.isnan(t).all()) for t in out.values() if t is not None)  # noqa: E731
    for kwargs, status in (({"ws_bytes": need - 1}, "GFC_ERR_WORKSPACE"), ({"ws_offset": 4}, "GFC_ERR_WORKSPACE")):
        out = fresh(73)
        with pytest.raises(nat.NativeError, match=status):
            run_block(*args, shape, out=out, **kwargs)
        assert untouched(out), kwargs
    for bad in ((0, 40, 33), (1, 40, 0)):
        out = fresh(73)
        with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
            run_block(*args, bad, out=out)
        assert untouched(out), bad
    out = fresh(73)  # dx_in without dx, dx_in as dx, no tables
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        run_block(*args, shape, out=dict(out, dx=None))
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        run_block(x, cos, sin, ctx, dctx, out["dx"], w, bias, shape, out=out)
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        run_block(x, None, None, ctx, dctx, dx_in, w, bias, shape, out=out)
    assert untouched(out)


# ---- the layer entry that keeps the self attention's context ------------------------------------------------------------
@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("shape", [(2, 130, 65), (8, 1024, 1024)], ids=["2x130x65", "8x1024x1024_fused_ffn"])
def test_keep_self_is_the_keep_entry_and_completes_the_self_block(shape, fold):
    """x, x_mid and the cross context are gfc_lg_layer_pairs_keep's bit for bit; the kept self context completes the self
    block to x_mid bit for bit with the entry points the layer took at that size."""
    b, m, n = shape
    lg = tos.model(fold_out_proj=fold)  # (kept alive: `params` holds raw pointers into its packed weights)
    p, x, cos, sin, self_p, cross_p, ws = tos.layer_call(lg, b, m, n, 5)
    rows, l = b * (m + n), tos.L - 1
    nan = lambda: torch.full_like(x, NAN)  # noqa: E731
    kept, both, mid, ctx, mid2, ctx2, ctx_self = x.clone(), x.clone(), nan(), nan(), nan(), nan(), nan()
    nat.call("gfc_lg_layer_pairs_keep", ctypes.byref(p), l, kept, cos, sin, b, m, n, self_p, cross_p, mid, ctx, ws, ws.numel())
    nat.call("gfc_lg_layer_pairs_keep_self", ctypes.byref(p), l, both, cos, sin, b, m, n, self_p, cross_p, mid2, ctx2,
             ctx_self, ws, ws.numel())
    torch.cuda.synchronize()
    assert torch.equal(kept, both) and torch.equal(mid, mid2) and torch.equal(ctx, ctx2)
    assert bool(torch.isfinite(ctx_self).all()) and not torch.equal(ctx_self, ctx)
    msg = ctx_self
    if not fold:
        msg = torch.empty((rows, D), device=DEV)
        nat.call("gfc_linear", ctx_self, D, D, None, 0, 0, p.s_out_w[l], D, p.s_out_b[l], None, None, 1.0, None, None, None,
                 0, msg, D, rows, D)
    h = torch.empty((rows, 512), device=DEV)
    if rows >= 128 * 128:  # gfc_ffn_fused, whose bits are those of gfc_linear_layernorm_gelu + gfc_linear
        nat.call("gfc_linear_layernorm_gelu", x, D, D, msg, D, D, p.s_ffn0_w[l], 512, p.s_ffn0_b[l], p.s_ln_g[l],
                 p.s_ln_b[l], h, 512, rows, 512)
    else:
        nat.call("gfc_linear", x, D, D, msg, D, D, p.s_ffn0_w[l], 512, p.s_ffn0_b[l], None, None, 1.0, None, None, None, 0,
                 h, 512, rows, 512)
        nat.call("gfc_layernorm_gelu", h, 512, rows, 512, p.s_ln_g[l], p.s_ln_b[l])
    y = torch.empty((rows, D), device=DEV)
    nat.call("gfc_linear", h, 512, 512, None, 0, 0, p.s_ffn3_w[l], 512, p.s_ffn3_b[l], None, None, 1.0, x, None, None, 0, y,
             D, rows, D)
    torch.cuda.synchronize()
    assert torch.equal(y, mid)


def test_keep_self_refuses_null_and_fp16():
    b, m, n = 1, 16, 16
    for net, what in ((tos.model(), "null"), (tos.model(matmul_precision="fp16"), "fp16")):
        p, x, cos, sin, self_p, cross_p, ws = tos.layer_call(net, b, m, n, 2)
        before = x.clone()
        outs = [torch.full_like(x, NAN) for _ in range(3)]
        for gone in ((0, 1, 2) if what == "null" else (None,)):
            args = [None if i == gone else t for i, t in enumerate(outs)]
            with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
                nat.call("gfc_lg_layer_pairs_keep_self", ctypes.byref(p), 0, x, cos, sin, b, m, n, self_p, cross_p, *args,
                         ws, ws.numel())
        torch.cuda.synchronize()
        assert torch.equal(x, before) and all(bool(torch.isnan(t).all()) for t in outs)  # before any launch


def test_zz_report_worst_fractions():
    print("self-attention backward: largest fraction of a bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    assert WORST and max(WORST.values()) <= 1.0
