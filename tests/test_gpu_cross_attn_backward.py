"""gfc_attention_cross_backward and gfc_lg_cross_attn_backward alone on the GPU, against the float64 closed form of
tests/cross_attn_grad_reference.py evaluated on the SAME bits: every output element within 2^-23 times its error sum
(derived there from the shape alone; the closed form runs in float64 torch on the device, so that the largest shape stays
a matter of seconds).

Shapes (B, M, N) at the edges of the kernel's plan -- a wave owns 32 rows, a workgroup 128, the keys come in tiles of 32,
and each side is both the owner and the keys: single rows and keys; 4 / 5 keys (the second lane half of the log-sum-exp
sees no key of a side of fewer than five); 31..33 and 63..65 (a wave, a key tile, two of them); 127..130 (a workgroup);
257, 300 (several workgroups, a ragged last tile); 1024 (many pairs' worth of workgroups) and 2048 with one pair (few
workgroups, long key streams).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_attn_grad_reference as car  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
D = car.D
SHAPES = ((1, 1, 1), (1, 1, 65), (1, 65, 1), (2, 63, 64), (1, 64, 65), (3, 130, 65), (2, 129, 257), (1, 300, 257),
          (2, 3, 2), (1, 5, 4), (1, 31, 33), (1, 32, 32), (1, 33, 31), (1, 127, 129), (1, 128, 128),
          (2, 1024, 1024), (1, 2048, 2048))
WORST = {}


def strided(t, ld):
    """A [R,256] view with leading dimension ld of a NaN-filled buffer, holding t."""
    buf = torch.full((t.shape[0], max(ld, D)), NAN, device=DEV)
    buf[:, :D] = t
    return buf


def run_core(qk, v, ctx, dctx, shape, lds=(D,) * 6, heads=4, scale=car.SCALE, ws_bytes=None, ws_offset=0, out=None):
    """One call on device tensors [R,256]; every operand is placed in a buffer of its leading dimension; the workspace
    and the outputs are filled with NaNs on entry.  -> (dqk, dv) as [R,256] views."""
    b, m, n = shape
    rows = qk.shape[0]
    ins = [strided(t, ld) for t, ld in zip((qk, v, ctx, dctx), lds)]
    outs = out or [torch.full((rows, ld), NAN, device=DEV) for ld in lds[4:]]
    need = nat.call("gfc_attention_cross_backward_workspace_bytes", max(b, 1), max(m, 1), max(n, 1), 4)
    ws = torch.full(((need if ws_bytes is None else ws_bytes) + ws_offset,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[ws_offset:]
    try:
        lib = nat.lib()
        status = lib.gfc_attention_cross_backward(
            ins[0].data_ptr(), lds[0], ins[1].data_ptr(), lds[1], ins[2].data_ptr(), lds[2], ins[3].data_ptr(), lds[3],
            b, m, n, heads, scale, outs[0].data_ptr(), lds[4], outs[1].data_ptr(), lds[5], ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    nat.check(status, "gfc_attention_cross_backward")
    for o, ld in zip(outs, lds[4:]):  # nothing is written outside the 256 columns
        assert ld == D or bool(torch.isnan(o[:, D:]).all())
    return outs[0][:, :D], outs[1][:, :D]


def check_core(tag, qk, v, ctx, dctx, shape, lds=(D,) * 6):
    """Float32 host tensors.  Two calls agree bit for bit; every element inside its bound."""
    dev = [t.to(DEV) for t in (qk, v, ctx, dctx)]
    got, again = run_core(*dev, shape, lds), run_core(*dev, shape, lds)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_), f"{tag}: two calls differ"
    want, errs = car.attention_backward(*(t.double() for t in dev), *shape)
    tol = car.bounds(errs)
    report = {}
    for k, g in zip(("dqk", "dv"), got):
        assert bool(torch.isfinite(g).all()), f"{tag}: {k} is not finite"
        report[k] = car.worst_ratio(g, want[k], tol[k])
        WORST[k] = max(WORST.get(k, 0.0), report[k])
    print(f"{tag}: fraction of the bound used: " + ", ".join(f"{k} {r:.3f}" for k, r in report.items()))
    assert max(report.values()) <= 1.0, (tag, report)
    return dict(zip(("dqk", "dv"), got)), want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_core_matches_closed_form(shape):
    check_core(f"core {shape}", *car.random_core(*shape, seed=sum(shape)), shape)


def test_core_negative_and_zero_dctx():
    shape = (2, 70, 45)
    qk, v, ctx, dctx = car.random_core(*shape, seed=5, dctx_sign=-1.0)
    check_core("negative dctx", qk, v, ctx, dctx, shape)
    dq, dv = run_core(qk.to(DEV), v.to(DEV), ctx.to(DEV), torch.zeros_like(dctx, device=DEV), shape)
    assert bool((dq == 0).all()) and bool((dv == 0).all())


def test_core_dctx_zero_on_one_side():
    """dctx0 = 0: D0 and dctx0 . v1 are exact zeros, so dv1 = P01^T dctx0 is exactly 0; the rest within its bounds."""
    b, m, n = shape = (2, 50, 77)
    qk, v, ctx, dctx = car.random_core(*shape, seed=9)
    dctx[:b * m] = 0
    got, _ = check_core("dctx zero on side 0", qk, v, ctx, dctx, shape)
    assert bool((got["dv"][b * m:] == 0).all()) and bool((got["dv"][:b * m] != 0).any())


def test_core_identical_keys():
    qk, v, ctx, dctx, shape = car.identical_keys_case()
    got, _ = check_core("64 identical keys", qk, v, ctx, dctx, shape)
    m = shape[1]
    # side 1's rows are indistinguishable as owners: the same S, the same lse, the same sums
    assert torch.equal(got["dv"][m:], got["dv"][m:m + 1].expand(64, D))


def test_core_dominant_key():
    qk, v, ctx, dctx, shape, key = car.dominant_key_case()
    got, _ = check_core("dominant key", qk, v, ctx, dctx, shape)
    m = shape[1]
    assert bool((got["dqk"] == 0).all()) and bool((got["dv"][:m] == 0).all())
    rest = [j for j in range(shape[2]) if j != key]
    assert bool((got["dv"][m:][rest] == 0).all())
    assert torch.equal(got["dv"][m + key], dctx[:m].to(DEV).sum(0))  # exact: integers over 1024


def test_core_leading_dimensions():
    shape = (2, 40, 67)
    t = car.random_core(*shape, seed=12)
    plain, _ = check_core("contiguous", *t, shape)
    wide, _ = check_core("leading dimensions", *t, shape, lds=(260, 512, 264, 300, 272, 768))
    assert torch.equal(plain["dqk"], wide["dqk"]) and torch.equal(plain["dv"], wide["dv"])


def test_core_refusals_leave_outputs_untouched():
    shape = (1, 40, 33)
    dev = [t.to(DEV) for t in car.random_core(*shape, seed=2)]
    wsb = lambda *a: nat.call("gfc_attention_cross_backward_workspace_bytes", *a)  # noqa: E731
    need = wsb(*shape, 4)
    assert need == 2 * 1280  # lse 73 * 4 floats | D 73 * 4 floats, each slot rounded up to 256 bytes
    assert wsb(0, 40, 33, 4) == 0 and wsb(1, 0, 33, 4) == 0 and wsb(1, 40, 0, 4) == 0 and wsb(1, 40, 33, 8) == 0
    assert wsb(1, 8388606, 1, 4) > 0 and wsb(1, 8388607, 1, 4) == 0
    for kwargs, status in (({"ws_bytes": need - 1}, "GFC_ERR_WORKSPACE"), ({"ws_offset": 4}, "GFC_ERR_WORKSPACE"),
                           ({"heads": 8}, "GFC_ERR_INVALID"), ({"lds": (D, D, D, D, D, 258)}, "GFC_ERR_INVALID"),
                           ({"lds": (D, 252, D, D, D, D)}, "GFC_ERR_INVALID")):
        lds = kwargs.get("lds", (D,) * 6)
        out = [torch.full((73, max(ld, D)), NAN, device=DEV) for ld in lds[4:]]
        with pytest.raises(nat.NativeError, match=status):
            run_core(*dev, shape, out=out, **kwargs)
        assert all(bool(torch.isnan(o).all()) for o in out), kwargs
    for bad in ((0, 40, 33), (1, 0, 33), (1, 40, 0)):
        with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
            run_core(*dev, bad)


# ---- the block entry --------------------------------------------------------------------------------------------------
NAMES = ("dWqk", "dbqk", "dWv", "dbv")


def run_block(x, ctx, dctx, dx_in, p, shape, want_dx=True, ws_bytes=None, ws_offset=0, out=None):
    rows = x.shape[0]
    if out is None:
        out = {"dWqk": torch.full((D, D), NAN, device=DEV), "dbqk": torch.full((D,), NAN, device=DEV),
               "dWv": torch.full((D, D), NAN, device=DEV), "dbv": torch.full((D,), NAN, device=DEV),
               "dx": torch.full((rows, D), NAN, device=DEV) if want_dx else None}
    need = nat.call("gfc_lg_cross_attn_backward_workspace_bytes", *(max(s, 1) for s in shape))
    ws = torch.full(((need if ws_bytes is None else ws_bytes) + ws_offset,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[ws_offset:]
    try:
        nat.call("gfc_lg_cross_attn_backward", x, ctx, dctx, dx_in, p["Wqk"], p["bqk"], p["Wv"], p["bv"], *shape,
                 out["dWqk"], out["dbqk"], out["dWv"], out["dbv"], out["dx"], ws, ws.numel())
    finally:
        torch.cuda.synchronize()
    return out


def random_block(shape, seed):
    """x, ctx, dctx, dx_in float32 on the device and the parameters: ctx is the device's own forward in float64, rounded,
    dx_in two hundred times the attention's share, as on the fixtures."""
    b, m, n = shape
    g = torch.Generator().manual_seed(seed)
    rows = b * (m + n)
    p = {k: t.to(DEV) for k, t in car.random_params(g).items()}
    x = torch.randn((rows, D), generator=g).to(DEV)
    dctx = (torch.randn((rows, D), generator=g) * 1e-3).to(DEV)
    dx_in = (torch.randn((rows, D), generator=g) * 0.2).to(DEV)
    p64 = car.to64(p)
    qk, v = car.linear(x.double(), p64["Wqk"], p64["bqk"])[0], car.linear(x.double(), p64["Wv"], p64["bv"])[0]
    ctx = car.attention_forward(qk, v, b, m, n).float()
    return x, ctx, dctx, dx_in, p


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 700, 1400)),
                         ids=lambda s: "x".join(map(str, s)))
def test_block_matches_closed_form(shape):
    x, ctx, dctx, dx_in, p = random_block(shape, 40 + sum(shape))
    full, again = run_block(x, ctx, dctx, dx_in, p, shape), run_block(x, ctx, dctx, dx_in, p, shape)
    att, bare = run_block(x, ctx, dctx, None, p, shape), run_block(x, ctx, dctx, None, p, shape, want_dx=False)
    for k in NAMES + ("dx",):
        assert torch.equal(full[k], again[k]), k
    for k in NAMES:  # the parameter gradients do not depend on the row outputs asked for
        assert torch.equal(full[k], att[k]) and torch.equal(full[k], bare[k]), k
    want, errs = car.backward(x.double(), ctx.double(), dctx.double(), dx_in.double(), car.to64(p), *shape)
    tol = car.bounds(errs)
    got = dict(full, dx_att=att["dx"])
    report = {k: car.worst_ratio(got[k], want[k], tol[k]) for k in car.OUTPUTS}
    for k, r in report.items():
        WORST[k] = max(WORST.get(k, 0.0), r)
    print(f"block {shape}: fraction of the bound used: " + ", ".join(f"{k} {r:.3f}" for k, r in report.items()))
    assert max(report.values()) <= 1.0, report
    # the attention's share is tested on its own: the summed dx is 200 times larger and blind to it
    assert float(want["dx_att"].abs().max()) < 0.05 * float(want["dx"].abs().max())


def test_block_refusals_leave_outputs_untouched():
    shape = (1, 40, 33)
    x, ctx, dctx, dx_in, p = random_block(shape, 3)
    need = nat.call("gfc_lg_cross_attn_backward_workspace_bytes", *shape)
    assert need > 0 and nat.call("gfc_lg_cross_attn_backward_workspace_bytes", 0, 40, 33) == 0

    def fresh():
        return {"dWqk": torch.full((D, D), NAN, device=DEV), "dbqk": torch.full((D,), NAN, device=DEV),
                "dWv": torch.full((D, D), NAN, device=DEV), "dbv": torch.full((D,), NAN, device=DEV),
                "dx": torch.full((73, D), NAN, device=DEV)}

    for kwargs, status in (({"ws_bytes": need - 1}, "GFC_ERR_WORKSPACE"), ({"ws_offset": 4}, "GFC_ERR_WORKSPACE")):
        out = fresh()
        with pytest.raises(nat.NativeError, match=status):
            run_block(x, ctx, dctx, dx_in, p, shape, out=out, **kwargs)
        assert all(bool(torch.isnan(t).all()) for t in out.values()), kwargs
    for bad in ((0, 40, 33), (1, 40, 0)):
        out = fresh()
        with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
            run_block(x, ctx, dctx, dx_in, p, bad, out=out)
        assert all(bool(torch.isnan(t).all()) for t in out.values()), bad
    out = fresh()  # dx_in without dx, and dx_in as dx
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        run_block(x, ctx, dctx, dx_in, p, shape, out=dict(out, dx=None))
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        run_block(x, ctx, dctx, out["dx"], p, shape, out=out)
    assert all(bool(torch.isnan(t).all()) for t in out.values())


def test_zz_report_worst_fractions():
    print("cross-attention backward: largest fraction of a bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    assert WORST and max(WORST.values()) <= 1.0
