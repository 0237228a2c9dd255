"""gfc_lg_ffn_backward alone on the GPU, against the float64 closed form of tests/output_stage_reference.py evaluated on
the SAME bits: every output element within c 2^-23 abs-sum + the erf term (both derived there, from the shape alone; the
closed form runs in float64 torch on the device, so that the largest row count stays a matter of seconds).

Row counts at the edges of the plan: 1, 2, the k step of 16, the 128-row output tile and column-sum chunk, the 1024-row
split-K parts (2049: three parts), and 128 * 1024 + 17, just past the 128-part cap, where the parts grow to 1040 rows.
Two weight sets: a cross block with Wout, and the NULL-Wout form.  Conditioning rows on exact integer data in the manner
of tests/conditioning_cases.py.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import output_stage_reference as osr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
D, H = osr.D, osr.H
ROWS = (1, 2, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2049, 128 * 1024 + 17)
SHAPES = {"dWout": (D, D), "dbout": (D,), "dW0": (H, H), "db0": (H,), "dgamma": (H,), "dbeta": (H,), "dW3": (D, H),
          "db3": (D,)}
ERF_ABS = 0.0 if "exact_erf" in os.path.basename(nat.LIB_PATH) else osr.ERF_ABS
WORST = {}


def alloc(r, with_out, want_rows=True):
    """Every output, pre-filled with NaN."""
    out = {k: torch.full(s, NAN, device=DEV) for k, s in SHAPES.items() if with_out or k not in ("dWout", "dbout")}
    out["dx_in"] = torch.full((r, D), NAN, device=DEV) if want_rows else None
    out["dctx"] = torch.full((r, D), NAN, device=DEV) if want_rows else None
    return out


def run(x, ctx, dy, p, rows=None, ws_bytes=None, ws_offset=0, want_rows=True, out=None):
    """One call on device tensors; the workspace is filled with 0xFF bytes (NaNs) on entry."""
    r = x.shape[0] if rows is None else rows
    out = alloc(x.shape[0], p["Wout"] is not None, want_rows) if out is None else out
    need = nat.call("gfc_lg_ffn_backward_workspace_bytes", max(r, 1))
    ws = torch.full(((need if ws_bytes is None else ws_bytes) + ws_offset,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = ws[ws_offset:]
    try:
        nat.call("gfc_lg_ffn_backward", x, ctx, dy, p["Wout"], p["bout"], p["W0"], p["b0"], p["gamma"], p["beta"],
                 p["W3"], r, out.get("dWout"), out.get("dbout"), out["dW0"], out["db0"], out["dgamma"], out["dbeta"],
                 out["dW3"], out["db3"], out["dx_in"], out["dctx"], ws, ws.numel())
    finally:
        torch.cuda.synchronize()
    return out


def on_device(p, dtype=None):
    return {k: None if v is None else v.to(device=DEV, dtype=dtype or v.dtype).contiguous() for k, v in p.items()}


def check(tag, x, ctx, dy, p, exact_h=False):
    """x, ctx, dy, p: float32 on the host.  Two calls agree bit for bit; every output inside its bound."""
    xd, cd, dd, pd = x.to(DEV), ctx.to(DEV), dy.to(DEV), on_device(p)
    got, again = run(xd, cd, dd, pd), run(xd, cd, dd, pd)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{tag}: {k} differs between two calls"
    with_out = p["Wout"] is not None
    want, sums, erfs = osr.backward(xd.double(), cd.double(), dd.double(), on_device(p, torch.float64), exact_h=exact_h)
    tol = osr.bounds(sums, erfs, ERF_ABS)
    report = []
    for k in got:
        v = got[k].double().reshape(want[k].shape)
        assert bool(torch.isfinite(v).all()), f"{tag}: {k} is not finite"
        frac = osr.worst_ratio(v, want[k], tol[k])
        WORST[k] = max(WORST.get(k, 0.0), frac)
        report.append(f"{k} {frac:.3f}")
    print(f"{tag}: fraction of the bound used: " + ", ".join(report))
    for k in got:
        assert osr.worst_ratio(got[k].double().reshape(want[k].shape), want[k], tol[k]) <= 1.0, (tag, k, report)
    return got, want


def random_rows(r, seed, dy_sign=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((r, D), generator=g) / D ** 0.5
    ctx = torch.randn((r, D), generator=g) / D ** 0.5
    dy = torch.randn((r, D), generator=g) * 1e-3
    if dy_sign is not None:
        dy = dy.abs() * dy_sign
    return x, ctx, dy


@pytest.mark.parametrize("with_out", [True, False], ids=["wout", "null_wout"])
@pytest.mark.parametrize("r", ROWS)
def test_ffn_backward_matches_closed_form(r, with_out):
    p = osr.random_params(torch.Generator().manual_seed(7 + with_out), with_out)
    check(f"R={r} {'Wout' if with_out else 'NULL'}", *random_rows(r, 100 + r), p)


def test_ffn_backward_negative_dy():
    p = osr.random_params(torch.Generator().manual_seed(3), True)
    check("negative dy", *random_rows(257, 5, dy_sign=-1.0), p)


COND_R, COL_POS, COL_NEG = osr.COND_R, osr.COL_POS, osr.COL_NEG
conditioning_case = osr.conditioning_case


@pytest.mark.parametrize("offset", [4096, 0])
def test_ffn_backward_conditioning_rows(offset):
    x, ctx, dy, p = conditioning_case(offset)
    got, want = check(f"conditioning offset {offset}", x, ctx, dy, p, exact_h=True)
    # u = +1e4: the derivative is exactly 1, so dbeta is the column sum of da; u = -1e4: exactly 0.  gamma = 0: dn = 0.
    assert torch.equal(got["dbeta"][COL_NEG], torch.zeros(4, device=DEV))
    assert torch.equal(got["dgamma"][COL_NEG], torch.zeros(4, device=DEV))
    # (u = +1e4: u phi(u) is exactly 0, not inf * 0 -- dbeta there is the column sum of da, held by its bound above)
    assert bool(torch.isfinite(got["dbeta"][COL_POS]).all()) and bool((got["dbeta"][COL_POS] != 0).all())
    # the one-pass variance would fail the offset rows: stated by the host test on the same case


def test_ffn_backward_zero_dy_gives_exact_zeros():
    x, ctx, _, p = conditioning_case(4096)
    r = osr.random_params(torch.Generator().manual_seed(5), True)
    for tag, params in (("conditioning", p), ("random", r)):
        got = run(x.to(DEV), ctx.to(DEV), torch.zeros((COND_R, D), device=DEV), on_device(params))
        for k, v in got.items():
            assert bool((v == 0).all()), (tag, k)


def test_ffn_backward_without_row_outputs():
    """dx_in and dctx are optional: the parameter gradients are the same bits without them."""
    p = on_device(osr.random_params(torch.Generator().manual_seed(9), True))
    x, ctx, dy = (t.to(DEV) for t in random_rows(300, 21))
    full, bare = run(x, ctx, dy, p), run(x, ctx, dy, p, want_rows=False)
    for k in SHAPES:
        assert torch.equal(full[k], bare[k]), k


def test_ffn_backward_refusals_leave_outputs_untouched():
    p = on_device(osr.random_params(torch.Generator().manual_seed(9), True))
    x, ctx, dy = (t.to(DEV) for t in random_rows(130, 22))
    need = nat.call("gfc_lg_ffn_backward_workspace_bytes", 130)
    assert need > 0 and nat.call("gfc_lg_ffn_backward_workspace_bytes", 0) == 0
    assert nat.call("gfc_lg_ffn_backward_workspace_bytes", 8388607) > 0
    assert nat.call("gfc_lg_ffn_backward_workspace_bytes", 8388608) == 0
    for kwargs, status in (({"ws_bytes": need - 1}, "GFC_ERR_WORKSPACE"), ({"ws_offset": 4}, "GFC_ERR_WORKSPACE"),
                           ({"rows": 0}, "GFC_ERR_INVALID")):
        out = alloc(130, True)
        with pytest.raises(nat.NativeError, match=status):
            run(x, ctx, dy, p, out=out, **kwargs)
        assert len(out) == 10 and all(bool(torch.isnan(t).all()) for t in out.values()), kwargs
    # Wout without its gradient buffers, and the other way round
    q = dict(p, Wout=None, bout=None)
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        nat.call("gfc_lg_ffn_backward", x, ctx, dy, q["Wout"], q["bout"], p["W0"], p["b0"], p["gamma"], p["beta"], p["W3"],
                 130, torch.empty((D, D), device=DEV), torch.empty((D,), device=DEV), torch.empty((H, H), device=DEV),
                 torch.empty((H,), device=DEV), torch.empty((H,), device=DEV), torch.empty((H,), device=DEV),
                 torch.empty((D, H), device=DEV), torch.empty((D,), device=DEV), None, None,
                 torch.empty((need,), dtype=torch.uint8, device=DEV), need)
    torch.cuda.synchronize()


def test_zz_report_worst_fractions():
    print("gfc_lg_ffn_backward: largest fraction of a bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    assert WORST and max(WORST.values()) <= 1.0
