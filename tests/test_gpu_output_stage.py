"""The last layer's output stage on the GPU: gfc_lg_layer_pairs_keep, `forward_layers(keep_output_stage=True)`,
`layer_loss_backward(output_stage=True)` and `output_stage_updated()`.

The kept tensors are checked by completing the block from them with the forward's own entry points on the packed
weights: that reproduces the layer's output bit for bit.  The eight gradients and the two row outputs are compared with
the float64 closed form of tests/output_stage_reference.py on the device's own kept tensors and its own head gradient
(the same bits), per element within c 2^-23 abs-sum + the erf term.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402
import output_stage_reference as osr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 0.05  # the step of the descent check, as tests/test_gpu_head_backward.py takes it
L = lc.N_LAYERS
PRE = f"transformers.{L - 1}.cross_attn."
NAMES = {"to_out.weight": "dWout", "to_out.bias": "dbout", "ffn.0.weight": "dW0", "ffn.0.bias": "db0",
         "ffn.1.weight": "dgamma", "ffn.1.bias": "dbeta", "ffn.3.weight": "dW3", "ffn.3.bias": "db3"}
KEPT = ("output_stage_rows0", "output_stage_rows1", "output_stage_context0", "output_stage_context1")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = int(np.load(os.path.join(GOLDEN, "layer_loss.npz"))["seed"])  # the seed the fixtures were made at
ERF_ABS = 0.0 if "exact_erf" in os.path.basename(nat.LIB_PATH) else osr.ERF_ABS


def model(**conf):
    return lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.0, **conf}).eval().cuda()


def inputs(case):
    c = lambda k: case[k].cuda()  # noqa: E731
    return {"keypoints0": c("keypoints0"), "keypoints1": c("keypoints1"), "descriptors0": c("descriptors0"),
            "descriptors1": c("descriptors1"), "view0": {"image_size": c("size")}, "view1": {"image_size": c("size")}}


def labels(case):
    out = {"gt_matches0": case["gt_matches0"].cuda(), "gt_matches1": case["gt_matches1"].cuda()}
    if case["gt_assignment"] is not None:
        out["gt_assignment"] = case["gt_assignment"].cuda()
    return out


def random_batch(b, m, n, seed):
    g = torch.Generator().manual_seed(seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)  # noqa: E731
    size = torch.tensor([[640.0, 480.0]]).expand(b, 2).contiguous().cuda()
    return {"keypoints0": (torch.rand((b, m, 2), generator=g) * 400).cuda(),
            "keypoints1": (torch.rand((b, n, 2), generator=g) * 400).cuda(),
            "descriptors0": unit(torch.randn((b, m, 256), generator=g)).cuda(),
            "descriptors1": unit(torch.randn((b, n, 256), generator=g)).cuda(),
            "view0": {"image_size": size}, "view1": {"image_size": size}}


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("shape", [(2, 130, 65), (8, 300, 257), (8, 1024, 1024)],
                         ids=["2x130x65", "8x300x257_stored_sim", "8x1024x1024_fused_ffn"])
def test_keep_is_the_default_forward_and_completes_the_block(shape, fold):
    b, m, n = shape
    lg = model(fold_out_proj=fold)
    data = random_batch(b, m, n, 3)
    with torch.no_grad():
        plain, kept = lg.forward_layers(data), lg.forward_layers(data, keep_output_stage=True)
    assert set(kept) == set(plain) | set(KEPT)
    for k in plain:
        assert torch.equal(plain[k], kept[k]), k
    rows = b * (m + n)
    x_mid = torch.cat([kept["output_stage_rows0"].reshape(-1, 256), kept["output_stage_rows1"].reshape(-1, 256)], 0)
    ctx = torch.cat([kept["output_stage_context0"].reshape(-1, 256), kept["output_stage_context1"].reshape(-1, 256)], 0)
    assert kept["output_stage_rows0"].shape == (b, m, 256) and kept["output_stage_context1"].shape == (b, n, 256)
    assert kept["output_stage_rows1"].data_ptr() == kept["output_stage_rows0"].data_ptr() + b * m * 256 * 4  # one buffer
    # the rest of the cross block from (x_mid, ctx), with the forward's entry points on the packed weights
    p, l = lg.ensure_packed(torch.device(DEV, 0))[0], L - 1
    msg = ctx
    if not fold:
        msg = torch.empty((rows, 256), device=DEV)
        nat.call("gfc_linear", ctx, 256, 256, None, 0, 0, p.c_out_w[l], 256, p.c_out_b[l], None, None, 1.0, None, None,
                 None, 0, msg, 256, rows, 256)
    want = torch.cat([kept["ref_descriptors0"][:, l].reshape(-1, 256), kept["ref_descriptors1"][:, l].reshape(-1, 256)], 0)
    # Below 128 x 128 rows the layer runs ffn[0], the LayerNorm + GELU and ffn[3] as gfc_linear + gfc_layernorm_gelu +
    # gfc_linear; from there on as gfc_ffn_fused, whose bits are those of gfc_linear_layernorm_gelu + gfc_linear
    # (tests/conditioning_cases.py).  The form the layer took reproduces x bit for bit; the other one is the same
    # function in another order of fp32 operations and its distance is printed.
    taken = "fused" if rows >= 128 * 128 else "two_launches"
    for first in ("fused", "two_launches"):
        h = torch.empty((rows, 512), device=DEV)
        if first == "fused":
            nat.call("gfc_linear_layernorm_gelu", x_mid, 256, 256, msg, 256, 256, p.c_ffn0_w[l], 512, p.c_ffn0_b[l],
                     p.c_ln_g[l], p.c_ln_b[l], h, 512, rows, 512)
        else:
            nat.call("gfc_linear", x_mid, 256, 256, msg, 256, 256, p.c_ffn0_w[l], 512, p.c_ffn0_b[l], None, None, 1.0, None,
                     None, None, 0, h, 512, rows, 512)
            nat.call("gfc_layernorm_gelu", h, 512, rows, 512, p.c_ln_g[l], p.c_ln_b[l])
        y = torch.empty((rows, 256), device=DEV)
        nat.call("gfc_linear", h, 512, 512, None, 0, 0, p.c_ffn3_w[l], 512, p.c_ffn3_b[l], None, None, 1.0, x_mid, None,
                 None, 0, y, 256, rows, 256)
        torch.cuda.synchronize()
        if first == taken:
            assert torch.equal(y, want), first
        else:
            print(f"{b} x ({m} + {n}), fold {fold}: the layer took {taken}; {first} differs from it by at most "
                  f"{float((y - want).abs().max()):.3g} of values up to {float(want.abs().max()):.3g}")
            assert float((y - want).abs().max()) <= 1e-4 * float(want.abs().max())


def layer_call(lg, b, m, n, seed):
    """What one gfc_lg_layer_pairs call takes for a uniform batch, built as forward_layers builds it: (packed parameters,
    rows x [B*M + B*N, 256], cos, sin, self and cross problem tables, a workspace)."""
    data = random_batch(b, m, n, seed)
    params = lg.ensure_packed(torch.device(DEV, 0))[0]
    rows = b * (m + n)
    x = torch.cat([data["descriptors0"].reshape(-1, 256), data["descriptors1"].reshape(-1, 256)], 0).contiguous()
    kp = torch.cat([data["keypoints0"].reshape(-1, 2), data["keypoints1"].reshape(-1, 2)], 0).contiguous()
    r0 = torch.arange(b, dtype=torch.int32) * m
    r1 = b * m + torch.arange(b, dtype=torch.int32) * n
    cm, cn = torch.full_like(r0, m), torch.full_like(r1, n)
    self_p = torch.cat([torch.stack([r0, cm, r0, cm], 1), torch.stack([r1, cn, r1, cn], 1)], 0).contiguous().to(DEV)
    cross_p = torch.cat([torch.stack([r0, cm, r1, cn], 1), torch.stack([r1, cn, r0, cm], 1)], 0).contiguous().to(DEV)
    row0, cnt = torch.cat([r0, r1]).to(DEV), torch.cat([cm, cn]).to(DEV)
    sizes = torch.cat([data["view0"]["image_size"], data["view1"]["image_size"]], 0).contiguous()
    cos, sin = torch.empty((rows, 64), device=DEV), torch.empty((rows, 64), device=DEV)
    nat.call("gfc_lg_posenc", kp, None, sizes, row0, cnt, 2 * b, max(m, n), params.posenc_wr, 2, cos, sin)
    ws = torch.empty(nat.call("gfc_lg_layer_pairs_workspace_bytes", b, m, n), dtype=torch.uint8, device=DEV)
    return params, x, cos, sin, self_p, cross_p, ws


@pytest.mark.parametrize("shape", [(2, 130, 65), (8, 300, 257)], ids=["2x130x65", "8x300x257_stored_sim"])
def test_the_keep_entry_is_gfc_lg_layer_pairs(shape):
    """gfc_lg_layer_pairs_keep called directly: x is gfc_lg_layer_pairs' bit for bit, on a middle layer too."""
    import ctypes

    b, m, n = shape
    lg = model()  # (kept alive: `params` holds raw pointers into its packed weights)
    params, x, cos, sin, self_p, cross_p, ws = layer_call(lg, b, m, n, 5)
    for layer in (3, L - 1):
        plain, kept = x.clone(), x.clone()
        mid, ctx = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        nat.call("gfc_lg_layer_pairs", ctypes.byref(params), layer, plain, cos, sin, b, m, n, self_p, cross_p, ws, ws.numel())
        nat.call("gfc_lg_layer_pairs_keep", ctypes.byref(params), layer, kept, cos, sin, b, m, n, self_p, cross_p, mid, ctx,
                 ws, ws.numel())
        torch.cuda.synchronize()
        assert torch.equal(plain, kept) and not torch.equal(plain, x)
        assert bool(torch.isfinite(mid).all()) and bool(torch.isfinite(ctx).all()) and not torch.equal(mid, kept)


def test_keep_refuses_fp16_and_null_outputs():
    import ctypes

    lg = model(matmul_precision="fp16")
    with pytest.raises(NotImplementedError, match="fp32"):
        lg.forward_layers(random_batch(1, 16, 16, 1), keep_output_stage=True)
    b, m, n = 1, 16, 16
    for net, args in ((model(), "null"), (lg, "fp16")):
        params, x, cos, sin, self_p, cross_p, ws = layer_call(net, b, m, n, 2)
        before = x.clone()
        mid, ctx = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        for pair in ([(None, ctx), (mid, None)] if args == "null" else [(mid, ctx)]):
            with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
                nat.call("gfc_lg_layer_pairs_keep", ctypes.byref(params), 0, x, cos, sin, b, m, n, self_p, cross_p, *pair,
                         ws, ws.numel())
        torch.cuda.synchronize()
        assert torch.equal(x, before) and bool(torch.isnan(mid).all()) and bool(torch.isnan(ctx).all())  # before any launch


@pytest.fixture(scope="module", params=["a", "b"])
def fx(request):
    """A case of tests/layer_loss_cases.py and ONE kept prediction shared by the tests (never changed)."""
    seed = int(np.load(os.path.join(GOLDEN, f"output_stage_{request.param}_gamma1.npz"))["seed"])  # the fixture's own
    case = lc.make_case(request.param, seed)
    lg = model()
    with torch.no_grad():
        pred = lg.forward_layers(inputs(case), keep_output_stage=True)
    torch.cuda.synchronize()
    return request.param, case, pred


@pytest.mark.parametrize("gamma", [0.5, 1.0])
def test_output_stage_gradients_against_the_closed_form(fx, gamma):
    name, case, pred = fx
    lg = model(loss={"gamma": gamma})
    plain = lg.layer_loss_backward(pred, labels(case), descriptor_grads=True, accumulate=False)
    grads = lg.layer_loss_backward(pred, labels(case), descriptor_grads=True, accumulate=False, output_stage=True)
    lean = lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True)
    torch.cuda.synchronize()
    extra = {PRE + k for k in NAMES} | {"grad_" + k for k in KEPT}
    assert set(grads) == set(plain) | extra and set(lean) == set(grads) - {"grad_ref_descriptors0", "grad_ref_descriptors1"}
    for k in plain:  # nothing that was returned before has changed
        assert torch.equal(plain[k], grads[k]), k
    for k in lean:   # the head gradient taken for the last layer alone is the same bits
        assert torch.equal(lean[k], grads[k]), k
    flat = lambda a, b: torch.cat([a.reshape(-1, 256), b.reshape(-1, 256)], 0).double()  # noqa: E731
    x = flat(pred["output_stage_rows0"], pred["output_stage_rows1"])
    ctx = flat(pred["output_stage_context0"], pred["output_stage_context1"])
    dy = flat(grads["grad_ref_descriptors0"][:, L - 1], grads["grad_ref_descriptors1"][:, L - 1])
    sd = lg.state_dict()
    p = {"Wout": sd[PRE + "to_out.weight"], "bout": sd[PRE + "to_out.bias"], "W0": sd[PRE + "ffn.0.weight"],
         "b0": sd[PRE + "ffn.0.bias"], "gamma": sd[PRE + "ffn.1.weight"], "beta": sd[PRE + "ffn.1.bias"],
         "W3": sd[PRE + "ffn.3.weight"], "b3": sd[PRE + "ffn.3.bias"]}
    p = {k: v.detach().double() for k, v in p.items()}
    # the kept tensors are the block's: its output is the layer's descriptors, to fp32 rounding of the folded weights
    y = osr.forward(x, ctx, p)
    last = flat(pred["ref_descriptors0"][:, L - 1], pred["ref_descriptors1"][:, L - 1])
    assert float((y - last).abs().max()) < 1e-4 * float(last.abs().max())
    want, sums, erfs = osr.backward(x, ctx, dy, p)
    tol = osr.bounds(sums, erfs, ERF_ABS)
    got = {v: grads[PRE + k] for k, v in NAMES.items()}
    got["dx_in"] = flat(grads["grad_output_stage_rows0"], grads["grad_output_stage_rows1"])
    got["dctx"] = flat(grads["grad_output_stage_context0"], grads["grad_output_stage_context1"])
    report = {k: osr.worst_ratio(got[k].double().reshape(want[k].shape), want[k], tol[k]) for k in want}
    print(f"case {name} gamma {gamma}: fraction of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))
    assert max(report.values()) <= 1.0, report
    # the reference's own autograd (float64 run): the kept tensors and the head gradient come from another evaluation of
    # the trunk, whose float32 error (head_grad_reference.trunk_c) and the head's own (head_c, dx) they arrive with
    z = np.load(os.path.join(GOLDEN, f"output_stage_{name}_gamma{'05' if gamma == 0.5 else '1'}.npz"))
    assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"])) and float(z["gamma"]) == gamma
    b, m, n = case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1]
    arrive = hg.trunk_c(L) + hg.head_c(b, m, n)["dx"]
    _, sums, erfs = osr.backward(x, ctx, dy, p, in_err=arrive)
    tol = osr.bounds(sums, erfs, ERF_ABS)
    t = lambda k: torch.from_numpy(z[k]).double().to(DEV)  # noqa: E731
    ref = {}
    for key, out in (("bout", "dbout"), ("b0", "db0"), ("gamma_", "dgamma"), ("beta", "dbeta"), ("b3", "db3")):
        ref[out] = osr.worst_ratio(got[out].double(), t(key), tol[out])
    for key, out in (("wout", "dWout"), ("w0", "dW0"), ("w3", "dW3")):
        rows_, cols = torch.from_numpy(z[key + "_pick_rows"]).to(DEV), torch.from_numpy(z[key + "_pick_cols"]).to(DEV)
        u, v = t(key + "_u"), t(key + "_v")
        g = got[out].double()
        ref[out] = max(osr.worst_ratio(g[rows_], t(key + "_rows"), tol[out][rows_]),
                       osr.worst_ratio(g[:, cols], t(key + "_cols"), tol[out][:, cols]),
                       float((u @ g @ v - float(z[key + "_bilinear"])).abs() / (u.abs() @ tol[out] @ v.abs())))
    r0, r1 = torch.from_numpy(z["rows0"]).to(DEV), torch.from_numpy(z["rows1"]).to(DEV) + b * m
    ref["dctx"] = max(osr.worst_ratio(got["dctx"][r0], t("dctx0"), tol["dctx"][r0]),
                      osr.worst_ratio(got["dctx"][r1], t("dctx1"), tol["dctx"][r1]))
    print(f"case {name} gamma {gamma}: against the reference's autograd: " + ", ".join(f"{k} {v:.3f}" for k, v in ref.items()))
    assert max(ref.values()) <= 1.0, ref
    for k in NAMES:
        assert grads[PRE + k].shape == lg.get_parameter(PRE + k).shape, k
    b, m, n = case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1]
    assert grads["grad_output_stage_rows0"].shape == (b, m, 256) and grads["grad_output_stage_context1"].shape == (b, n, 256)


def test_output_stage_accumulates_and_refuses(fx):
    _, case, pred = fx
    lg = model()
    once = lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True)
    assert all(q.grad is None for q in lg.parameters())
    lg.layer_loss_backward(pred, labels(case), output_stage=True)
    lg.layer_loss_backward(pred, labels(case), output_stage=True)
    for k in NAMES:
        q, g = lg.get_parameter(PRE + k), once[PRE + k]
        assert q.grad.shape == q.shape and bool(((q.grad - 2 * g).abs() <= 2.0 ** -22 * g.abs()).all()), k
    named = {k for k in once if not k.startswith("grad_")}
    assert all(q.grad is None for k, q in lg.named_parameters() if k not in named)
    bare = {k: v for k, v in pred.items() if k not in KEPT}
    with pytest.raises(ValueError, match="keep_output_stage"):
        lg.layer_loss_backward(bare, labels(case), accumulate=False, output_stage=True)
    with pytest.raises(NotImplementedError, match="fp32 matcher"):
        model(matmul_precision="fp16").layer_loss_backward(pred, labels(case), output_stage=True)


@pytest.mark.parametrize("where", ["cuda", "cpu", "fp16", "graph", "unfolded", "unfolded_cpu"])
def test_sgd_step_output_stage_updated_and_descent(where):
    """An SGD step of EPS on the heads, the tokens and the eight tensors, `heads_updated()` + `output_stage_updated()`,
    and `forward`, `forward_layers` and `forward_pairs` are what a fresh module loaded from `state_dict()` gives; the loss
    has fallen by EPS |grad|^2 within [0.9, 1.1], as tests/test_gpu_head_backward.py asks of the heads."""
    case = lc.make_case("a", SEED)
    conf = {"weights": "synthetic", "filter_threshold": 0.0}
    if where == "fp16":
        conf["matmul_precision"] = "fp16"
    if where == "graph":
        conf["graph_max_rows"] = 4096
    if where.startswith("unfolded"):
        conf["fold_out_proj"] = False
    lg = lightglue.LightGlue(conf).eval()
    if not where.endswith("cpu"):
        lg = lg.cuda()
    data = inputs(case)
    size = case["size"][:1].cuda()
    items = [{"keypoints0": data["keypoints0"][i:i + 1], "keypoints1": data["keypoints1"][i:i + 1],
              "descriptors0": data["descriptors0"][i:i + 1], "descriptors1": data["descriptors1"][i:i + 1],
              "view0": {"image_size": size}, "view1": {"image_size": size}} for i in range(2)]
    donor = model(fold_out_proj=conf.get("fold_out_proj", True)) if where == "fp16" else lg
    with torch.no_grad():
        plain = lg(data)
        pred = donor.forward_layers(data, keep_output_stage=True)
        before, _ = donor.layer_loss(pred, labels(case))
    grads = donor.layer_loss_backward(pred, labels(case), output_stage=True, accumulate=where != "fp16")
    grads = {k: g for k, g in grads.items() if not k.startswith("grad_")}
    if where == "fp16":  # gradients are built for the fp32 matcher: they come from an fp32 module of the same weights
        for k, g in grads.items():
            lg.get_parameter(k).grad = g.clone()
    assert len(grads) == 4 * L + 2 * (L - 1) + 8
    frozen = {k: v.detach().clone() for k, v in lg.state_dict().items() if k not in grads}
    opt = torch.optim.SGD([q for k, q in lg.named_parameters() if k in grads], lr=EPS)
    opt.step()
    lg.heads_updated()
    lg.output_stage_updated()
    for k, v in frozen.items():
        assert torch.equal(lg.state_dict()[k], v), k
    fresh = lightglue.LightGlue(conf).eval()
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in lg.state_dict().items()})
    if not where.endswith("cpu"):
        fresh = fresh.cuda()
    with torch.no_grad():
        new, want = lg.forward_layers(data), fresh.forward_layers(data)
        new_plain, want_plain = lg(data), fresh(data)
        new_pairs, want_pairs = lg.forward_pairs(items), fresh.forward_pairs(items)
    for k in want:
        assert torch.equal(new[k], want[k]), k
        assert torch.equal(new_plain[k], want_plain[k]), k
    for a, b in zip(new_pairs, want_pairs):
        for k in b:
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(new_plain["log_assignment"], plain["log_assignment"])
    assert torch.equal(new["ref_descriptors0"][:, :L - 1], pred["ref_descriptors0"][:, :L - 1]) or where == "fp16"
    assert not torch.equal(new["ref_descriptors0"][:, L - 1], pred["ref_descriptors0"][:, L - 1])  # the stage has moved
    if where != "fp16":
        with torch.no_grad():
            after, _ = fresh.cuda().layer_loss(fresh.forward_layers(data), labels(case))
        sq = sum(float((g.double() ** 2).sum()) for g in grads.values())
        ratio = float((after["total"].double().mean() - before["total"].double().mean())) / (-EPS * sq)
        print(f"{where}: descent ratio {ratio:.4f}: total {float(before['total'].mean()):.6f} -> "
              f"{float(after['total'].mean()):.6f}, |grad|^2 {sq:.4e}")
        assert 0.9 <= ratio <= 1.1
    # a second backward reads the refreshed unfolded copies: it is the fresh module's
    if where != "fp16":
        again = lg.layer_loss_backward(lg.forward_layers(data, keep_output_stage=True), labels(case), accumulate=False,
                                       output_stage=True)
        ref = fresh.layer_loss_backward(fresh.forward_layers(data, keep_output_stage=True), labels(case),
                                        accumulate=False, output_stage=True)
        for k in ref:
            assert torch.equal(again[k], ref[k]), k


@pytest.mark.parametrize("name", ["a", "b"])
def test_descent_matches_the_float64_ratio(name):
    """An SGD step of osr.DESCENT_EPS on the eight tensors alone + `output_stage_updated()`: `total - confidence` (the
    part of the loss they move smoothly; the host test says why) falls by the float64 ratio the host test measures and
    records (osr.DESCENT_RATIO) times eps |grad|^2.  Allowed distance: 0.005 for what the trunk's float32 error does to
    the gradient and the curvature (both relative errors of 1e-4 to 1e-3 of terms of order 1), plus 32 roundings of
    2^-23 of the loss value against the size of the difference: the two losses are float32 numbers, each the end of a
    chain of sums whose errors are largely but not wholly common to both."""
    seed = int(np.load(os.path.join(GOLDEN, f"output_stage_{name}_gamma1.npz"))["seed"])
    case = lc.make_case(name, seed)
    lg = model(loss={"gamma": 1.0})
    data, eps = inputs(case), osr.DESCENT_EPS
    smooth = lambda losses: float((losses["total"].double() - losses["confidence"].double()).mean())  # noqa: E731
    with torch.no_grad():
        pred = lg.forward_layers(data, keep_output_stage=True)
        before = smooth(lg.layer_loss(pred, labels(case))[0])
    grads = lg.layer_loss_backward(pred, labels(case), output_stage=True, accumulate=False)
    stage = {PRE + k: grads[PRE + k] for k in NAMES}
    with torch.no_grad():
        for k, g in stage.items():
            lg.get_parameter(k).sub_(eps * g)
    lg.output_stage_updated()
    with torch.no_grad():
        after = smooth(lg.layer_loss(lg.forward_layers(data), labels(case))[0])
    sq = sum(float((g.double() ** 2).sum()) for g in stage.values())
    ratio = (after - before) / (-eps * sq)
    allowed = 0.005 + 32 * osr.U * abs(before) / (eps * sq)
    print(f"case {name}: descent ratio {ratio:.4f} (float64: {osr.DESCENT_RATIO[name]:.4f}, allowed distance "
          f"{allowed:.4f}): {before:.6f} -> {after:.6f}, |grad|^2 {sq:.4e}")
    assert abs(ratio - osr.DESCENT_RATIO[name]) <= allowed


def test_finetune_heads_with_the_output_stage(tmp_path, capsys):
    import shutil

    import endopatches_reference as er

    from glue_factory_colon_amd import finetune_heads, weights

    names = er.make_tree(tmp_path, per_sequence=3, hw=(120, 160))
    for n in names:
        shutil.copy(tmp_path / "frames" / "test" / n, tmp_path / "frames" / "val" / n)
    common = ["--data_dir", str(tmp_path / "frames"), "--pair_batch", "4", "--max_num_keypoints", "128", "--num_workers",
              "0", "--optimizer", "sgd", "--lr", "0.01", "--epochs", "2", "--max_steps", "2"]
    out = tmp_path / "tuned.pth"
    before, after = finetune_heads.main(common + ["--params", "all+output_stage", "--out", str(out)])
    capsys.readouterr()
    print(f"loss/total_deep {before['loss/total_deep']:.6f} -> {after['loss/total_deep']:.6f}")
    assert after["loss/total_deep"] < before["loss/total_deep"]
    tuned = torch.load(str(out), map_location="cpu")
    start = weights.lightglue_state_dict(0)
    moved = {k for k, v in start.items() if k in tuned and not torch.equal(tuned[k], v)}
    stage = {PRE + k for k in NAMES}
    assert stage <= moved and all(k in stage or k.startswith(("log_assignment.", "token_confidence.")) for k in moved)
    loaded = lightglue.LightGlue({"weights": str(out)}).eval().cuda()
    for k, v in tuned.items():
        assert torch.equal(loaded.state_dict()[k].cpu(), v), k
    # the saved state dict reloads to the tuned forward: a fresh pipeline on the file (its `_pack` folds the tuned to_out
    # into ffn[0]), no step taken, reports every loss and metric the tuner reported after its last step, bit for bit
    again, _ = finetune_heads.main(common[:-2]  # (without "--max_steps 2")
                                   + ["--matcher_weights", str(out), "--max_steps", "0", "--params", "all", "--out",
                                      str(tmp_path / "unused.pth")])
    capsys.readouterr()
    assert set(again) == set(after) and again["loss/total_deep"] == after["loss/total_deep"]
    for k in (k for k in after if k.startswith(("loss/", "layer/"))):
        assert again[k] == after[k] or (after[k] != after[k] and again[k] != again[k]), k
    only = tmp_path / "stage_only.pth"
    finetune_heads.main(common + ["--params", "output_stage", "--out", str(only)])
    moved = {k for k, v in start.items() if not torch.equal(torch.load(str(only), map_location="cpu")[k], v)}
    assert moved == stage
    # --params all still leaves the eight tensors as they were
    plain = tmp_path / "all.pth"
    finetune_heads.main(common + ["--params", "all", "--out", str(plain)])
    kept = torch.load(str(plain), map_location="cpu")
    for k in stage:
        assert torch.equal(kept[k], start[k]), k
