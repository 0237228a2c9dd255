"""The last self block's backward through the module on the GPU: `forward_layers(keep_self_block=True)`,
`layer_loss_backward(..., self_block=True)`, `self_block_updated()` and `finetune_heads --params last_layer`.

The ten gradients of `transformers.{L-1}.self_attn.` and the gradient at the layer's input rows are compared
  * with the float64 closed forms of tests/output_stage_reference.py (the FFN part) and tests/self_block_grad_reference.py
    (rotary attention and Wqkv) on the device's own kept tensors and its own `grad_cross_block_rows` (the same bits), per
    element within 2^-23 times the error sum: the SHARP comparison;
  * with torch's float64 autograd of the WHOLE last layer (self block and cross block as the reference writes them,
    lightglue.py:124-164,193-222) from the device's rows of layer L - 2 and head L - 1's direct gradient: this one
    re-evaluates the layer's forward in float64, so the float32 error of the kept tensors arrives as an input error.  It is
    loose (TOL_LAYER below) and pins the wiring: which rows, which gradient goes where, the row order of Wqkv.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_loss_cases as lc  # noqa: E402
import output_stage_reference as osr  # noqa: E402
import self_block_grad_reference as sbr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 0.05  # the SGD step of the refresh test, as tests/test_gpu_output_stage.py takes it
L = lc.N_LAYERS
SELF = f"transformers.{L - 1}.self_attn."
CROSS = f"transformers.{L - 1}.cross_attn."
STAGE = {"out_proj.weight": "dWout", "out_proj.bias": "dbout", "ffn.0.weight": "dW0", "ffn.0.bias": "db0",
         "ffn.1.weight": "dgamma", "ffn.1.bias": "dbeta", "ffn.3.weight": "dW3", "ffn.3.bias": "db3"}
TEN = tuple(STAGE) + ("Wqkv.weight", "Wqkv.bias")
ROWS = ("grad_self_block_rows0", "grad_self_block_rows1", "grad_layer_input_rows0", "grad_layer_input_rows1")
KEPT = ("self_block_context0", "self_block_context1", "self_block_cos", "self_block_sin")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = int(np.load(os.path.join(GOLDEN, "layer_loss.npz"))["seed"])
ERF_ABS = 0.0 if "exact_erf" in os.path.basename(nat.LIB_PATH) else osr.ERF_ABS
# Against the float64 re-evaluation of the whole layer, per tensor, relative to its largest element.  The kept rows and
# contexts are float32 results of depth-256 / depth-512 products and two soft-maxes: about 1e-6 of their size.  The
# gradients are sums in which terms cancel (P (dP - D): the Wqkv gradient is two orders smaller than its addends), which
# leaves 1e-4, and that is what is allowed.  The per-element comparisons with carried error sums are the same-bits one
# above and the one against the reference's fixtures below; this one pins the wiring of the whole layer.
TOL_LAYER = 1e-4


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


def flat(a, b):
    return torch.cat([a.reshape(-1, 256), b.reshape(-1, 256)], 0).double()


ALL_ON = {"output_stage": True, "cross_attention": True, "self_block": True}


@pytest.fixture(scope="module", params=["a", "b"])
def fx(request):
    """A case of tests/layer_loss_cases.py and ONE kept prediction shared by the tests (never changed)."""
    seed = int(np.load(os.path.join(GOLDEN, f"self_block_grad_{request.param}_gamma1.npz"))["seed"])  # the fixture's own
    case = lc.make_case(request.param, seed)
    lg = model()
    with torch.no_grad():
        pred = lg.forward_layers(inputs(case), keep_output_stage=True, keep_self_block=True)
    torch.cuda.synchronize()
    return request.param, case, pred


def test_keep_self_block_is_the_default_forward(fx):
    _, case, kept = fx
    lg = model()
    b, m, n = case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1]
    with torch.no_grad():
        plain, stage = lg.forward_layers(inputs(case)), lg.forward_layers(inputs(case), keep_output_stage=True)
    assert set(kept) == set(stage) | set(KEPT) and set(plain) < set(stage)
    for k in stage:
        assert torch.equal(stage[k], kept[k]), k
    assert kept["self_block_context0"].shape == (b, m, 256) and kept["self_block_context1"].shape == (b, n, 256)
    assert kept["self_block_cos"].shape == kept["self_block_sin"].shape == (b * (m + n), 64)
    with pytest.raises(ValueError, match="keep_output_stage"):
        lg.forward_layers(inputs(case), keep_self_block=True)
    with pytest.raises(NotImplementedError, match="fp32"):
        model(matmul_precision="fp16").forward_layers(inputs(case), keep_output_stage=True, keep_self_block=True)
    empty = dict(inputs(case), keypoints0=case["keypoints0"][:, :0].cuda(), descriptors0=case["descriptors0"][:, :0].cuda())
    with torch.no_grad():
        e = lg.forward_layers(empty, keep_output_stage=True, keep_self_block=True)
    assert e["self_block_context0"].shape == (b, 0, 256) and e["self_block_context1"].shape == (b, n, 256)
    assert e["self_block_cos"].shape == (b * n, 64) and not bool(e["self_block_context1"].any())


def layer_autograd(lg, x_in, cos, sin, dy, shape):
    """torch float64 autograd of sum(y * dy), y the last layer's output on x_in as the reference writes the layer
    (lightglue.py:124-164,193-222): {state-dict name: gradient} of its 22 tensors, and the gradient at x_in."""
    b, m, n = shape
    sd = {k: v.detach().double().requires_grad_() for k, v in lg.state_dict().items()
          if k.startswith(f"transformers.{L - 1}.")}
    x = x_in.detach().clone().requires_grad_()
    lin = lambda t, pre: t @ sd[pre + ".weight"].t() + sd[pre + ".bias"]  # noqa: E731

    def ffn(t, msg, pre):
        h = lin(torch.cat([t, msg], -1), pre + "ffn.0")
        h = torch.nn.functional.layer_norm(h, (512,), sd[pre + "ffn.1.weight"], sd[pre + "ffn.1.bias"], 1e-5)
        return t + lin(torch.nn.functional.gelu(h), pre + "ffn.3")

    half = lambda t: torch.stack((-t[..., 1::2], t[..., 0::2]), -1).flatten(-2)  # noqa: E731  rotate_half
    heads = lambda t, cnt: t.reshape(b, cnt, 4, 64).transpose(1, 2)  # noqa: E731
    sides = []
    for rows, cnt in ((slice(0, b * m), m), (slice(b * m, None), n)):  # the self block, per side
        xs = x[rows].reshape(b, cnt, 256)
        c, s = (t[rows].double().reshape(b, 1, cnt, 64) for t in (cos, sin))
        qkv = lin(xs, SELF + "Wqkv").unflatten(-1, (4, -1, 3)).transpose(1, 2)
        q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
        q, k = q * c + half(q) * s, k * c + half(k) * s
        ctx = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).reshape(b, cnt, 256)
        sides.append(ffn(xs, lin(ctx, SELF + "out_proj"), SELF))
    x0, x1 = sides  # the cross block
    q0, q1 = (heads(lin(t, CROSS + "to_qk"), cnt) * 0.125 ** 0.5 for t, cnt in ((x0, m), (x1, n)))
    v0, v1 = heads(lin(x0, CROSS + "to_v"), m), heads(lin(x1, CROSS + "to_v"), n)
    sim = q0 @ q1.transpose(-1, -2)
    m0 = (torch.softmax(sim, -1) @ v1).transpose(1, 2).reshape(b, m, 256)
    m1 = (torch.softmax(sim, -2).transpose(-1, -2) @ v0).transpose(1, 2).reshape(b, n, 256)
    y = torch.cat([ffn(x0, lin(m0, CROSS + "to_out"), CROSS).reshape(-1, 256),
                   ffn(x1, lin(m1, CROSS + "to_out"), CROSS).reshape(-1, 256)], 0)
    (y * dy).sum().backward()
    return {k: v.grad for k, v in sd.items()}, x.grad, y.detach()


@pytest.mark.parametrize("gamma", [0.5, 1.0])
def test_self_block_gradients(fx, gamma):
    name, case, pred = fx
    lg = model(loss={"gamma": gamma})
    before = lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True, cross_attention=True,
                                    descriptor_grads=True)
    grads = lg.layer_loss_backward(pred, labels(case), accumulate=False, descriptor_grads=True, **ALL_ON)
    lean = lg.layer_loss_backward(pred, labels(case), accumulate=False, **ALL_ON)
    torch.cuda.synchronize()
    assert set(grads) == set(before) | {SELF + k for k in TEN} | set(ROWS)
    assert set(lean) == set(grads) - {"grad_ref_descriptors0", "grad_ref_descriptors1"}
    for k in before:  # nothing that was returned before has changed
        assert torch.equal(before[k], grads[k]), k
    for k in lean:    # head L - 2's gradient taken for that layer alone is the same bits
        assert torch.equal(lean[k], grads[k]), k
    b, m, n = shape = (case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1])
    for k in TEN:
        assert grads[SELF + k].shape == lg.get_parameter(SELF + k).shape, k
    assert grads[ROWS[0]].shape == (b, m, 256) and grads[ROWS[3]].shape == (b, n, 256)
    x = flat(pred["ref_descriptors0"][:, L - 2], pred["ref_descriptors1"][:, L - 2])
    ctx = flat(pred["self_block_context0"], pred["self_block_context1"])
    cos, sin = pred["self_block_cos"].double(), pred["self_block_sin"].double()
    dy = flat(grads["grad_cross_block_rows0"], grads["grad_cross_block_rows1"])
    sd = {k: v.detach().double() for k, v in lg.state_dict().items()}
    # ---- the same bits: the FFN part, then the attention with the FFN part's row gradients and their error sums
    p = {key: sd[SELF + nm] for key, nm in (("Wout", "out_proj.weight"), ("bout", "out_proj.bias"), ("W0", "ffn.0.weight"),
                                            ("b0", "ffn.0.bias"), ("gamma", "ffn.1.weight"), ("beta", "ffn.1.bias"),
                                            ("W3", "ffn.3.weight"), ("b3", "ffn.3.bias"))}
    mid = flat(pred["output_stage_rows0"], pred["output_stage_rows1"])
    assert float((osr.forward(x, ctx, p) - mid).abs().max()) < 1e-4 * float(mid.abs().max())  # the kept context is its
    want, sums, erfs = osr.backward(x, ctx, dy, p)
    tol = osr.bounds(sums, erfs, ERF_ABS)
    report = {v: osr.worst_ratio(grads[SELF + k].double().reshape(want[v].shape), want[v], tol[v]) for k, v in STAGE.items()}
    wqkv, bqkv = sbr.to_packed(sd[SELF + "Wqkv.weight"]), sbr.to_packed(sd[SELF + "Wqkv.bias"])
    awant, aerrs = sbr.backward(x, cos, sin, ctx, want["dctx"], want["dx_in"], wqkv, bqkv, *shape,
                                err={"dctx": tol["dctx"] / sbr.U, "dx_in": tol["dx_in"] / sbr.U})
    atol = sbr.bounds(aerrs)
    report["dWqkv"] = sbr.worst_ratio(grads[SELF + "Wqkv.weight"], sbr.to_state_dict(awant["dWqkv"]),
                                      sbr.to_state_dict(atol["dWqkv"]))
    report["dbqkv"] = sbr.worst_ratio(grads[SELF + "Wqkv.bias"], sbr.to_state_dict(awant["dbqkv"]),
                                      sbr.to_state_dict(atol["dbqkv"]))
    dx = flat(grads[ROWS[0]], grads[ROWS[1]])
    report["dx"] = sbr.worst_ratio(dx, awant["dx"], atol["dx"])
    print(f"case {name} gamma {gamma}: fraction of the bound used: " + ", ".join(f"{k} {v:.2e}" for k, v in report.items()))
    assert max(report.values()) <= 1.0, report
    # grad_layer_input_rows = that plus head L - 2's direct gradient, one fp32 addition
    head = flat(grads["grad_ref_descriptors0"][:, L - 2], grads["grad_ref_descriptors1"][:, L - 2])
    total = flat(grads[ROWS[2]], grads[ROWS[3]])
    assert bool(((total - (dx + head)).abs() <= sbr.U * (dx + head).abs()).all()) and float(head.abs().max()) > 0
    # ---- the whole layer by torch's float64 autograd, from the rows of layer L - 2 and head L - 1's direct gradient
    dy_head = flat(grads["grad_ref_descriptors0"][:, L - 1], grads["grad_ref_descriptors1"][:, L - 1])
    ref, ref_dx, y = layer_autograd(lg, x, cos, sin, dy_head, shape)
    last = flat(pred["ref_descriptors0"][:, L - 1], pred["ref_descriptors1"][:, L - 1])
    assert float((y - last).abs().max()) < 1e-4 * float(last.abs().max())  # the layer written here is the device's
    rel = {k: float((grads[k].double() - g).abs().max() / g.abs().max()) for k, g in ref.items()}
    rel["rows"] = float((dx - ref_dx).abs().max() / ref_dx.abs().max())
    assert len(ref) == 22
    print(f"case {name} gamma {gamma}: against float64 autograd of the layer, largest |difference| / max |gradient|: "
          + ", ".join(f"{k.split('.', 2)[2]} {v:.1e}" for k, v in rel.items() if k != "rows") + f", rows {rel['rows']:.1e}")
    assert max(rel.values()) <= TOL_LAYER, rel


def test_self_block_accumulates_and_refuses(fx):
    _, case, pred = fx
    lg = model()
    once = lg.layer_loss_backward(pred, labels(case), accumulate=False, **ALL_ON)
    assert all(q.grad is None for q in lg.parameters())
    lg.layer_loss_backward(pred, labels(case), **ALL_ON)
    lg.layer_loss_backward(pred, labels(case), **ALL_ON)
    for k in TEN:
        q, g = lg.get_parameter(SELF + k), once[SELF + k]
        assert q.grad.shape == q.shape and bool(((q.grad - 2 * g).abs() <= 2.0 ** -22 * g.abs()).all()), k
    named = {k for k in once if not k.startswith("grad_")}
    assert len(named) == 4 * L + 2 * (L - 1) + 22
    assert all(q.grad is None for k, q in lg.named_parameters() if k not in named)
    with pytest.raises(ValueError, match="cross_attention=True"):
        lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True, self_block=True)
    bare = {k: v for k, v in pred.items() if not k.startswith("self_block_")}
    with pytest.raises(ValueError, match="keep_self_block"):
        lg.layer_loss_backward(bare, labels(case), accumulate=False, **ALL_ON)
    with pytest.raises(NotImplementedError, match="fp32 matcher"):
        model(matmul_precision="fp16").layer_loss_backward(pred, labels(case), **ALL_ON)


@pytest.mark.parametrize("where", ["cuda", "cpu", "fp16", "graph", "unfolded"])
def test_sgd_step_and_the_four_updated_calls(where):
    """An SGD step of EPS on the heads, the tokens and the 22 tensors of the last layer, then the four `*_updated()`
    calls: `forward`, `forward_layers` and `forward_pairs` are what a fresh module loaded from `state_dict()` gives, bit
    for bit."""
    from glue_factory_colon_amd import weights

    case = lc.make_case("a", SEED)
    conf = {"weights": "synthetic", "filter_threshold": 0.0}
    if where == "fp16":
        conf["matmul_precision"] = "fp16"
    if where == "graph":
        conf["graph_max_rows"] = 4096
    if where == "unfolded":
        conf["fold_out_proj"] = False
    lg = lightglue.LightGlue(conf).eval()
    if where != "cpu":
        lg = lg.cuda()
    data = inputs(case)
    size = case["size"][:1].cuda()
    items = [{"keypoints0": data["keypoints0"][i:i + 1], "keypoints1": data["keypoints1"][i:i + 1],
              "descriptors0": data["descriptors0"][i:i + 1], "descriptors1": data["descriptors1"][i:i + 1],
              "view0": {"image_size": size}, "view1": {"image_size": size}} for i in range(2)]
    donor = model() if where == "fp16" else lg
    with torch.no_grad():
        plain = lg(data)
        pred = donor.forward_layers(data, keep_output_stage=True, keep_self_block=True)
    grads = donor.layer_loss_backward(pred, labels(case), accumulate=where != "fp16", **ALL_ON)
    grads = {k: g for k, g in grads.items() if not k.startswith("grad_")}
    if where == "fp16":  # gradients are built for the fp32 matcher: they come from an fp32 module of the same weights
        for k, g in grads.items():
            lg.get_parameter(k).grad = g.clone()
    assert len(grads) == 4 * L + 2 * (L - 1) + 22
    frozen = {k: v.detach().clone() for k, v in lg.state_dict().items() if k not in grads}
    # the attention's own gradients are small beside the FFN part's: they get a step of their own size, so that the
    # refresh of the packed Wqkv is seen in the forward
    with torch.no_grad():
        for k in ("Wqkv.weight", "Wqkv.bias"):
            lg.get_parameter(SELF + k).grad *= 100.0
    torch.optim.SGD([q for k, q in lg.named_parameters() if k in grads], lr=EPS).step()
    lg.heads_updated()
    lg.output_stage_updated()
    lg.cross_attention_updated()
    lg.self_block_updated()
    for k, v in frozen.items():
        assert torch.equal(lg.state_dict()[k], v), k
    fresh = lightglue.LightGlue(conf).eval()
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in lg.state_dict().items()})
    if where != "cpu":
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
    # without self_block_updated() the packed self block would be stale: the refresh is what makes these equal.  A module
    # with the cross block and the heads as tuned and the self block as it started gives another layer L - 1.
    stale = lightglue.LightGlue(conf).eval()
    sd = {k: v.detach().cpu().clone() for k, v in lg.state_dict().items()}
    for k in ("Wqkv.weight", "Wqkv.bias"):
        sd[SELF + k] = weights.lightglue_state_dict(0)[SELF + k].clone()
    stale.load_state_dict(sd)
    with torch.no_grad():
        old = (stale.cuda() if where != "cpu" else stale).forward_layers(data)
    assert not torch.equal(old["ref_descriptors0"][:, L - 1], new["ref_descriptors0"][:, L - 1])
    if where != "fp16":
        keep = {"keep_output_stage": True, "keep_self_block": True}
        again = lg.layer_loss_backward(lg.forward_layers(data, **keep), labels(case), accumulate=False, **ALL_ON)
        ref = fresh.layer_loss_backward(fresh.forward_layers(data, **keep), labels(case), accumulate=False, **ALL_ON)
        for k in ref:
            assert torch.equal(again[k], ref[k]), k


def test_finetune_heads_with_the_last_layer(tmp_path, capsys):
    import shutil

    import endopatches_reference as er

    from glue_factory_colon_amd import finetune_heads, weights

    names = er.make_tree(tmp_path, per_sequence=3, hw=(120, 160))
    for n in names:
        shutil.copy(tmp_path / "frames" / "test" / n, tmp_path / "frames" / "val" / n)
    common = ["--data_dir", str(tmp_path / "frames"), "--pair_batch", "4", "--max_num_keypoints", "128", "--num_workers",
              "0", "--optimizer", "sgd", "--lr", "0.01", "--epochs", "2", "--max_steps", "2"]
    out = tmp_path / "tuned.pth"
    before, after = finetune_heads.main(common + ["--params", "last_layer", "--out", str(out)])
    capsys.readouterr()
    print(f"loss/total_deep {before['loss/total_deep']:.6f} -> {after['loss/total_deep']:.6f}")
    assert after["loss/total_deep"] < before["loss/total_deep"]
    tuned = torch.load(str(out), map_location="cpu")
    start = weights.lightglue_state_dict(0)
    moved = {k for k, v in start.items() if k in tuned and not torch.equal(tuned[k], v)}
    assert moved == {k for k in start if k.startswith(f"transformers.{L - 1}.")} and len(moved) == 22
    # the saved state dict reloads to the tuned forward: a fresh pipeline on the file, no step taken, reports every loss
    # the tuner reported after its last step, bit for bit -- the packed self block was refreshed after every step
    again, _ = finetune_heads.main(common[:-2] + ["--matcher_weights", str(out), "--max_steps", "0", "--params", "all",
                                                  "--out", str(tmp_path / "unused.pth")])
    capsys.readouterr()
    for k in (k for k in after if k.startswith(("loss/", "layer/"))):
        assert again[k] == after[k] or (after[k] != after[k] and again[k] != again[k]), k
    both = tmp_path / "both.pth"
    finetune_heads.main(common + ["--params", "all+last_layer", "--out", str(both)])
    moved = {k for k, v in start.items() if not torch.equal(torch.load(str(both), map_location="cpu")[k], v)}
    assert {k for k in start if k.startswith(f"transformers.{L - 1}.")} <= moved
    assert all(k.startswith((f"transformers.{L - 1}.", "log_assignment.", "token_confidence.")) for k in moved)


# ---- the reference's own autograd (tests/golden/self_block_grad_*.npz) and the descent ----------------------------------
import cross_attn_grad_reference as car  # noqa: E402
import head_grad_reference as hg  # noqa: E402
import test_self_block_grad_reference_host as sbh  # noqa: E402  (fixture_ratios, in_state_dict_order)


@pytest.mark.parametrize("gamma", [0.5, 1.0])
def test_self_block_gradients_against_the_references_fixtures(fx, gamma):
    """The ten gradients and `grad_layer_input_rows` against the REFERENCE's float64 autograd (the kept inputs' .grad of
    its last `self_attn`).  The kept tensors come from another evaluation of the trunk (head_grad_reference.trunk_c) and
    dy from another evaluation of the head, the output stage and the cross attention, whose error sums are carried in as
    tests/test_gpu_cross_attn_module.py carries them.  That bound is loose (the carried error of dy exceeds dy); the
    same-bits comparison above is the sharp one.  The fixture's case is the one of `fx` (its input checksum is compared)."""
    name, case, pred = fx
    lg = model(loss={"gamma": gamma})
    grads = lg.layer_loss_backward(pred, labels(case), accumulate=False, descriptor_grads=True, **ALL_ON)
    torch.cuda.synchronize()
    z = np.load(os.path.join(GOLDEN, f"self_block_grad_{name}_gamma{'05' if gamma == 0.5 else '1'}.npz"))
    assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"])) and float(z["gamma"]) == gamma
    b, m, n = shape = (case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1])
    sd = {k: v.detach().double() for k, v in lg.state_dict().items()}
    trunk, head_c = hg.trunk_c(L), hg.head_c(b, m, n)["dx"]
    # the error sum dy = grad_cross_block_rows arrives with: the output stage, then the cross attention
    x_mid = flat(pred["output_stage_rows0"], pred["output_stage_rows1"])
    ctx_c = flat(pred["output_stage_context0"], pred["output_stage_context1"])
    dy_head = flat(grads["grad_ref_descriptors0"][:, L - 1], grads["grad_ref_descriptors1"][:, L - 1])
    _, oe, _ = osr.backward(x_mid, ctx_c, dy_head, osr.stage_params(sd, L - 1), in_err=trunk + head_c)
    dctx = flat(grads["grad_output_stage_context0"], grads["grad_output_stage_context1"])
    dx_in = flat(grads["grad_output_stage_rows0"], grads["grad_output_stage_rows1"])
    _, ce = car.backward(x_mid, ctx_c, dctx, dx_in, car.stage_params(sd, L - 1), *shape,
                         err={"x": trunk * x_mid.abs(), "ctx": trunk * ctx_c.abs(), "dctx": oe["dctx"], "dx_in": oe["dx_in"]})
    x = flat(pred["ref_descriptors0"][:, L - 2], pred["ref_descriptors1"][:, L - 2])
    ctx = flat(pred["self_block_context0"], pred["self_block_context1"])
    dy = flat(grads["grad_cross_block_rows0"], grads["grad_cross_block_rows1"])
    head = flat(grads["grad_ref_descriptors0"][:, L - 2], grads["grad_ref_descriptors1"][:, L - 2])
    p, wqkv, bqkv = sbr.stage_params(sd, L - 1)
    _, tol = sbr.block_backward(x, pred["self_block_cos"].double(), pred["self_block_sin"].double(), ctx, dy, head, p, wqkv,
                                bqkv, *shape, erf_abs=ERF_ABS, in_err=trunk, dy_err=ce["dx"],
                                head_err=(trunk + head_c) * head.abs())
    got = {v: grads[SELF + k].double() for k, v in STAGE.items()}
    got.update(dWqkv=grads[SELF + "Wqkv.weight"].double(), dbqkv=grads[SELF + "Wqkv.bias"].double(),
               layer_input=flat(grads[ROWS[2]], grads[ROWS[3]]))
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    ref = sbh.fixture_ratios(z, "", cpu(got), cpu(sbh.in_state_dict_order(tol)), shape)
    print(f"case {name} gamma {gamma}: against the reference's autograd: " + ", ".join(f"{k} {v:.2e}" for k, v in ref.items()))
    assert max(ref.values()) <= 1.0, ref


@pytest.mark.parametrize("name", ["a", "b"])
def test_descent_matches_the_float64_ratio(name):
    """An SGD step of sbr.DESCENT_EPS on the 22 tensors of the last layer + the three `*_updated()` calls that concern
    them: `total - confidence` falls by the float64 ratio the host test measures and records (sbr.DESCENT_RATIO) times
    eps |grad|^2.  Allowed distance as tests/test_gpu_output_stage.py derives it: 0.005 for what the trunk's float32 error
    does to the gradient and the curvature, plus 32 roundings of 2^-23 of the loss value against the size of the
    difference."""
    seed = int(np.load(os.path.join(GOLDEN, f"self_block_grad_{name}_gamma1.npz"))["seed"])
    case = lc.make_case(name, seed)
    lg = model(loss={"gamma": 1.0})
    data, eps = inputs(case), sbr.DESCENT_EPS
    smooth = lambda losses: float((losses["total"].double() - losses["confidence"].double()).mean())  # noqa: E731
    with torch.no_grad():
        pred = lg.forward_layers(data, keep_output_stage=True, keep_self_block=True)
        before = smooth(lg.layer_loss(pred, labels(case))[0])
    grads = lg.layer_loss_backward(pred, labels(case), accumulate=False, **ALL_ON)
    layer = {k: g for k, g in grads.items() if k.startswith(f"transformers.{L - 1}.")}
    assert len(layer) == 22
    with torch.no_grad():
        for k, g in layer.items():
            lg.get_parameter(k).sub_(eps * g)
    lg.output_stage_updated()
    lg.cross_attention_updated()
    lg.self_block_updated()
    with torch.no_grad():
        after = smooth(lg.layer_loss(lg.forward_layers(data), labels(case))[0])
    sq = sum(float((g.double() ** 2).sum()) for g in layer.values())
    ratio = (after - before) / (-eps * sq)
    allowed = 0.005 + 32 * sbr.U * abs(before) / (eps * sq)
    print(f"case {name}: descent ratio {ratio:.4f} (float64: {sbr.DESCENT_RATIO[name]:.4f}, allowed distance "
          f"{allowed:.4f}): {before:.6f} -> {after:.6f}, |grad|^2 {sq:.4e}")
    assert abs(ratio - sbr.DESCENT_RATIO[name]) <= allowed
