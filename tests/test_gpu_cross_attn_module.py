"""The last cross block's attention backward through the module on the GPU:
`layer_loss_backward(output_stage=True, cross_attention=True)`, `cross_attention_updated()` and
`finetune_heads --params cross_block`.

The four gradients and the complete gradient at the block's input rows are compared with the float64 closed form of
tests/cross_attn_grad_reference.py on the device's own kept tensors and its own output-stage row gradients (the same
bits), per element within 2^-23 times the error sum, and with the reference's autograd (tests/golden/cross_attn_grad_*)
with the trunk's and the output stage's float32 error added.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_attn_grad_reference as car  # noqa: E402
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402
import output_stage_reference as osr  # noqa: E402

from glue_factory_colon_amd import lightglue  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 0.05  # the SGD step of the refresh test, as tests/test_gpu_output_stage.py takes it
L = lc.N_LAYERS
PRE = f"transformers.{L - 1}.cross_attn."
NAMES = {"to_qk.weight": "dWqk", "to_qk.bias": "dbqk", "to_v.weight": "dWv", "to_v.bias": "dbv"}
STAGE = ("to_out.weight", "to_out.bias", "ffn.0.weight", "ffn.0.bias", "ffn.1.weight", "ffn.1.bias", "ffn.3.weight",
         "ffn.3.bias")
ROWS = ("grad_cross_block_rows0", "grad_cross_block_rows1")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = int(np.load(os.path.join(GOLDEN, "layer_loss.npz"))["seed"])


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


@pytest.fixture(scope="module", params=["a", "b"])
def fx(request):
    """A case of tests/layer_loss_cases.py and ONE kept prediction shared by the tests (never changed)."""
    seed = int(np.load(os.path.join(GOLDEN, f"cross_attn_grad_{request.param}_gamma1.npz"))["seed"])
    case = lc.make_case(request.param, seed)
    lg = model()
    with torch.no_grad():
        pred = lg.forward_layers(inputs(case), keep_output_stage=True)
    torch.cuda.synchronize()
    return request.param, case, pred


@pytest.mark.parametrize("gamma", [0.5, 1.0])
def test_cross_attention_gradients_against_the_closed_form(fx, gamma):
    name, case, pred = fx
    lg = model(loss={"gamma": gamma})
    stage = lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True)
    grads = lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True, cross_attention=True)
    torch.cuda.synchronize()
    assert set(grads) == set(stage) | {PRE + k for k in NAMES} | set(ROWS)
    for k in stage:  # nothing that was returned before has changed
        assert torch.equal(stage[k], grads[k]), k
    b, m, n = shape = (case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1])
    for k in NAMES:
        assert grads[PRE + k].shape == lg.get_parameter(PRE + k).shape, k
    assert grads[ROWS[0]].shape == (b, m, 256) and grads[ROWS[1]].shape == (b, n, 256)
    x = flat(pred["output_stage_rows0"], pred["output_stage_rows1"])
    ctx = flat(pred["output_stage_context0"], pred["output_stage_context1"])
    dctx = flat(grads["grad_output_stage_context0"], grads["grad_output_stage_context1"])
    dx_in = flat(grads["grad_output_stage_rows0"], grads["grad_output_stage_rows1"])
    pc = {k: v.detach().double() for k, v in car.stage_params(lg.state_dict(), L - 1).items()}
    # the kept context is this attention's: the closed form's forward on the kept rows gives it, to fp32 rounding
    mine = car.attention_forward(x @ pc["Wqk"].t() + pc["bqk"], x @ pc["Wv"].t() + pc["bv"], *shape)
    assert float((mine - ctx).abs().max()) < 1e-4 * float(ctx.abs().max())
    want, errs = car.backward(x, ctx, dctx, dx_in, pc, *shape)
    tol = car.bounds(errs)
    got = {v: grads[PRE + k].double() for k, v in NAMES.items()}
    got["dx"] = flat(grads[ROWS[0]], grads[ROWS[1]])
    got["dx_att"] = got["dx"] - dx_in  # (dx = fl(dx_in + att): the rounding of that sum is inside the bound of dx)
    report = {k: car.worst_ratio(got[k], want[k], tol["dx" if k == "dx_att" else k]) for k in want}
    print(f"case {name} gamma {gamma}: fraction of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))
    assert max(report.values()) <= 1.0, report
    # the reference's own autograd (float64 run): the kept tensors come from another evaluation of the trunk
    # (head_grad_reference.trunk_c), dctx and dx_in from another evaluation of the head and the output stage
    z = np.load(os.path.join(GOLDEN, f"cross_attn_grad_{name}_gamma{'05' if gamma == 0.5 else '1'}.npz"))
    assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"])) and float(z["gamma"]) == gamma
    trunk = hg.trunk_c(L)
    dy = flat(*stage_dy(lg, pred, case))
    p_os = {k: v.detach().double() for k, v in osr.stage_params(lg.state_dict(), L - 1).items()}
    _, oe, _ = osr.backward(x, ctx, dy, p_os, in_err=trunk + hg.head_c(b, m, n)["dx"])
    _, errs_in = car.backward(x, ctx, dctx, dx_in, pc, *shape,
                              err={"x": trunk * x.abs(), "ctx": trunk * ctx.abs(), "dctx": oe["dctx"], "dx_in": oe["dx_in"]})
    tol = car.bounds(errs_in)
    t = lambda k: torch.from_numpy(z[k]).double().to(DEV)  # noqa: E731
    ref = {"dbqk": car.worst_ratio(got["dbqk"], t("bqk"), tol["dbqk"]),
           "dbv": car.worst_ratio(got["dbv"], t("bv"), tol["dbv"])}
    for key, out in (("wqk", "dWqk"), ("wv", "dWv")):
        rows_, cols = torch.from_numpy(z[key + "_pick_rows"]).to(DEV), torch.from_numpy(z[key + "_pick_cols"]).to(DEV)
        u, v = t(key + "_u"), t(key + "_v")
        g = got[out]
        ref[out] = max(car.worst_ratio(g[rows_], t(key + "_rows"), tol[out][rows_]),
                       car.worst_ratio(g[:, cols], t(key + "_cols"), tol[out][:, cols]),
                       float((u @ g @ v - float(z[key + "_bilinear"])).abs() / (u.abs() @ tol[out] @ v.abs())))
    r0, r1 = torch.from_numpy(z["rows0"]).to(DEV), torch.from_numpy(z["rows1"]).to(DEV) + b * m
    ref["dx"] = max(car.worst_ratio(got["dx"][r0], t("dx0"), tol["dx"][r0]),
                    car.worst_ratio(got["dx"][r1], t("dx1"), tol["dx"][r1]))
    print(f"case {name} gamma {gamma}: against the reference's autograd: " + ", ".join(f"{k} {v:.2e}" for k, v in ref.items()))
    assert max(ref.values()) <= 1.0, ref


def stage_dy(lg, pred, case):
    """Head L - 1's direct gradient at the last layer's descriptors, per side."""
    g = lg.layer_loss_backward(pred, labels(case), descriptor_grads=True, accumulate=False)
    return g["grad_ref_descriptors0"][:, L - 1], g["grad_ref_descriptors1"][:, L - 1]


def test_cross_attention_accumulates_and_refuses(fx):
    _, case, pred = fx
    lg = model()
    once = lg.layer_loss_backward(pred, labels(case), accumulate=False, output_stage=True, cross_attention=True)
    assert all(q.grad is None for q in lg.parameters())
    lg.layer_loss_backward(pred, labels(case), output_stage=True, cross_attention=True)
    lg.layer_loss_backward(pred, labels(case), output_stage=True, cross_attention=True)
    for k in NAMES:
        q, g = lg.get_parameter(PRE + k), once[PRE + k]
        assert q.grad.shape == q.shape and bool(((q.grad - 2 * g).abs() <= 2.0 ** -22 * g.abs()).all()), k
    named = {k for k in once if not k.startswith("grad_")}
    assert len(named) == 4 * L + 2 * (L - 1) + 12
    assert all(q.grad is None for k, q in lg.named_parameters() if k not in named)
    with pytest.raises(ValueError, match="output_stage=True"):
        lg.layer_loss_backward(pred, labels(case), accumulate=False, cross_attention=True)
    bare = {k: v for k, v in pred.items() if not k.startswith("output_stage_")}
    with pytest.raises(ValueError, match="keep_output_stage"):
        lg.layer_loss_backward(bare, labels(case), accumulate=False, output_stage=True, cross_attention=True)
    with pytest.raises(NotImplementedError, match="fp32 matcher"):
        model(matmul_precision="fp16").layer_loss_backward(pred, labels(case), output_stage=True, cross_attention=True)


@pytest.mark.parametrize("where", ["cuda", "cpu", "fp16", "graph", "unfolded"])
def test_sgd_step_cross_attention_updated_and_descent(where):
    """An SGD step of EPS on the heads, the tokens and the twelve tensors of the last cross block, then the three
    `*_updated()` calls: `forward`, `forward_layers` and `forward_pairs` are what a fresh module loaded from
    `state_dict()` gives, bit for bit (the descent has a test of its own below)."""
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
        pred = donor.forward_layers(data, keep_output_stage=True)
    grads = donor.layer_loss_backward(pred, labels(case), output_stage=True, cross_attention=True,
                                      accumulate=where != "fp16")
    grads = {k: g for k, g in grads.items() if not k.startswith("grad_")}
    if where == "fp16":  # gradients are built for the fp32 matcher: they come from an fp32 module of the same weights
        for k, g in grads.items():
            lg.get_parameter(k).grad = g.clone()
    assert len(grads) == 4 * L + 2 * (L - 1) + 12
    frozen = {k: v.detach().clone() for k, v in lg.state_dict().items() if k not in grads}
    # the attention's own gradients are small beside the output stage's: they get a step of their own size, so that the
    # refresh of the packed [to_qk; to_v] is seen in the forward
    with torch.no_grad():
        for k in NAMES:
            lg.get_parameter(PRE + k).grad *= 100.0
    opt = torch.optim.SGD([q for k, q in lg.named_parameters() if k in grads], lr=EPS)
    opt.step()
    lg.heads_updated()
    lg.output_stage_updated()
    lg.cross_attention_updated()
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
    # without cross_attention_updated() the packed [to_qk; to_v] would be stale: the refresh is what makes these equal
    stale = lightglue.LightGlue(conf).eval()
    sd = {k: v.detach().cpu().clone() for k, v in lg.state_dict().items()}
    for k in NAMES:
        sd[PRE + k] = frozen_or_start(k)
    stale.load_state_dict(sd)
    with torch.no_grad():
        old = (stale.cuda() if where != "cpu" else stale).forward_layers(data)
    assert not torch.equal(old["ref_descriptors0"][:, L - 1], new["ref_descriptors0"][:, L - 1])
    if where != "fp16":
        again = lg.layer_loss_backward(lg.forward_layers(data, keep_output_stage=True), labels(case), accumulate=False,
                                       output_stage=True, cross_attention=True)
        ref = fresh.layer_loss_backward(fresh.forward_layers(data, keep_output_stage=True), labels(case),
                                        accumulate=False, output_stage=True, cross_attention=True)
        for k in ref:
            assert torch.equal(again[k], ref[k]), k


def frozen_or_start(k):
    from glue_factory_colon_amd import weights

    return weights.lightglue_state_dict(0)[PRE + k].clone()


@pytest.mark.parametrize("name", ["a", "b"])
def test_descent_matches_the_float64_ratio(name):
    """An SGD step of car.DESCENT_EPS on the twelve tensors alone + `output_stage_updated()` +
    `cross_attention_updated()`: `total - confidence` falls by the float64 ratio the host test measures and records
    (car.DESCENT_RATIO) times eps |grad|^2.  Allowed distance as tests/test_gpu_output_stage.py derives it: 0.005 for
    what the trunk's float32 error does to the gradient and the curvature, plus 32 roundings of 2^-23 of the loss value
    against the size of the difference."""
    seed = int(np.load(os.path.join(GOLDEN, f"cross_attn_grad_{name}_gamma1.npz"))["seed"])
    case = lc.make_case(name, seed)
    lg = model(loss={"gamma": 1.0})
    data, eps = inputs(case), car.DESCENT_EPS
    smooth = lambda losses: float((losses["total"].double() - losses["confidence"].double()).mean())  # noqa: E731
    with torch.no_grad():
        pred = lg.forward_layers(data, keep_output_stage=True)
        before = smooth(lg.layer_loss(pred, labels(case))[0])
    grads = lg.layer_loss_backward(pred, labels(case), output_stage=True, cross_attention=True, accumulate=False)
    twelve = {PRE + k: grads[PRE + k] for k in STAGE + tuple(NAMES)}
    with torch.no_grad():
        for k, g in twelve.items():
            lg.get_parameter(k).sub_(eps * g)
    lg.output_stage_updated()
    lg.cross_attention_updated()
    with torch.no_grad():
        after = smooth(lg.layer_loss(lg.forward_layers(data), labels(case))[0])
    sq = sum(float((g.double() ** 2).sum()) for g in twelve.values())
    ratio = (after - before) / (-eps * sq)
    allowed = 0.005 + 32 * car.U * abs(before) / (eps * sq)
    print(f"case {name}: descent ratio {ratio:.4f} (float64: {car.DESCENT_RATIO[name]:.4f}, allowed distance "
          f"{allowed:.4f}): {before:.6f} -> {after:.6f}, |grad|^2 {sq:.4e}")
    assert abs(ratio - car.DESCENT_RATIO[name]) <= allowed


def test_finetune_heads_with_the_cross_block(tmp_path, capsys):
    import shutil

    import endopatches_reference as er

    from glue_factory_colon_amd import finetune_heads, weights

    names = er.make_tree(tmp_path, per_sequence=3, hw=(120, 160))
    for n in names:
        shutil.copy(tmp_path / "frames" / "test" / n, tmp_path / "frames" / "val" / n)
    common = ["--data_dir", str(tmp_path / "frames"), "--pair_batch", "4", "--max_num_keypoints", "128", "--num_workers",
              "0", "--optimizer", "sgd", "--lr", "0.01", "--epochs", "2", "--max_steps", "2"]
    out = tmp_path / "tuned.pth"
    before, after = finetune_heads.main(common + ["--params", "cross_block", "--out", str(out)])
    capsys.readouterr()
    print(f"loss/total_deep {before['loss/total_deep']:.6f} -> {after['loss/total_deep']:.6f}")
    assert after["loss/total_deep"] < before["loss/total_deep"]
    tuned = torch.load(str(out), map_location="cpu")
    start = weights.lightglue_state_dict(0)
    moved = {k for k, v in start.items() if k in tuned and not torch.equal(tuned[k], v)}
    assert moved == {PRE + k for k in STAGE + tuple(NAMES)}
    # the saved state dict reloads to the tuned forward: a fresh pipeline on the file, no step taken, reports every loss
    # the tuner reported after its last step, bit for bit -- the packed [to_qk; to_v] was refreshed after every step
    again, _ = finetune_heads.main(common[:-2] + ["--matcher_weights", str(out), "--max_steps", "0", "--params", "all",
                                                  "--out", str(tmp_path / "unused.pth")])
    capsys.readouterr()
    for k in (k for k in after if k.startswith(("loss/", "layer/"))):
        assert again[k] == after[k] or (after[k] != after[k] and again[k] != again[k]), k
    both = tmp_path / "both.pth"
    finetune_heads.main(common + ["--params", "all+cross_block", "--out", str(both)])
    moved = {k for k, v in start.items() if not torch.equal(torch.load(str(both), map_location="cpu")[k], v)}
    assert {PRE + k for k in STAGE + tuple(NAMES)} <= moved
    assert all(k.startswith((PRE, "log_assignment.", "token_confidence.")) for k in moved)
