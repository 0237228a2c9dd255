"""Time the last layer's output-stage gradients against float32 torch autograd of the same stage and loss, and record how
much of their per-element bounds they use.

    python tools/output_stage_bench.py --out profiles  ->  profiles/output_stage_bench.json, output_stage_parity.json

Per shape (B = 32 x 1024 + 1024 and B = 8 x 2048 + 2048 key points, name-seeded weights, unit descriptors), alternating
in one process on the same GPU, medians of device-event timings in ms per batch:
  backward         LightGlue.layer_loss_backward(accumulate=False)        backward_stage   the same with output_stage
  torch_stage      the same output stage, last head and loss as float32 torch operations with autograd on the same GPU:
                   to_out, the concatenation, ffn, the residual, the head of layer L - 1 and its nll, from the kept rows
                   and context (autograd has to run the forward it differentiates), over torch_head, the last head alone
  kernel           gfc_lg_ffn_backward alone (with dx_in and dctx): the TFLOP/s of its matrix part -- m, h, da, dW3, dW0,
                   dcat, dWout, dctx: 2 R (3 * 256 * 256 + 3 * 512 * 512 + 2 * 256 * 512) flop -- against the 157 TF peak
                   of the fp32 matrix instructions
The yardstick of the stage is torch_stage - torch_head against backward_stage - backward: what the stage adds to each.

output_stage_parity.json: the largest fraction of its bound (tests/output_stage_reference.py) that any element of each
output uses, for the kernel alone (random rows at every row count of the kernel test, with and without Wout, and the two
exact-integer conditioning cases) and for the module on the two fixture batches (against the closed form on the device's
own kept tensors).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from head_backward_bench import PEAK_TF, alternate, torch_head, torch_nll  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402

NAMES = {"to_out.weight": "dWout", "to_out.bias": "dbout", "ffn.0.weight": "dW0", "ffn.0.bias": "db0",
         "ffn.1.weight": "dgamma", "ffn.1.bias": "dbeta", "ffn.3.weight": "dW3", "ffn.3.bias": "db3"}


def torch_stage(lg, pred, weights, w_last, with_stage):
    """.grad of the last head (and, with_stage, of the eight tensors of the output stage) from autograd."""
    nl = lg.conf.n_layers
    ca = lg.transformers[nl - 1].cross_attn
    if with_stage:
        xs = []
        for s in "01":
            x, ctx = pred["output_stage_rows" + s], pred["output_stage_context" + s]
            xs.append(x + ca.ffn(torch.cat([x, ca.to_out(ctx)], -1)))
    else:
        xs = [pred["ref_descriptors0"][:, nl - 1], pred["ref_descriptors1"][:, nl - 1]]
    la = torch_head(xs[0], xs[1], lg.log_assignment[nl - 1])
    torch.mean(torch_nll(la, weights) * w_last).backward()


def bench_shape(b, m, n, rounds, iters):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(b + m)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)  # noqa: E731
    size = torch.tensor([[640.0, 480.0]]).expand(b, 2).to(dev)
    data = {"keypoints0": (torch.rand((b, m, 2), generator=g) * 479).to(dev),
            "keypoints1": (torch.rand((b, n, 2), generator=g) * 479).to(dev),
            "descriptors0": unit(torch.randn((b, m, 256), generator=g)).to(dev),
            "descriptors1": unit(torch.randn((b, n, 256), generator=g)).to(dev),
            "view0": {"image_size": size}, "view1": {"image_size": size}}
    gt0 = torch.randint(-2, n, (b, m), generator=g).to(dev)
    gt1 = torch.randint(-2, m, (b, n), generator=g).to(dev)
    labels = {"gt_matches0": gt0, "gt_matches1": gt1}
    lg = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.1}).eval().to(dev)
    nl = lg.conf.n_layers
    pre = f"transformers.{nl - 1}.cross_attn."
    with torch.no_grad():
        pred = lg.forward_layers(data, keep_output_stage=True)
    weights = torch.zeros((b, m + 1, n + 1), device=dev)
    bi, ii = torch.nonzero(gt0 > -1, as_tuple=True)
    weights[bi, ii, gt0[bi, ii]] = 1.0
    weights[:, :m, -1] = (gt0 == -1).float()
    weights[:, -1, :n] = (gt1 == -1).float()
    w_last = 1.0 / nl  # loss.gamma 1.0

    def ours(stage):
        return lg.layer_loss_backward(pred, labels, accumulate=False, output_stage=stage)

    def torch_form(stage):
        for p in lg.parameters():
            p.grad = None
        torch_stage(lg, pred, weights, w_last, stage)

    mine = ours(True)
    torch_form(True)
    worst = 0.0
    for k in NAMES:
        ref = lg.get_parameter(pre + k).grad
        worst = max(worst, float((mine[pre + k] - ref).abs().max() / ref.abs().max().clamp(min=1e-30)))
    out = {"B": b, "M": m, "N": n, "max_difference_over_max_abs": worst}
    del mine
    out.update(alternate({"backward": lambda: ours(False), "backward_stage": lambda: ours(True),
                          "torch_head": lambda: torch_form(False), "torch_stage": lambda: torch_form(True)}, rounds, iters))
    med = out["median_ms"]
    out["stage_ms"] = med["backward_stage"] - med["backward"]
    out["torch_stage_ms"] = med["torch_stage"] - med["torch_head"]
    out["torch_over_ours_stage_only"] = out["torch_stage_ms"] / out["stage_ms"]
    # the kernel alone
    rows = b * (m + n)
    w = lg._output_stage_weights(dev)
    flat = lambda k: torch.cat([pred[k + "0"].reshape(-1, 256), pred[k + "1"].reshape(-1, 256)], 0).contiguous()  # noqa: E731
    x, ctx = flat("output_stage_rows"), flat("output_stage_context")
    dy = torch.randn((rows, 256), device=dev) * 1e-3
    o = {k: torch.empty_like(w[k]) for k in NAMES}
    dx, dc = torch.empty((rows, 256), device=dev), torch.empty((rows, 256), device=dev)
    ws = torch.empty(nat.call("gfc_lg_ffn_backward_workspace_bytes", rows), dtype=torch.uint8, device=dev)

    def kernel():
        nat.call("gfc_lg_ffn_backward", x, ctx, dy, w["to_out.weight"], w["to_out.bias"], w["ffn.0.weight"], w["ffn.0.bias"],
                 w["ffn.1.weight"], w["ffn.1.bias"], w["ffn.3.weight"], rows, o["to_out.weight"], o["to_out.bias"],
                 o["ffn.0.weight"], o["ffn.0.bias"], o["ffn.1.weight"], o["ffn.1.bias"], o["ffn.3.weight"], o["ffn.3.bias"],
                 dx, dc, ws, ws.numel())

    k = alternate({"kernel": kernel}, rounds, iters)
    flop = 2.0 * rows * (3 * 256 * 256 + 3 * 512 * 512 + 2 * 256 * 512)
    tf = flop / (k["median_ms"]["kernel"] * 1e-3) / 1e12
    out["kernel"] = {"median_ms": k["median_ms"]["kernel"], "matrix_flop": flop, "tflops": tf,
                     "fraction_of_fp32_matrix_peak": tf / PEAK_TF, "workspace_bytes": ws.numel()}
    return out


PARITY_ROWS = (1, 2, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2049, 128 * 1024 + 17)


def run_kernel(x, ctx, dy, p):
    """{output: tensor} of one gfc_lg_ffn_backward call on device tensors (p keyed as output_stage_reference keys it)."""
    dev, rows = x.device, x.shape[0]
    e = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    out = {"dW0": e(512, 512), "db0": e(512), "dgamma": e(512), "dbeta": e(512), "dW3": e(256, 512), "db3": e(256),
           "dx_in": e(rows, 256), "dctx": e(rows, 256)}
    if p["Wout"] is not None:
        out["dWout"], out["dbout"] = e(256, 256), e(256)
    ws = torch.empty(nat.call("gfc_lg_ffn_backward_workspace_bytes", rows), dtype=torch.uint8, device=dev)
    nat.call("gfc_lg_ffn_backward", x, ctx, dy, p["Wout"], p["bout"], p["W0"], p["b0"], p["gamma"], p["beta"], p["W3"], rows,
             out.get("dWout"), out.get("dbout"), out["dW0"], out["db0"], out["dgamma"], out["dbeta"], out["dW3"], out["db3"],
             out["dx_in"], out["dctx"], ws, ws.numel())
    return out


def parity():
    import numpy as np

    import layer_loss_cases as lc
    import output_stage_reference as osr

    dev = torch.device("cuda")
    kernel, module = {}, {}
    to = lambda p, dtype: {k: None if v is None else v.to(device=dev, dtype=dtype).contiguous()  # noqa: E731
                           for k, v in p.items()}

    def kernel_case(x, ctx, dy, p, exact_h):
        x, ctx, dy = x.to(dev), ctx.to(dev), dy.to(dev)
        got = run_kernel(x, ctx, dy, to(p, torch.float32))
        want, errs, erfs = osr.backward(x.double(), ctx.double(), dy.double(), to(p, torch.float64), exact_h=exact_h)
        tol = osr.bounds(errs, erfs)
        for k in want:
            kernel[k] = max(kernel.get(k, 0.0), osr.worst_ratio(got[k].double().reshape(want[k].shape), want[k], tol[k]))

    for rows in PARITY_ROWS:
        for with_out in (True, False):
            g = torch.Generator().manual_seed(100 + rows)
            x, ctx = torch.randn((rows, 256), generator=g) / 16, torch.randn((rows, 256), generator=g) / 16
            dy = torch.randn((rows, 256), generator=g) * 1e-3
            kernel_case(x, ctx, dy, osr.random_params(torch.Generator().manual_seed(7 + with_out), with_out), False)
    for offset in (4096, 0):
        kernel_case(*osr.conditioning_case(offset), True)
    nl = lc.N_LAYERS
    pre = f"transformers.{nl - 1}.cross_attn."
    for name in ("a", "b"):
        seed = int(np.load(os.path.join(ROOT, "tests", "golden", f"output_stage_{name}_gamma1.npz"))["seed"])
        case = lc.make_case(name, seed)
        c = lambda k: case[k].to(dev)  # noqa: E731
        data = {"keypoints0": c("keypoints0"), "keypoints1": c("keypoints1"), "descriptors0": c("descriptors0"),
                "descriptors1": c("descriptors1"), "view0": {"image_size": c("size")}, "view1": {"image_size": c("size")}}
        labels = {"gt_matches0": c("gt_matches0"), "gt_matches1": c("gt_matches1")}
        if case["gt_assignment"] is not None:
            labels["gt_assignment"] = c("gt_assignment")
        for gamma in (0.5, 1.0):
            lg = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.0, "loss": {"gamma": gamma}}).eval().to(dev)
            with torch.no_grad():
                pred = lg.forward_layers(data, keep_output_stage=True)
            grads = lg.layer_loss_backward(pred, labels, descriptor_grads=True, accumulate=False, output_stage=True)
            flat = lambda a, b: torch.cat([a.reshape(-1, 256), b.reshape(-1, 256)], 0).double()  # noqa: E731
            sd = lg.state_dict()
            p = {"Wout": sd[pre + "to_out.weight"], "bout": sd[pre + "to_out.bias"], "W0": sd[pre + "ffn.0.weight"],
                 "b0": sd[pre + "ffn.0.bias"], "gamma": sd[pre + "ffn.1.weight"], "beta": sd[pre + "ffn.1.bias"],
                 "W3": sd[pre + "ffn.3.weight"], "b3": sd[pre + "ffn.3.bias"]}
            want, errs, erfs = osr.backward(
                flat(pred["output_stage_rows0"], pred["output_stage_rows1"]),
                flat(pred["output_stage_context0"], pred["output_stage_context1"]),
                flat(grads["grad_ref_descriptors0"][:, nl - 1], grads["grad_ref_descriptors1"][:, nl - 1]),
                {k: v.detach().double() for k, v in p.items()})
            tol = osr.bounds(errs, erfs)
            got = {v: grads[pre + k] for k, v in NAMES.items()}
            got["dx_in"] = flat(grads["grad_output_stage_rows0"], grads["grad_output_stage_rows1"])
            got["dctx"] = flat(grads["grad_output_stage_context0"], grads["grad_output_stage_context1"])
            for k in want:
                module[k] = max(module.get(k, 0.0),
                                osr.worst_ratio(got[k].double().reshape(want[k].shape), want[k], tol[k]))
    return {"kernel": kernel, "module": module}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("output_stage_bench needs the GPU: nothing is measured without one")
    os.makedirs(args.out, exist_ok=True)
    par = {"what": "largest fraction of the per-element bound (tests/output_stage_reference.py) used, per output",
           "device": torch.cuda.get_device_name(0), "worst_fraction": parity()}
    with open(os.path.join(args.out, "output_stage_parity.json"), "w") as f:
        json.dump(par, f, indent=1)
    print(json.dumps(par, indent=1), flush=True)
    res = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "iters_per_timing": args.iters, "fp32_matrix_peak_tflops": PEAK_TF, "shapes": {}}
    for key, shape in (("b32_1024", (32, 1024, 1024)), ("b8_2048", (8, 2048, 2048))):
        res["shapes"][key] = bench_shape(*shape, args.rounds, args.iters)
        print(key, json.dumps(res["shapes"][key], indent=1), flush=True)
    path = os.path.join(args.out, "output_stage_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
