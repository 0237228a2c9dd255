"""Time the last cross block's attention backward against float32 torch autograd of the same stage.

    python tools/cross_attn_backward_bench.py --out profiles  ->  profiles/cross_attn_backward_bench.json

Per shape (B = 32 x 1024 + 1024 and B = 8 x 2048 + 2048 key points, name-seeded weights, unit descriptors), alternating
in one process on the same GPU, medians of device-event timings in ms per batch:
  core             gfc_attention_cross_backward alone on the block's own qk and v: TFLOP/s at 10 * 2 * 64 flop per score
                   element, head and pair (both directions) against the 157 TF peak of the fp32 matrix instructions
  block            gfc_lg_cross_attn_backward (to_qk, to_v, the core, the four reductions, dx)
  backward_stage   LightGlue.layer_loss_backward(accumulate=False, output_stage=True): the parent's call
  backward_cross   the same with cross_attention=True
  torch_cross      to_qk, to_v and the attention as float32 torch operations from the kept rows, and autograd of
                   sum(ctx * dctx) + sum(x * dx_in) for the four tensors and the rows (autograd has to run the forward it
                   differentiates; it stores the [B,4,M,N] matrices)
The yardsticks are torch_cross against backward_cross - backward_stage (what the attention adds), and backward_cross over
backward_stage (what a caller of the parent's call pays for the four more gradients).
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

from head_backward_bench import PEAK_TF, alternate  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402

NAMES = ("to_qk.weight", "to_qk.bias", "to_v.weight", "to_v.bias")


def torch_cross(ca, x0, x1, dctx0, dctx1, dx0, dx1):
    """.grad of to_qk / to_v and of the rows, from autograd on the reference's own formulation (lightglue.py:196-218)."""
    x0, x1 = x0.detach().requires_grad_(), x1.detach().requires_grad_()
    split = lambda t: t.unflatten(-1, (4, -1)).transpose(1, 2)  # noqa: E731
    qk0, qk1, v0, v1 = split(ca.to_qk(x0)), split(ca.to_qk(x1)), split(ca.to_v(x0)), split(ca.to_v(x1))
    qk0, qk1 = qk0 * 64 ** -0.25, qk1 * 64 ** -0.25
    sim = torch.einsum("bhid, bhjd -> bhij", qk0, qk1)
    attn01 = torch.softmax(sim, -1)
    attn10 = torch.softmax(sim.transpose(-2, -1).contiguous(), -1)
    m0 = torch.einsum("bhij, bhjd -> bhid", attn01, v1).transpose(1, 2).flatten(start_dim=-2)
    m1 = torch.einsum("bhji, bhjd -> bhid", attn10.transpose(-2, -1), v0).transpose(1, 2).flatten(start_dim=-2)
    ((m0 * dctx0).sum() + (m1 * dctx1).sum() + (x0 * dx0).sum() + (x1 * dx1).sum()).backward()
    return x0.grad, x1.grad


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
    labels = {"gt_matches0": torch.randint(-2, n, (b, m), generator=g).to(dev),
              "gt_matches1": torch.randint(-2, m, (b, n), generator=g).to(dev)}
    lg = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.1}).eval().to(dev)
    nl = lg.conf.n_layers
    pre = f"transformers.{nl - 1}.cross_attn."
    ca = lg.transformers[nl - 1].cross_attn
    with torch.no_grad():
        pred = lg.forward_layers(data, keep_output_stage=True)

    def ours(cross):
        return lg.layer_loss_backward(pred, labels, accumulate=False, output_stage=True, cross_attention=cross)

    mine = ours(True)
    x0, x1 = pred["output_stage_rows0"], pred["output_stage_rows1"]
    dc0, dc1 = mine["grad_output_stage_context0"], mine["grad_output_stage_context1"]
    di0, di1 = mine["grad_output_stage_rows0"], mine["grad_output_stage_rows1"]

    def torch_form():
        for p in lg.parameters():
            p.grad = None
        return torch_cross(ca, x0, x1, dc0, dc1, di0, di1)

    gx0, gx1 = torch_form()
    rel = lambda a, ref: float((a - ref).abs().max() / ref.abs().max().clamp(min=1e-30))  # noqa: E731
    out = {"B": b, "M": m, "N": n,
           "max_difference_over_max_abs": {**{k: rel(mine[pre + k], ca.get_parameter(k).grad) for k in NAMES},
                                           "grad_cross_block_rows": max(rel(mine["grad_cross_block_rows0"], gx0),
                                                                        rel(mine["grad_cross_block_rows1"], gx1))}}
    rows = b * (m + n)
    flat = lambda a, c: torch.cat([a.reshape(-1, 256), c.reshape(-1, 256)], 0).contiguous()  # noqa: E731
    x, ctx = flat(x0, x1), flat(pred["output_stage_context0"], pred["output_stage_context1"])
    dctx, dx_in = flat(dc0, dc1), flat(di0, di1)
    del mine, gx0, gx1
    w = lg._cross_attention_weights(dev)
    qk, v = torch.empty_like(x), torch.empty_like(x)
    for wt, bias, y in ((w["to_qk.weight"], w["to_qk.bias"], qk), (w["to_v.weight"], w["to_v.bias"], v)):
        nat.call("gfc_linear", x, 256, 256, None, 0, 0, wt, 256, bias, None, None, 1.0, None, None, None, 0, y, 256, rows,
                 256)
    dqk, dv, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    o = {k: torch.empty_like(w[k]) for k in NAMES}
    ws = torch.empty(nat.call("gfc_lg_cross_attn_backward_workspace_bytes", b, m, n), dtype=torch.uint8, device=dev)
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream

    def core():
        nat.check(lib.gfc_attention_cross_backward(qk.data_ptr(), 256, v.data_ptr(), 256, ctx.data_ptr(), 256,
                                                   dctx.data_ptr(), 256, b, m, n, 4, 0.125, dqk.data_ptr(), 256,
                                                   dv.data_ptr(), 256, ws.data_ptr(), ws.numel(), stream), "core")

    def block():
        nat.call("gfc_lg_cross_attn_backward", x, ctx, dctx, dx_in, w["to_qk.weight"], w["to_qk.bias"], w["to_v.weight"],
                 w["to_v.bias"], b, m, n, o["to_qk.weight"], o["to_qk.bias"], o["to_v.weight"], o["to_v.bias"], dx, ws,
                 ws.numel())

    out.update(alternate({"core": core, "block": block, "backward_stage": lambda: ours(False),
                          "backward_cross": lambda: ours(True), "torch_cross": torch_form}, rounds, iters))
    med = out["median_ms"]
    flop = 10.0 * 2 * 64 * 4 * b * m * n
    tf = flop / (med["core"] * 1e-3) / 1e12
    out["core"] = {"flop": flop, "tflops": tf, "fraction_of_fp32_matrix_peak": tf / PEAK_TF}
    out["cross_ms"] = med["backward_cross"] - med["backward_stage"]
    out["torch_over_ours_cross_only"] = med["torch_cross"] / out["cross_ms"]
    out["backward_cross_over_backward_stage"] = med["backward_cross"] / med["backward_stage"]
    out["workspace_bytes"] = ws.numel()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "library": nat.lib().gfc_version().decode(),
           "shapes": [bench_shape(32, 1024, 1024, args.rounds, args.iters),
                      bench_shape(8, 2048, 2048, args.rounds, args.iters)]}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "cross_attn_backward_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
