"""Time the last self block's backward against float32 torch autograd of the same block.

    python tools/self_block_backward_bench.py --out profiles  ->  profiles/self_block_backward_bench.json

Per shape (B = 32 x 1024 + 1024 and B = 8 x 2048 + 2048 key points, name-seeded weights, unit descriptors), alternating
in one process on the same GPU, medians of device-event timings in ms per batch:
  core             gfc_attention_self_backward alone on the block's own rotated qkv: TFLOP/s at 8 * 2 * 64 flop per score
                   element, head and side against the 157 TF peak of the fp32 matrix instructions (the EXECUTED products:
                   S three times and dctx v^T twice among them; 5 of the 8 are the minimum, so the useful rate is 5 / 8
                   of the figure -- the cross core's figure counts 10 executed against a minimum of 7)
  block            gfc_lg_self_attn_backward (Wqkv with rotary, the core, the two reductions, dx)
  backward_cross   LightGlue.layer_loss_backward(accumulate=False, output_stage=True, cross_attention=True): the parent's
  backward_self    the same with self_block=True
  torch_self       the self block (Wqkv, rotary, attention, out_proj, FFN) as float32 torch operations from the rows of
                   layer L - 2, and autograd of sum(y * dy) for its ten tensors and the rows (autograd has to run the
                   forward it differentiates; it stores the [B,4,n,n] matrices)
The yardstick is torch_self against backward_self - backward_cross (what the self block adds).
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

ON = {"output_stage": True, "cross_attention": True}


def torch_self(sa, xs, tabs, dys):
    """.grad of the ten tensors and of the rows, from autograd on the reference's formulation (lightglue.py:43-50,
    124-129, 151-164), per side."""
    half = lambda t: torch.stack((-t[..., 1::2], t[..., 0::2]), -1).flatten(-2)  # noqa: E731
    leaves, total = [x.detach().requires_grad_() for x in xs], 0.0
    for x, (c, s), dy in zip(leaves, tabs, dys):
        qkv = sa.Wqkv(x).unflatten(-1, (4, -1, 3)).transpose(1, 2)
        q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
        q, k = q * c + half(q) * s, k * c + half(k) * s
        ctx = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).flatten(start_dim=-2)
        y = x + sa.ffn(torch.cat([x, sa.out_proj(ctx)], -1))
        total = total + (y * dy).sum()
    total.backward()
    return [x.grad for x in leaves]


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
    pre = f"transformers.{nl - 1}.self_attn."
    sa = lg.transformers[nl - 1].self_attn
    with torch.no_grad():
        pred = lg.forward_layers(data, keep_output_stage=True, keep_self_block=True)

    def ours(self_block):
        return lg.layer_loss_backward(pred, labels, accumulate=False, self_block=self_block, **ON)

    mine = ours(True)
    cos, sin = pred["self_block_cos"], pred["self_block_sin"]
    xs = [pred["ref_descriptors0"][:, nl - 2].contiguous(), pred["ref_descriptors1"][:, nl - 2].contiguous()]
    tabs = [(cos[:b * m].reshape(b, 1, m, 64), sin[:b * m].reshape(b, 1, m, 64)),
            (cos[b * m:].reshape(b, 1, n, 64), sin[b * m:].reshape(b, 1, n, 64))]
    dys = [mine["grad_cross_block_rows0"], mine["grad_cross_block_rows1"]]

    def torch_form():
        for p in lg.parameters():
            p.grad = None
        return torch_self(sa, xs, tabs, dys)

    gx = torch_form()
    rel = lambda a, ref: float((a - ref).abs().max() / ref.abs().max().clamp(min=1e-30))  # noqa: E731
    names = [k for k, _ in sa.named_parameters()]
    out = {"B": b, "M": m, "N": n,
           "max_difference_over_max_abs": {**{k: rel(mine[pre + k], sa.get_parameter(k).grad) for k in names},
                                           "grad_self_block_rows": max(rel(mine["grad_self_block_rows0"], gx[0]),
                                                                       rel(mine["grad_self_block_rows1"], gx[1]))}}
    rows = b * (m + n)
    flat = lambda a, c: torch.cat([a.reshape(-1, 256), c.reshape(-1, 256)], 0).contiguous()  # noqa: E731
    x, ctx = flat(*xs), flat(pred["self_block_context0"], pred["self_block_context1"])
    dctx = flat(mine["grad_output_stage_context0"], mine["grad_output_stage_context1"])  # (of the right size and scale)
    dx_in = flat(*dys)
    del mine, gx
    by_ptr = {t.data_ptr(): t for t in lg._packed[1]}
    wqkv, bqkv = by_ptr[lg._packed[0].wqkv[nl - 1]], by_ptr[lg._packed[0].bqkv[nl - 1]]
    qkv, dqkv = torch.empty((rows, 768), device=dev), torch.empty((rows, 768), device=dev)
    nat.call("gfc_linear", x, 256, 256, None, 0, 0, wqkv, 256, bqkv, None, None, 1.0, None, cos, sin, 512, qkv, 768, rows, 768)
    dw, db, dx = torch.empty_like(wqkv), torch.empty_like(bqkv), torch.empty_like(x)
    ws = torch.empty(nat.call("gfc_lg_self_attn_backward_workspace_bytes", b, m, n), dtype=torch.uint8, device=dev)
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream

    def core():
        nat.check(lib.gfc_attention_self_backward(qkv.data_ptr(), 768, ctx.data_ptr(), 256, dctx.data_ptr(), 256,
                                                  cos.data_ptr(), sin.data_ptr(), b, m, n, 4, 0.125, dqkv.data_ptr(), 768,
                                                  ws.data_ptr(), ws.numel(), stream), "core")

    def block():
        nat.call("gfc_lg_self_attn_backward", x, cos, sin, ctx, dctx, dx_in, wqkv, bqkv, b, m, n, dw, db, dx, ws, ws.numel())

    out.update(alternate({"core": core, "block": block, "backward_cross": lambda: ours(False),
                          "backward_self": lambda: ours(True), "torch_self": torch_form}, rounds, iters))
    med = out["median_ms"]
    flop = 8.0 * 2 * 64 * 4 * b * (m * m + n * n)
    tf = flop / (med["core"] * 1e-3) / 1e12
    out["core"] = {"flop": flop, "tflops": tf, "fraction_of_fp32_matrix_peak": tf / PEAK_TF}
    out["self_ms"] = med["backward_self"] - med["backward_cross"]
    out["torch_over_ours_self_only"] = med["torch_self"] / out["self_ms"]
    out["backward_self_over_backward_cross"] = med["backward_self"] / med["backward_cross"]
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
    with open(os.path.join(args.out, "self_block_backward_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
