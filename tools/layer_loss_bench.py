"""Time the per-layer loss and exit report against the plain validation step, and its scoring kernel against torch.

    python tools/layer_loss_bench.py --out profiles      ->  profiles/layer_loss_bench.json

Per shape (B = 32 x 1024 + 1024 and B = 8 x 2048 + 2048 key points, synthetic weights, unit descriptors), alternating in
one process on the same GPU, medians of device-event timings in ms per batch:
  deep     LightGlue.forward_layers + layer_loss      plain    LightGlue.forward + loss        (the price of the report)
  kernel   gfc_lg_layer_scores alone                  torch    the same arithmetic as torch operations on the same GPU
`kernel` also reports the bytes it reads over its time: both log assignments [B, M+1, N+1] are read twice (along the
rows, down the columns), so the rate counts 4 B (M+1) (N+1) floats; `matrix_gb_s` counts each matrix once.
The kernel's outputs are compared with the torch form's before anything is timed.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402


def time_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(forms, rounds, iters):
    for fn in forms.values():  # warm every form at this shape
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(time_ms(fn, iters))
    return {"median_ms": {k: sorted(v)[len(v) // 2] for k, v in times.items()},
            "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()}}


def torch_scores(la, lf, x0, x1, thr):
    """TokenConfidence.loss and the predicate of check_if_stop as the reference writes them (float32)."""
    c0 = lf[:, :-1, :].max(-1).indices == la[:, :-1, :].max(-1).indices
    c1 = lf[:, :, :-1].max(-2).indices == la[:, :, :-1].max(-2).indices
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    return torch.stack([c0.sum(-1).float(), c1.sum(-1).float(), bce(x0, c0.float(), reduction="none").mean(-1),
                        bce(x1, c1.float(), reduction="none").mean(-1), (~(torch.sigmoid(x0) < thr)).sum(-1).float(),
                        (~(torch.sigmoid(x1) < thr)).sum(-1).float()], 1)


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

    def deep():
        pred = lg.forward_layers(data)
        return pred, lg.layer_loss(pred, labels)

    def plain():
        pred = lg(data)
        return pred, lg.loss(pred, labels)

    with torch.no_grad():
        (pd, (ld, report)), (pp, (lp, _)) = deep(), plain()
        out = {"B": b, "M": m, "N": n,
               "matches_equal_to_forward": bool(torch.equal(pd["matches0"], pp["matches0"])),
               "max_abs_last_nll_difference": float((ld["last"] - lp["last"]).abs().max()),
               "report_means": {k: [float(x) for x in v.float().mean(0).reshape(-1)] for k, v in report.items()},
               "step": alternate({"deep": deep, "plain": plain}, rounds, iters)}
        med = out["step"]["median_ms"]
        out["step"]["deep_over_plain"] = med["deep"] / med["plain"]
        # the kernel alone: the final assignment against the one of the first layer's own head
        la = torch.empty_like(pd["log_assignment"])
        lf = pd["log_assignment"]
        x = lg.ensure_packed(dev)[0]
        rows = pd["ref_descriptors0"][:, 0].reshape(b * m, 256)
        stack0 = torch.cat([rows, pd["ref_descriptors1"][:, 0].reshape(b * n, 256)], 0).contiguous()
        t = [torch.empty((b, m), dtype=torch.long, device=dev), torch.empty((b, n), dtype=torch.long, device=dev),
             torch.empty((b, m), device=dev), torch.empty((b, n), device=dev)]
        ws = torch.empty(max(nat.call("gfc_lg_assign_workspace_bytes", b, m, n),
                             nat.call("gfc_lg_layer_scores_workspace_bytes", b, m, n)), dtype=torch.uint8, device=dev)
        nat.call("gfc_lg_assign", ctypes.byref(x), 0, stack0, stack0[b * m:], b, m, n, 0.1, *t, la, ws, ws.numel())
        logits = torch.empty((b * (m + n),), device=dev)
        nat.call("gfc_lg_rowdot", stack0, 256, b * (m + n), x.token_w[0], x.token_b[0], 0, logits)
        x0, x1 = logits[:b * m].view(b, m), logits[b * m:].view(b, n)
        thr = float(lg.confidence_thresholds[0])
        res = torch.empty((b, 6), device=dev)

        def kernel():
            nat.call("gfc_lg_layer_scores", la, lf, x0, x1, thr, b, m, n, res, None, None, ws, ws.numel())
            return res

        ref = torch_scores(la, lf, x0, x1, thr)
        got = kernel().clone()
        out["kernel"] = {"counts_equal_to_torch": bool(torch.equal(got[:, [0, 1, 4, 5]], ref[:, [0, 1, 4, 5]])),
                         "max_abs_bce_difference": float((got[:, 2:4] - ref[:, 2:4]).abs().max()),
                         **alternate({"kernel": kernel, "torch": lambda: torch_scores(la, lf, x0, x1, thr)}, rounds,
                                     iters)}
        med = out["kernel"]["median_ms"]
        matrix_bytes = 2.0 * b * (m + 1) * (n + 1) * 4
        out["kernel"].update(torch_over_kernel=med["torch"] / med["kernel"], bytes_read=2 * matrix_bytes,
                             read_gb_s=2 * matrix_bytes / med["kernel"] / 1e6,
                             matrix_gb_s=matrix_bytes / med["kernel"] / 1e6)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layer_loss_bench needs the GPU: nothing is measured without one")
    res = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "iters_per_timing": args.iters,
           "shapes": {"b32_1024": bench_shape(32, 1024, 1024, args.rounds, args.iters),
                      "b8_2048": bench_shape(8, 2048, 2048, args.rounds, args.iters)}}
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "layer_loss_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["shapes"], indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
