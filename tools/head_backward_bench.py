"""Time the head and exit-token gradients against float32 torch autograd of the same heads and loss, and record how
much of their per-element bounds they use.

    python tools/head_backward_bench.py --out profiles  ->  profiles/head_backward_bench.json, head_backward_parity.json

Per shape (B = 32 x 1024 + 1024 and B = 8 x 2048 + 2048 key points, name-seeded weights, unit descriptors), alternating
in one process on the same GPU, medians of device-event timings in ms per batch:
  backward      LightGlue.layer_loss_backward(accumulate=False)          backward_dx   the same with descriptor_grads
  torch         the same nine heads, eight tokens and loss as float32 torch operations with autograd on the same GPU, a
  torch_dx      layer at a time (forward and backward of the head: autograd has to run the forward it differentiates);
                _dx: the layer's descriptors require a gradient too
  forward       LightGlue.forward_layers + layer_loss
  kernel        gfc_lg_head_backward alone on one layer (with dx): the TFLOP/s of its matrix part -- md, S, G md1,
                G^T md0, dmd^T x, dmd Wf: 2 * 256 * (3 R 256 + 3 B M N) flop, R = B (M + N) -- against the 157 TF peak of
                the fp32 matrix instructions
The torch form is the comparison; its gradients are compared with the module's before anything is timed.

head_backward_parity.json: the largest fraction of its bound c 2^-23 abs-sum (tests/head_grad_reference.py) that any
element of each output uses, on the two fixture batches (all three loss.gamma, against the closed form on the device's
own descriptors).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402

PEAK_TF = 157.0


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


def torch_head(x0, x1, head):
    """MatchAssignment + sigmoid_log_double_softmax as the reference writes them (lightglue.py:257-288)."""
    F = torch.nn.functional
    md0, md1 = head.final_proj(x0) / 4.0, head.final_proj(x1) / 4.0
    sim = torch.einsum("bmd,bnd->bmn", md0, md1)
    z0, z1 = head.matchability(x0), head.matchability(x1)
    b, m, n = sim.shape
    scores = sim.new_full((b, m + 1, n + 1), 0)
    scores[:, :m, :n] = F.log_softmax(sim, 2) + F.log_softmax(sim.transpose(-1, -2).contiguous(), 2).transpose(-1, -2) \
        + F.logsigmoid(z0) + F.logsigmoid(z1).transpose(1, 2)
    scores[:, :-1, -1] = F.logsigmoid(-z0.squeeze(-1))
    scores[:, -1, :-1] = F.logsigmoid(-z1.squeeze(-1))
    return scores


def torch_nll(la, weights, balancing=0.5):
    """weight_loss + NLLLoss.forward (losses.py:6-60)."""
    m, n = la.shape[1] - 1, la.shape[2] - 1
    sc = la * weights
    num_neg = weights[:, :m, -1].sum(-1).clamp(min=1.0) + weights[:, -1, :n].sum(-1).clamp(min=1.0)
    num_pos = weights[:, :m, :n].sum((-1, -2)).clamp(min=1.0)
    nll_pos = -sc[:, :m, :n].sum((-1, -2)) / num_pos
    nll_neg = (-sc[:, :m, -1].sum(-1) - sc[:, -1, :n].sum(-1)) / num_neg
    return balancing * nll_pos + (1 - balancing) * nll_neg


def torch_backward(lg, pred, weights, layer_weights, with_dx):
    """.grad of every head and token from autograd, a layer at a time (one log assignment alive); -> the dx list."""
    nl = lg.conf.n_layers
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    final = pred["log_assignment"]
    dxs = []
    for i in range(nl):
        x0 = pred["ref_descriptors0"][:, i].detach().requires_grad_(with_dx)
        x1 = pred["ref_descriptors1"][:, i].detach().requires_grad_(with_dx)
        la = torch_head(x0, x1, lg.log_assignment[i])
        total = torch_nll(la, weights) * layer_weights[i]
        if i < nl - 1:
            tok = lg.token_confidence[i].token[0]
            now = la.detach()
            c0 = final[:, :-1, :].max(-1).indices == now[:, :-1, :].max(-1).indices
            c1 = final[:, :, :-1].max(-2).indices == now[:, :, :-1].max(-2).indices
            conf = (bce(tok(x0.detach()).squeeze(-1), c0.float(), reduction="none").mean(-1)
                    + bce(tok(x1.detach()).squeeze(-1), c1.float(), reduction="none").mean(-1)) / 2.0
            total = total + conf / (nl - 1)
        torch.mean(total).backward()
        if with_dx:
            dxs.append((x0.grad, x1.grad))
    return dxs


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
    with torch.no_grad():
        pred = lg.forward_layers(data)
    # the reference's weight matrix (losses.py:62-73), made once: it depends on the labels only
    weights = torch.zeros((b, m + 1, n + 1), device=dev)
    bi, ii = torch.nonzero(gt0 > -1, as_tuple=True)
    weights[bi, ii, gt0[bi, ii]] = 1.0
    weights[:, :m, -1] = (gt0 == -1).float()
    weights[:, -1, :n] = (gt1 == -1).float()
    lw = [1.0] * nl  # loss.gamma 1.0
    lw = [w / sum(lw) for w in lw]

    def ours(dx):
        return lg.layer_loss_backward(pred, labels, descriptor_grads=dx, accumulate=False)

    def torch_form(dx):
        for p in lg.parameters():
            p.grad = None
        return torch_backward(lg, pred, weights, lw, dx)

    def forward():
        with torch.no_grad():
            p = lg.forward_layers(data)
            return lg.layer_loss(p, labels)

    # the two forms agree before anything is timed
    mine = ours(True)
    dxs = torch_form(True)
    worst = 0.0
    for k, v in mine.items():
        if k.startswith("grad_ref"):
            continue
        ref = lg.get_parameter(k).grad
        worst = max(worst, float((v - ref).abs().max() / ref.abs().max().clamp(min=1e-30)))
    dx0 = torch.stack([d[0] for d in dxs], 1)
    worst_dx = float((mine["grad_ref_descriptors0"] - dx0).abs().max() / dx0.abs().max())
    out = {"B": b, "M": m, "N": n, "max_difference_over_max_abs": {"parameters": worst, "dx0": worst_dx}}
    del mine, dxs, dx0
    out.update(alternate({"backward": lambda: ours(False), "backward_dx": lambda: ours(True),
                          "torch": lambda: torch_form(False), "torch_dx": lambda: torch_form(True),
                          "forward": forward}, rounds, iters))
    med = out["median_ms"]
    out["torch_over_backward"] = med["torch"] / med["backward"]
    out["torch_dx_over_backward_dx"] = med["torch_dx"] / med["backward_dx"]
    out["backward_over_forward"] = med["backward"] / med["forward"]
    out["backward_dx_over_forward"] = med["backward_dx"] / med["forward"]
    # the head kernel alone on one layer
    params = lg.ensure_packed(dev)[0]
    rows = b * (m + n)
    x = torch.cat([pred["ref_descriptors0"][:, 4].reshape(b * m, 256), pred["ref_descriptors1"][:, 4].reshape(b * n, 256)],
                  0).contiguous()
    gw = torch.full((b,), 1.0 / b, device=dev)
    o = [torch.empty((256, 256), device=dev), torch.empty((256,), device=dev), torch.empty((256,), device=dev),
         torch.empty((1,), device=dev), torch.empty((rows, 256), device=dev)]
    ws = torch.empty(nat.call("gfc_lg_head_backward_workspace_bytes", b, m, n), dtype=torch.uint8, device=dev)

    def kernel():
        nat.call("gfc_lg_head_backward", ctypes.byref(params), 4, x, x[b * m:], gt0, gt1, None, gw, 0.5, b, m, n, *o, ws,
                 ws.numel())

    k = alternate({"kernel": kernel}, rounds, iters)
    flop = 2.0 * 256 * (3.0 * rows * 256 + 3.0 * b * m * n)
    tf = flop / (k["median_ms"]["kernel"] * 1e-3) / 1e12
    out["kernel"] = {"median_ms": k["median_ms"]["kernel"], "matrix_flop": flop, "tflops": tf,
                     "fraction_of_fp32_matrix_peak": tf / PEAK_TF, "workspace_bytes": ws.numel()}
    return out


def parity():
    """{output: the largest fraction of its bound used}."""
    import head_grad_reference as hg
    import layer_loss_cases as lc

    dev = torch.device("cuda")
    worst = {}
    for name in ("a", "b"):
        z = np.load(os.path.join(ROOT, "tests", "golden", f"head_grad_{name}_gamma1.npz"))
        case = lc.make_case(name, int(z["seed"]))
        c = lambda k: case[k].to(dev)  # noqa: E731
        data = {"keypoints0": c("keypoints0"), "keypoints1": c("keypoints1"), "descriptors0": c("descriptors0"),
                "descriptors1": c("descriptors1"), "view0": {"image_size": c("size")}, "view1": {"image_size": c("size")}}
        labels = {"gt_matches0": c("gt_matches0"), "gt_matches1": c("gt_matches1")}
        if case["gt_assignment"] is not None:
            labels["gt_assignment"] = c("gt_assignment")
        cpu = {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"], "gt_assignment": case["gt_assignment"]}
        for gamma in (0.5, 0.0, 1.0):
            lg = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.0, "loss": {"gamma": gamma}}).eval().to(dev)
            with torch.no_grad():
                pred = lg.forward_layers(data)
            grads = lg.layer_loss_backward(pred, labels, descriptor_grads=True, accumulate=False)
            xs0 = [pred["ref_descriptors0"][:, i].double().cpu() for i in range(lc.N_LAYERS)]
            xs1 = [pred["ref_descriptors1"][:, i].double().cpu() for i in range(lc.N_LAYERS)]
            sd = {k: v.detach().double().cpu() for k, v in lg.state_dict().items()}
            want, sums, cs = hg.model_grads(xs0, xs1, sd, cpu, gamma=gamma, descriptor_grads=True)
            for k, w in want.items():
                frac = float(((grads[k].double().cpu() - w).abs() / (cs[k] * hg.U * sums[k])).max())
                key = k.split(".", 2)[-1]
                worst[key] = max(worst.get(key, 0.0), frac)
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_backward_bench needs the GPU: nothing is measured without one")
    os.makedirs(args.out, exist_ok=True)
    par = {"what": "largest fraction of the per-element bound c 2^-23 abs-sum used, per output",
           "device": torch.cuda.get_device_name(0), "worst_fraction": parity()}
    with open(os.path.join(args.out, "head_backward_parity.json"), "w") as f:
        json.dump(par, f, indent=1)
    print(json.dumps(par, indent=1), flush=True)
    res = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "iters_per_timing": args.iters, "fp32_matrix_peak_tflops": PEAK_TF, "shapes": {}}
    for key, shape in (("b32_1024", (32, 1024, 1024)), ("b8_2048", (8, 2048, 2048))):
        res["shapes"][key] = bench_shape(*shape, args.rounds, args.iters)
        print(key, json.dumps(res["shapes"][key], indent=1), flush=True)
    path = os.path.join(args.out, "head_backward_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
