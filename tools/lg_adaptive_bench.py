"""Matcher-only timing of adaptive depth / width LightGlue over a list of pairs: pair by pair (`adaptive_pair_batch`
off, `forward_pairs` -> `_forward_adaptive` per pair) against the batched pass (`_forward_adaptive_pairs`), alternated
in one process.

    python tools/lg_adaptive_bench.py --out DIR [--iters N] [--warmup W]

Inputs: 32 synthetic VGA pairs, 1024 key points per image from this package's SuperPoint (name-seeded weights), the
first B = 1, 2, 8 and 32 of them; configurations (depth_confidence, width_confidence, prune_z) of
tests/adaptive_reference.py::CONFIGS on weights.lightglue_adaptive_state_dict.  Each call is timed with HIP events
after warm-up, the two paths alternating iteration by iteration.  Also recorded per case: the stop layer and the
surviving rows of every pair on both paths, and how many pairs took identical decisions.  B = 1 is there to show
whether a pair count exists below which `forward_pairs` should keep the single-pair path (`crossover_pairs` in the
output: the smallest measured B from which the batched pass is not slower in any configuration).  Writes
DIR/adaptive_pairs_bench.json.

The weights are name-seeded: where pairs stop and how much they prune is a property of those weights, so the ratios
say what batching buys at a given amount of adaptivity, nothing about the speed-up on a trained checkpoint.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import adaptive_reference as ar  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue, superpoint_open, synthetic, weights  # noqa: E402

PAIRS = (1, 2, 8, 32)


def inputs(b, h, w, k, dev):
    ext = superpoint_open.SuperPoint({"weights": "synthetic", "max_num_keypoints": k, "detection_threshold": 0.0,
                                      "nms_radius": 3, "force_num_keypoints": True}).eval().to(dev)
    v0, v1 = synthetic.synthetic_pairs(b, h, w, seed=1234, device=dev)
    size = torch.tensor([[float(w), float(h)]], device=dev)
    with torch.no_grad():
        f0, f1 = ext({"image": v0}), ext({"image": v1})
    return [{"keypoints0": f0["keypoints"][i:i + 1].contiguous(), "keypoints1": f1["keypoints"][i:i + 1].contiguous(),
             "descriptors0": f0["descriptors"][i:i + 1].contiguous(),
             "descriptors1": f1["descriptors"][i:i + 1].contiguous(),
             "view0": {"image_size": size}, "view1": {"image_size": size}} for i in range(b)]


def time_alternating(calls, iters, warmup):
    times = {name: [] for name in calls}
    with torch.no_grad():
        for _ in range(warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(iters):
            for name, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "n": len(t)}
            for name, t in times.items()}


def decisions(outs):
    return {"stop_layer": [int(o["stop_layer"]) for o in outs],
            "surviving_rows": [[o["log_assignment"].shape[1] - 1, o["log_assignment"].shape[2] - 1] for o in outs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    items = inputs(max(PAIRS), 480, 640, 1024, dev)
    result = {"tool": "tools/lg_adaptive_bench.py", "version": nat.lib().gfc_version().decode(),
              "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
              "weights": "name-seeded (weights.lightglue_adaptive_state_dict): the stop layers and pruning rates below "
                         "belong to these weights, not to a trained checkpoint",
              "cases": {}}
    slower = []
    for depth, width, pz in ar.CONFIGS:
        conf = {"filter_threshold": ar.FILTER_THRESHOLD, "depth_confidence": depth, "width_confidence": width}
        seq = lightglue.LightGlue(conf).eval()
        bat = lightglue.LightGlue({**conf, "adaptive_pair_batch": True}).eval()
        for m in (seq, bat):
            m.load_state_dict(weights.lightglue_adaptive_state_dict(0, prune_z=pz), strict=False)
            m.to(dev)
        for b in PAIRS:
            sub = items[:b]
            calls = {"sequential": lambda: seq.forward_pairs(sub), "batched": lambda: bat.forward_pairs(sub)}
            t = time_alternating(calls, args.iters, args.warmup)
            with torch.no_grad():
                ds, db = decisions(calls["sequential"]()), decisions(calls["batched"]())
            t["batched_over_sequential"] = t["batched"]["median_ms"] / t["sequential"]["median_ms"]
            t["pairs_per_s_matcher_only"] = {k: b * 1000.0 / t[k]["median_ms"] for k in ("sequential", "batched")}
            t["sequential_decisions"], t["batched_decisions"] = ds, db
            t["pairs_with_identical_decisions"] = sum(
                1 for i in range(b) if ds["stop_layer"][i] == db["stop_layer"][i]
                and ds["surviving_rows"][i] == db["surviving_rows"][i])
            name = f"depth{depth}_width{width}_prunez{pz}_b{b}"
            if t["batched_over_sequential"] > 1.0:
                slower.append(name)
            result["cases"][name] = t
            print(name, json.dumps({k: t[k] for k in ("sequential", "batched", "batched_over_sequential")}), flush=True)
    result["batched_slower_in"] = slower
    ok = [b for b in PAIRS if not any(n.endswith(f"_b{c}") for n in slower for c in PAIRS if c >= b)]
    result["crossover_pairs"] = min(ok) if ok else None
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "adaptive_pairs_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"batched_slower_in": slower}))


if __name__ == "__main__":
    main()
