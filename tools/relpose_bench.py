"""Time the GPU five-point RANSAC relative-pose estimator (eval_utils.relative_pose_ransac, csrc/relpose.hip).

    python tools/relpose_bench.py --out profiles [--pairs 512] [--keypoints 1024] [--hypotheses 2048]

`--pairs` synthetic.posed_relief_pairs with `--keypoints` + `--keypoints` key points each (about 0.7 x keypoints
matches), all in ONE call, at T = 1 (1 px) and T = 6 (the sweep).  Per configuration: `--warmup` untimed calls, then
the median device-event time of `--repeats` calls, and the split of one further call over its kernels (torch.profiler's
device activities).  The homography estimator's call (eval_utils.homography_ransac) at the same pairs, matches and T
runs in the same process as context -- it solves another problem; nothing in the parent commit is comparable.
Written to <out>/relpose_eval.json.  No GPU: an error.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from glue_factory_colon_amd import eval_utils, geometry, synthetic  # noqa: E402

SWEEP = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def kernel_split(fn):
    """{kernel name: milliseconds} of one call, from the profiler's device activities; None when it reports none."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if "cuda" in str(ev.device_type).lower() and ("ransac" in ev.name or "relpose" in ev.name):
            name = ev.name.split("(")[0].split("<")[0]
            dur = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0) or ev.cpu_time_total
            out[name] = out.get(name, 0.0) + dur / 1e3
    return out or None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--keypoints", type=int, default=1024)
    ap.add_argument("--hypotheses", type=int, default=2048)
    ap.add_argument("--model", default="PINHOLE", choices=geometry.CAMERA_MODELS)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=12)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("relpose_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda", 0)
    k = args.keypoints
    items, preds = synthetic.posed_relief_pairs(args.pairs, 480, 640, seed=7, model=args.model, num_keypoints=(k, k))
    kp0 = torch.stack([p["keypoints0"] for p in preds]).to(dev)
    kp1 = torch.stack([p["keypoints1"] for p in preds]).to(dev)
    m0 = torch.stack([p["matches0"] for p in preds]).to(dev)
    cam0 = geometry.Camera(torch.cat([it["view0"]["camera"]._data for it in items]).to(dev), model=args.model)
    cam1 = geometry.Camera(torch.cat([it["view1"]["camera"]._data for it in items]).to(dev), model=args.model)
    T = geometry.Pose(torch.cat([it["T_0to1"]._data for it in items]).to(dev))
    matches = float((m0 > -1).sum(1).float().mean())
    result = {"what": "five-point RANSAC relative pose, all pairs in one call: device-event milliseconds per call, median "
                      "of the repeats after the warm-up; kernel split of one further call; the homography estimator's "
                      "call at the same pairs / matches / T in the same process as context",
              "device": torch.cuda.get_device_name(0), "pairs": args.pairs, "keypoints": [k, k],
              "mean_matches": matches, "hypotheses": args.hypotheses, "camera_model": args.model,
              "warmup": args.warmup, "repeats": args.repeats, "configurations": {}}
    for name, ths in (("T1", [1.0]), ("T6", SWEEP)):
        def pose(ths=ths):
            return eval_utils.relative_pose_ransac(kp0, kp1, m0, cam0, cam1, ths, T, num_hypotheses=args.hypotheses)

        def homography(ths=ths):
            return eval_utils.homography_ransac(None, kp0, kp1, m0, None, ths, num_hypotheses=args.hypotheses)

        entry = {}
        for label, fn in (("relative_pose", pose), ("homography_context", homography)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ms = [timed(fn) for _ in range(args.repeats)]
            entry[label] = {"ms_per_call": ms, "median_ms": statistics.median(ms), "kernels_ms": kernel_split(fn)}
        out = pose()
        err = torch.maximum(out["r_err"], out["t_err"])
        entry["success_share"] = float(out["success"].float().mean())
        entry["median_pose_error_deg"] = [float(v) for v in err.median(0).values.tolist()]
        result["configurations"][name] = entry
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "relpose_eval.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({c: {"relative_pose_ms": e["relative_pose"]["median_ms"],
                          "homography_ms": e["homography_context"]["median_ms"],
                          "kernels_ms": e["relative_pose"]["kernels_ms"]} for c, e in result["configurations"].items()}
                     | {"written": path}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
