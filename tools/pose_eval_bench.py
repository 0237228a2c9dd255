"""Time the pose / depth evaluation: the kernels (eval_utils.pose_depth_metrics + pose_epipolar_metrics, csrc/eval_pose.hip)
against the torch-op form of the same arithmetic (tests/pose_reference.py) with its tensors on the same GPU.

    python tools/pose_eval_bench.py --out profiles [--pairs 512] [--keypoints 1024] [--model OPENCV_FISHEYE]

`--pairs` synthetic.posed_plane_pairs with `--keypoints` + `--keypoints` key points each.  One pass = all pairs
through both metrics: the kernel path in calls of `--batch` pairs, the torch path pair by pair (it builds each pair's
M x N matrices, as the reference's functions do).  The two paths alternate in ONE process, each pass timed with device
events (the torch path ends every pair in a host read, the kernel path every call), and the medians are reported as
pairs/s in <out>/pose_eval_bench.json.  Before timing, the two paths' results are compared.  No GPU: an error.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_reference as pr  # noqa: E402
from glue_factory_colon_amd import eval_utils, geometry, synthetic  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--keypoints", type=int, default=1024)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--model", default="OPENCV_FISHEYE", choices=geometry.CAMERA_MODELS)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_eval_bench needs a GPU: a CPU timing says nothing about the kernels")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    dev = torch.device("cuda", 0)
    k = args.keypoints
    items, preds = synthetic.posed_plane_pairs(args.pairs, args.height, args.width, seed=7, model=args.model,
                                               num_keypoints=(k, k))
    cat = lambda f: torch.cat([f(it) for it in items]).to(dev)  # noqa: E731
    kp0 = torch.stack([p["keypoints0"] for p in preds]).to(dev)
    kp1 = torch.stack([p["keypoints1"] for p in preds]).to(dev)
    m0 = torch.stack([p["matches0"] for p in preds]).to(dev)
    depth0, depth1 = cat(lambda it: it["view0"]["depth"]), cat(lambda it: it["view1"]["depth"])
    cam0, cam1 = cat(lambda it: it["view0"]["camera"]._data), cat(lambda it: it["view1"]["camera"]._data)
    T = cat(lambda it: it["T_0to1"]._data)

    def kernel_pass():
        rows = []
        for s in range(0, args.pairs, args.batch):
            e = slice(s, s + args.batch)
            c0, c1 = geometry.Camera(cam0[e], model=args.model), geometry.Camera(cam1[e], model=args.model)
            P = geometry.Pose(T[e])
            dep = eval_utils.pose_depth_metrics(kp0[e], kp1[e], m0[e], depth0[e], depth1[e], c0, c1, P)
            epi = eval_utils.pose_epipolar_metrics(kp0[e], kp1[e], m0[e], c0, c1, P)
            rows.append(torch.cat([dep, epi], 1).cpu())  # the host read that ends a call
        return torch.cat(rows)

    def torch_pass():
        dep, _, _ = pr.depth_metrics(kp0, kp1, m0, depth0, depth1, cam0, args.model, cam1, args.model, T)
        epi = pr.epipolar_metrics(kp0, kp1, m0, cam0, args.model, cam1, args.model, T)
        return torch.cat([dep, epi], 1)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / 1e3, out

    # warm-up of both paths, and the comparison of what they compute: counts equal, ratios to 4 / (number of matches)
    # (the two run the same float32 arithmetic in different operation orders on real-sized scenes: a match whose error
    # lies within a rounding error of a threshold may fall on either side; the fixture of the tests has no such match)
    a, b = kernel_pass().double(), torch_pass()
    count_cols, ratio_cols = [3, 10, 11], [0, 1, 2, 5, 6, 7, 8, 9]
    n_match = float(a[:, 10].min())
    worst = float((a[:, ratio_cols] - b[:, ratio_cols]).abs().max())
    assert worst <= 4.0 / max(n_match, 1), f"the two paths disagree: ratios differ by {worst}"
    assert float((a[:, count_cols] - b[:, count_cols]).abs().max()) <= 2, "the two paths disagree in a count"
    t_kernel, t_torch = [], []
    for _ in range(args.passes):
        t_kernel.append(timed(kernel_pass)[0])
        t_torch.append(timed(torch_pass)[0])
    result = {
        "what": "pose / depth + epipolar match metrics of posed pairs: device-event time of one pass over all pairs, "
                "median of the passes; the two paths alternate in one process on the same GPU",
        "device": torch.cuda.get_device_name(0), "pairs": args.pairs, "keypoints": [k, k],
        "depth_map": [args.height, args.width], "camera_model": args.model, "kernel_batch": args.batch,
        "passes": args.passes,
        "kernel_path": {"seconds_per_pass": t_kernel, "median_s": statistics.median(t_kernel),
                        "pairs_per_s": args.pairs / statistics.median(t_kernel)},
        "torch_path_same_gpu": {"seconds_per_pass": t_torch, "median_s": statistics.median(t_torch),
                                "pairs_per_s": args.pairs / statistics.median(t_torch)},
        "largest_ratio_difference_between_the_paths": worst,
    }
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "pose_eval_bench.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"kernel_pairs_per_s": result["kernel_path"]["pairs_per_s"],
                      "torch_pairs_per_s": result["torch_path_same_gpu"]["pairs_per_s"], "written": path}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
