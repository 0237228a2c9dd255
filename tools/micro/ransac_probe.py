"""What the GPU RANSAC homography estimator costs (profiles/ransac_eval.json): medians of >= 10 repetitions after warm-up,
HIP events for the kernel calls.

  (a) `eval_utils.homography_ransac` at B = 540, ~700 matches of 1024 key points, 2048 hypotheses, T = 1 and T = 6;
  (b) `HPatchesPipeline.run_eval` on a 540-pair synthetic HPatches-shaped directory without and with the estimator
      (six-threshold sweep);
  (c) for context: the float64 numpy restatement (tests/ransac_reference.py) on 8 of the pairs of (a), 8 processes.

    python tools/micro/ransac_probe.py [out.json] [--kernels-only]     (--kernels-only: three calls of (a), for a kernel trace)
"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ransac_reference as rr  # noqa: E402

from glue_factory_colon_amd import eval_hpatches, eval_utils, synthetic  # noqa: E402

B, KPTS, HYP, REPS = 540, 1024, 2048, 12


def make_cases(count):
    return [rr.make_case(KPTS, 0.3, 0.5, seed=9000 + i, unmatched_share=0.316) for i in range(count)]


def restate(args):
    c, sid = args
    t = time.perf_counter()
    res = rr.ransac(c["kp0"], c["kp1"], c["m0"], rr.SWEEP, HYP, 3, 0, sid, c["H_gt"], c["size"])
    return time.perf_counter() - t, [x["error"] for x in res]


def event_median(fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def write_ppm(path, img):
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n" + f"{w} {h}\n255\n".encode() + img.tobytes())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels-only" in sys.argv
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "ransac_eval.json")
    cases = make_cases(B)
    result = {"device": None, "B": B, "key_points": KPTS, "hypotheses": HYP, "lo_iters": 3, "repetitions": REPS,
              "mean_matches": float(np.mean([(c["m0"] >= 0).sum() for c in cases]))}
    if not kernels_only:  # (c) first: the worker processes are forked before this process touches the GPU
        t = time.perf_counter()
        with ProcessPoolExecutor(max_workers=8) as ex:
            per = list(ex.map(restate, [(c, i) for i, c in enumerate(cases[:8])]))
        result["c_restatement_8_pairs_T6"] = {"wall_s_8_processes": time.perf_counter() - t,
                                              "per_pair_s": [p[0] for p in per]}
        print("(c)", result["c_restatement_8_pairs_T6"], flush=True)
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(0)

    def st(key, dtype):
        return torch.from_numpy(np.stack([c[key] for c in cases])).to(device=dev, dtype=dtype)

    H, kp0, kp1, m0, size = st("H_gt", torch.float32), st("kp0", torch.float32), st("kp1", torch.float32), st("m0", torch.long), st("size", torch.float32)
    sids = torch.arange(B, device=dev)
    if kernels_only:
        for ths in ([1.0], rr.SWEEP):
            for _ in range(3):
                eval_utils.homography_ransac(H, kp0, kp1, m0, size, ths, num_hypotheses=HYP, stream_id=sids)
        torch.cuda.synchronize()
        return
    result["a_homography_ransac_ms"] = {}
    for name, ths in (("T1", [1.0]), ("T6", rr.SWEEP)):
        med, lo, hi = event_median(lambda: eval_utils.homography_ransac(H, kp0, kp1, m0, size, ths, num_hypotheses=HYP, stream_id=sids))
        out = eval_utils.homography_ransac(H, kp0, kp1, m0, size, ths, num_hypotheses=HYP, stream_id=sids)
        result["a_homography_ransac_ms"][name] = {"median": med, "min": lo, "max": hi, "thresholds": ths,
                                                  "median_corner_error_px": out["error"].median(0).values.cpu().tolist()}
        print("(a)", name, result["a_homography_ransac_ms"][name], flush=True)
    med, lo, hi = event_median(lambda: eval_utils.homography_dlt(H, kp0, kp1, m0, torch.ones_like(kp0[..., 0]), size))
    result["a_homography_dlt_ms_for_scale"] = {"median": med, "min": lo, "max": hi}
    # (b) the evaluation pass on a 540-pair directory
    root = tempfile.mkdtemp(prefix="gfc_rs_")
    try:
        raw = synthetic.hpatches_like_host_images(B, seed=7000, pin=False, shared_view0=True)
        for i, it in enumerate(raw):
            d = os.path.join(root, "hpatches-sequences-release", "v_" + it["scene"])
            os.makedirs(d, exist_ok=True)
            if i % 5 == 0:
                write_ppm(os.path.join(d, "1.ppm"), it["view0"]["image"].numpy())
            write_ppm(os.path.join(d, f"{i % 5 + 2}.ppm"), it["view1"]["image"].numpy())
            with open(os.path.join(d, f"H_1_{i % 5 + 2}"), "w") as f:
                f.write("1 0 0\n0 1 0\n0 0 1\n")
        del raw
        print("directory written", flush=True)
        data = {"data_dir": os.path.join(root, "hpatches-sequences-release")}
        model = eval_hpatches.build_model("synthetic", "synthetic", official=True).cuda()
        plain = eval_hpatches.HPatchesPipeline(data, pair_batch=32, num_workers=8)
        pred = plain.get_predictions(os.path.join(root, "exp"), model, overwrite=True)
        robust = eval_hpatches.HPatchesPipeline(data, pair_batch=32, num_workers=8,
                                                eval_conf={"estimator": "gfc_amd", "ransac_th": -1})
        result["b_run_eval_s"] = {}
        for name, pipe in (("without_estimator", plain), ("with_estimator_sweep", robust), ("without_estimator_again", plain)):
            times = []
            for rep in range(REPS + 2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                summaries, _ = pipe.run_eval(pred)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t)
            times = times[2:]
            result["b_run_eval_s"][name] = {"median": statistics.median(times), "min": min(times), "max": max(times)}
            print("(b)", name, result["b_run_eval_s"][name], flush=True)
            if name == "with_estimator_sweep":
                result["b_summaries_with_estimator"] = {k: v for k, v in summaries.items()
                                                        if "ransac" in k or "dlt" in k or k == "mean_num_matches"}
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
