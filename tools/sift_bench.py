"""Extraction-only timing of the SIFT extractor, and its pyramid kernel against the same pyramid as torch operations.

    python tools/sift_bench.py --out DIR [--iters N] [--warmup W]

Cases: B = 32 images of 480 x 640 (four seeded fixtures -- blobs and band-limited noise inside a black vignette -- repeated), max_num_keypoints
1024 and 4096, first_octave -1 and 0, four octaves.  Timed with device events after warm-up:
  * the model's whole call (`SIFT._forward`: the stages, the post-processing and its two reads of counts);
  * every stage alone on the inputs the model gives it (pyramid, detect, orient, describe, filter);
  * the pyramid as torch operations -- F.interpolate(scale 2, bilinear) and separable F.conv2d with the same fp32 taps
    and replicate padding, DoG by subtraction, the next octave by slicing -- alternating with the HIP pyramid, call by
    call, in one process.  The two are compared before anything is timed.
The pyramid's traffic is counted from the shapes (per level: its input read once, the level and its DoG level written
once, the decimated copy of level 3) and reported over the HIP pyramid's time, as a fraction of 8 TB/s.
Writes DIR/sift_bench.json.  No threshold is asserted: these figures had not been measured before.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import sift_reference as sr  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import sift  # noqa: E402

HBM_PEAK = 8.0e12
CAP = 65536


def timed(fns, iters, warmup):
    """name -> callable; alternating, one event pair per call"""
    times = {name: [] for name in fns}
    with torch.no_grad():
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(iters):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "n": len(t)}
            for name, t in times.items()}


def torch_pyramid(image, first_octave, num_octaves, taps):
    """[B,H,W] -> (gauss, dog): lists per octave of [B,6,h,w] and [B,5,h,w]."""
    x = image[:, None]
    if first_octave < 0:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)

    def blur(x, t):
        r = t.numel() // 2
        x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="replicate"), t.view(1, 1, 1, -1))
        return F.conv2d(F.pad(x, (0, 0, r, r), mode="replicate"), t.view(1, 1, -1, 1))

    gauss, dog = [], []
    for o in range(num_octaves):
        if min(x.shape[-2:]) < sr.MIN_SIDE:
            break
        levels = [blur(x, taps[0]) if o == 0 else x]
        for s in range(1, 6):
            levels.append(blur(levels[-1], taps[s]))
        g = torch.cat(levels, 1)
        gauss.append(g)
        dog.append(g[:, 1:] - g[:, :-1])
        h, w = x.shape[-2:]
        x = levels[3][:, :, 0: 2 * (h // 2): 2, 0: 2 * (w // 2): 2].contiguous()
    return gauss, dog


def pyramid_bytes(b, h, w, lay, first_octave):
    total = 0
    for o, oc in enumerate(lay.octaves):
        plane = oc.h * oc.w
        if o == 0:
            total += h * w + plane  # the input (read through the up-sample when first_octave = -1) and level 0
        total += 5 * 3 * plane  # levels 1..5: one plane read, the level and the DoG level written
        if o + 1 < len(lay.octaves):
            total += lay.octaves[o + 1].h * lay.octaves[o + 1].w  # the decimated copy
    return 4 * b * total


def case(images, k, first_octave, iters, warmup):
    dev = images.device
    b, _, h, w = images.shape
    no = 4
    model = sift.SIFT({"max_num_keypoints": k, "first_octave": first_octave, "num_octaves": no,
                       "force_num_keypoints": True, "candidate_cap": CAP}).eval()
    plane = images[:, 0].contiguous()
    taps = [torch.from_numpy(sr.gaussian_taps(s)).to(dev) for s in sr.step_sigmas(first_octave)]
    with torch.no_grad():
        pred = model({"image": images})
        gauss, dog, lay = sift.pyramid(plane, None, first_octave, no)
        tg, td = torch_pyramid(plane, first_octave, no, taps)
        diff = max(float((sift.level(gauss, lay, 0, o, s) - tg[o][0, s]).abs().max()) for o in range(len(tg)) for s in range(6))
        assert diff < 1e-5, diff
        raw_f, raw_i, counts = sift.detect(dog, h, w, None, first_octave, no, cap=CAP)
        host = counts.cpu()
        assert int(host[:, 2].max()) == 0
        n_raw = int(host[:, 0].max())
        raw_f, raw_i = raw_f[:, :n_raw].contiguous(), raw_i[:, :n_raw].contiguous()
        ori_f, ori_i, ocounts = sift.orient(gauss, h, w, raw_f, raw_i, counts, None, first_octave, no, ocap=4 * n_raw)
        desc = sift.describe(gauss, h, w, ori_f, ori_i, ocounts, None, first_octave, no)
    t = timed({
        "model": lambda: model({"image": images}),
        "pyramid_hip": lambda: sift.pyramid(plane, None, first_octave, no),
        "pyramid_torch_ops": lambda: torch_pyramid(plane, first_octave, no, taps),
        "detect": lambda: sift.detect(dog, h, w, None, first_octave, no, cap=CAP),
        "orient": lambda: sift.orient(gauss, h, w, raw_f, raw_i, counts, None, first_octave, no, ocap=4 * n_raw),
        "describe": lambda: sift.describe(gauss, h, w, ori_f, ori_i, ocounts, None, first_octave, no),
        "filter": lambda: sift.filter_list(ori_f, desc, ocounts, h, w, None, None, 0, False, k, True, out_cap=k),
    }, iters, warmup)
    nbytes = pyramid_bytes(b, h, w, lay, first_octave)
    hip = t["pyramid_hip"]["median_ms"]
    return {"B": b, "H": h, "W": w, "max_num_keypoints": k, "first_octave": first_octave, "num_octaves": len(lay.octaves),
            "times": t, "images_per_second": b / t["model"]["median_ms"] * 1e3,
            "key_points_raw_per_image": float(host[:, 0].float().mean()),
            "candidates_per_image": float(host[:, 1].float().mean()),
            "key_points_oriented_per_image": float(ocounts[:, 0].float().mean()),
            "key_points_returned_per_image": float(pred["num_keypoints_detected"].float().mean()),
            "pyramid_bytes": nbytes, "pyramid_bytes_per_second": nbytes / (hip * 1e-3),
            "pyramid_fraction_of_hbm_peak": nbytes / (hip * 1e-3) / HBM_PEAK,
            "pyramid_speedup_over_torch_ops": t["pyramid_torch_ops"]["median_ms"] / hip,
            "pyramid_hip_vs_torch_ops_max_abs_diff": diff}


def dense_image(seed, h=480, w=640):
    """The textured fixture plus band-limited noise (a few thousand key points per image), black outside the vignette."""
    base = sr.textured_image(h, w, seed, n=500)
    noise = sr.blur(np.random.RandomState(seed).rand(h, w), sr.gaussian_taps(1.5))
    img = np.clip(base + 0.8 * (noise - 0.5), 0.0, 1.0)
    img[base == 0] = 0.0
    return img.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sift_bench needs the GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    four = np.stack([dense_image(200 + i) for i in range(4)])
    images = torch.from_numpy(four).repeat((args.batch + 3) // 4, 1, 1)[: args.batch, None].contiguous().to(dev)
    cases = [case(images, k, fo, args.iters, args.warmup) for fo in (-1, 0) for k in (1024, 4096)]
    for c in cases:
        print(json.dumps({k: c[k] for k in ("first_octave", "max_num_keypoints", "images_per_second",
                                            "pyramid_fraction_of_hbm_peak", "pyramid_speedup_over_torch_ops")}
                         | {name: round(v["median_ms"], 3) for name, v in c["times"].items()}))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "sift_bench.json"), "w") as f:
        json.dump({"what": "SIFT extraction alone (backend gfc_amd), seeded textured fixtures; stages alone and the pyramid "
                           "against torch operations, alternating in one process, device events; medians",
                   "device": torch.cuda.get_device_name(0), "library": nat.lib().gfc_version().decode(),
                   "hbm_peak_bytes_per_second": HBM_PEAK, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
