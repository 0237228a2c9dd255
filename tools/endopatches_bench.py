"""Measure the EndoPatches pair generator on the GPU -> profiles/endopatches_feed_bench.json.

    python tools/endopatches_bench.py [--rounds 20] [--sources 36] [--out profiles/endopatches_feed_bench.json]

1. The feeder's warp stage for one pair batch -- 4 resident 540 x 720 x 3 byte sources, per source view 0 + nine
   variants (36 pairs, 40 warps) into 426 x 580 through the window (81, 55, 582, 429), four `gfc_warp_perspective`
   calls -- against THE SAME RULE written as torch gather operations on the same GPU (the yardstick: fp64 positions, the
   1/32-pixel grid, four masked gathers from the converted window, the fp32 weighted sum).  Both forms alternate in one
   process, device events around each, every shape warmed up; the outputs must agree within twice the bound of
   tests/warp_reference.py (two fp32 evaluations of one float64 value).
2. `Endopatches1800Pipeline.run` (SuperPoint-open + LightGlue, name-seeded weights, 1024 key points) on `--sources`
   generated 540 x 720 PNG frames x 9 variants: pairs per second, host clock around the run, which ends in the host copy
   of the last records; the feeder alone (sampling + decode + upload + warp) over the same list, first pass and with
   the sampled homographies kept; the host's homography sampling alone and its PNG decode alone (one thread each).
A run without a GPU fails; nothing here falls back.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from glue_factory_colon_amd import eval_endopatches, eval_hpatches  # noqa: E402
from glue_factory_colon_amd import homographies as hg  # noqa: E402

WINDOW, SIZE, SOURCE_HW = (81, 55, 582, 429), (426, 580), (540, 720)
ENDO = {"difficulty": 0.7, "max_angle": 45, "translation": 1.0, "n_angles": 10, "patch_shape": [580, 426],
        "min_convexity": 0.05}


def torch_warp(src_u8, mats, size, window):
    """The rule of gfc_warp_perspective as torch operations: src_u8 [H,W,C] on the GPU, mats [B,3,3] float64."""
    left, top, cw, ch = window
    win = (src_u8[top: top + ch, left: left + cw].permute(2, 0, 1).to(torch.float32) / 255.0).reshape(src_u8.shape[2], -1)
    oh, ow = size
    x = torch.arange(ow, dtype=torch.float64, device=mats.device)[None, None, :]
    y = torch.arange(oh, dtype=torch.float64, device=mats.device)[None, :, None]
    m = mats.reshape(-1, 9, 1, 1)
    X = m[:, 0] * x + (m[:, 1] * y + m[:, 2])
    Y = m[:, 3] * x + (m[:, 4] * y + m[:, 5])
    Wd = m[:, 6] * x + (m[:, 7] * y + m[:, 8])
    Wd = torch.where(Wd != 0, 32.0 / Wd, torch.zeros_like(Wd))
    qx = torch.round((X * Wd).clamp(-2147483648.0, 2147483647.0)).to(torch.int64)
    qy = torch.round((Y * Wd).clamp(-2147483648.0, 2147483647.0)).to(torch.int64)
    sx, sy = qx >> 5, qy >> 5
    ax, ay = (qx & 31).to(torch.float32) / 32.0, (qy & 31).to(torch.float32) / 32.0

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < cw) & (yy >= 0) & (yy < ch)
        flat = (yy.clamp(0, ch - 1) * cw + xx.clamp(0, cw - 1)).reshape(-1)
        v = win[:, flat].reshape(win.shape[0], *yy.shape).permute(1, 0, 2, 3)
        return v * ok[:, None]

    w00, w01, w10, w11 = (1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay
    t00, t01, t10, t11 = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    out = t00 * w00[:, None] + t01 * w01[:, None] + t10 * w10[:, None] + t11 * w11[:, None]
    max_tap = torch.stack([t00, t01, t10, t11]).abs().amax(dim=(0, 2))
    return out, max_tap


def warp_stage(rounds):
    dev = torch.device("cuda")
    g = np.random.RandomState(0)
    sources = [torch.from_numpy(g.randint(0, 256, (*SOURCE_HW, 3)).astype(np.uint8)).to(dev) for _ in range(4)]
    mats = []
    for s in range(4):  # a scheduled source: view 0 + nine variants, seeds as the schedule numbers them
        views = [hg.sample_view(WINDOW[2:], {**ENDO, "difficulty": 0.0}, np.random.RandomState(0))]
        for k in range(9):
            level = (0.3, 0.5, 0.7)[k // 3]
            views.append(hg.sample_view(WINDOW[2:], {**ENDO, "difficulty": level}, np.random.RandomState(2 * (9 * s + k) + 1)))
        mats.append(torch.from_numpy(np.stack([np.linalg.inv(v["H"]) for v in views])).to(dev))
    index = torch.zeros(10, dtype=torch.int32, device=dev)

    def kernel():
        return [hg.warp_perspective(src, index, m, SIZE, crop=WINDOW) for src, m in zip(sources, mats)]

    def torch_form():
        return [torch_warp(src, m, SIZE, WINDOW)[0] for src, m in zip(sources, mats)]

    worst = 0.0
    for a, (src, m) in zip(kernel(), zip(sources, mats)):  # (also the warm-up of both forms)
        b, max_tap = torch_warp(src, m, SIZE, WINDOW)
        excess = ((a - b).abs() - 2 * 7 * 2.0 ** -24 * max_tap[:, None]).max().item()
        worst = max(worst, excess)
        assert excess <= 0, f"kernel and torch form differ by more than twice the bound: excess {excess}"
    torch_form()
    times = {"kernel": [], "torch": []}
    for _ in range(rounds):
        for name, fn in (("kernel", kernel), ("torch", torch_form)):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(5):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / 5)
    out_bytes, in_bytes = 40 * 3 * SIZE[0] * SIZE[1] * 4, 4 * SOURCE_HW[0] * SOURCE_HW[1] * 3
    k_ms, t_ms = float(np.median(times["kernel"])), float(np.median(times["torch"]))
    return {"pairs": 36, "warps": 40, "calls": 4, "source_hw": list(SOURCE_HW), "window": list(WINDOW), "size": list(SIZE),
            "kernel_ms_per_batch": k_ms, "torch_ms_per_batch": t_ms,
            "kernel_ms_spread": [float(min(times["kernel"])), float(max(times["kernel"]))],
            "torch_ms_spread": [float(min(times["torch"])), float(max(times["torch"]))],
            "kernel_pairs_per_s": 36 / (k_ms * 1e-3), "torch_pairs_per_s": 36 / (t_ms * 1e-3),
            "kernel_bytes_moved_GB_per_s": (out_bytes + in_bytes) / (k_ms * 1e-3) / 1e9,
            "largest_excess_over_twice_the_bound": worst, "rounds": rounds}


def make_frames(root, n):
    from PIL import Image

    h, w = SOURCE_HW
    yy, xx = np.mgrid[0:h, 0:w]
    for split in ("train", "val", "test"):
        os.makedirs(os.path.join(root, "frames", split), exist_ok=True)
    for k in range(n):
        g = np.random.RandomState(k)
        base = np.stack([127 + 100 * np.sin(xx / (9.0 + c + k % 5)) * np.cos(yy / (7.0 + c)) for c in range(3)], -1)
        img = np.clip(base + g.randint(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "frames", "test", f"Seq_{k % 2:03d}_{k:06d}.png"))
    for split in ("train", "val"):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(os.path.join(root, "frames", split, "Seq_009_000000.png"))


def run_stage(n_sources):
    with tempfile.TemporaryDirectory() as root:
        make_frames(root, n_sources)
        conf = {"data_dir": "frames", "test_size": 9 * n_sources, "test_sequences": ["Seq_000", "Seq_001"],
                "test_source_dir": None, "photometric": {"name": "identity"}}
        pipe = eval_endopatches.Endopatches1800Pipeline(conf, data_root=root, pair_batch=36)
        ds = pipe.dataset
        n = len(ds)
        model = eval_hpatches.build_model("synthetic", "synthetic", official=False, max_num_keypoints=1024).cuda()
        pipe.run(os.path.join(root, "warm"), model)  # every shape of the timed window, once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        summaries, _ = pipe.run(os.path.join(root, "exp"), model)
        torch.cuda.synchronize()
        run_s = time.perf_counter() - t0
        # the feeder alone: on a fresh list (its homographies still to be drawn on the host), then with them kept
        fresh = eval_endopatches.Endopatches1800Pipeline(conf, data_root=root, pair_batch=36).dataset
        feed = []
        for _ in range(2):
            t0 = time.perf_counter()
            for _ in fresh.feeder(batch=36):
                pass
            torch.cuda.synchronize()
            feed.append(time.perf_counter() - t0)
        cold = eval_endopatches.Endopatches1800Pipeline(conf, data_root=root, pair_batch=36).dataset
        t0 = time.perf_counter()
        for i in range(n):
            cold.geometry(i, SOURCE_HW)
        geometry_s = time.perf_counter() - t0
        names = list(dict.fromkeys(ds.source_name(i) for i in range(n)))
        t0 = time.perf_counter()
        for name in names:
            ds.read_source(name)
        decode_s = time.perf_counter() - t0
        file_bytes = sum(os.path.getsize(os.path.join(root, "frames", "test", nm)) for nm in names)
    return {"sources": n_sources, "pairs": n, "max_num_keypoints": 1024, "pair_batch": 36, "run_pairs_per_s": n / run_s,
            "feeder_pairs_per_s_first_pass": n / feed[0], "feeder_pairs_per_s_homographies_kept": n / feed[1],
            "host_homography_sampling_pairs_per_s_one_thread": n / geometry_s, "decode_sources_per_s_one_thread": len(names) / decode_s,
            "decode_pairs_per_s_one_thread": n / decode_s, "png_bytes_per_source": file_bytes / len(names),
            "mean_num_keypoints": summaries["mean_num_keypoints"], "mean_num_matches": summaries["mean_num_matches"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sources", type=int, default=36)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "endopatches_feed_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16)))
    result = {"device": torch.cuda.get_device_name(0), "warp_stage": warp_stage(args.rounds), "run": run_stage(args.sources)}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
