"""Time the posed-image path: `posed_images.PosedPairFeeder` alone, `PosePairsPipeline.run`, and the GPU preparation of
image, depth and mask (gfc_preprocess_resample, csrc/preprocess.hip) against the same preparation as torch operations on
the same GPU (slicing, `F.interpolate`, a device-side unpack of the packed mask).

    python tools/posed_feed_bench.py --out profiles [--pairs 256] [--images 32]

Two generated directories (tests/posed_reference.write_dataset; `--pairs` pairs over `--images` distinct files each):
  a     540x720 PNG files, Endomapper-dense crop, depth scales, packed specular masks, no resize;
  area  1200x1800 PNG files, `preprocessing = {resize: 1600, side: long, interpolation: area, antialias: False}`.
Per directory, after the first pairs went once through everything: items/s of the feeder alone (file decoding on the
host included; one pass ended by a device synchronise), pairs/s of `run` with the name-seeded weights (export, then the
evaluation, which reads the list a second time), and the preparation alone on views
that are already decoded and on the device -- kernel path and torch path alternated in ONE process, each pass timed with
device events, medians reported.  Before timing the two paths' outputs are compared.  Writes
<out>/posed_feed_bench.json.  No GPU: an error.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import posed_reference as pr  # noqa: E402
from glue_factory_colon_amd import eval_pose_pairs, posed_images  # noqa: E402
from glue_factory_colon_amd.eval_hpatches import build_model  # noqa: E402
from glue_factory_colon_amd.image_preprocessor import endomapper_dense_window, resample  # noqa: E402

CONF_AREA = {**pr.CONF_B, "preprocessing": {"resize": 1600, "side": "long", "interpolation": "area", "antialias": False}}


def device_views(ds, n, dev):
    """The first n distinct views of the list, decoded, on the device."""
    seen, out = set(), []
    for scene, *names in ds.items:
        for name in names:
            if name not in seen and len(out) < n:
                seen.add(name)
                v = ds.raw_view(scene, name)
                out.append({"image": torch.from_numpy(v["image"]).to(dev), "depth": torch.from_numpy(v["depth"]).to(dev),
                            "scale": v["depth_scale"] or 1.0, "bits_shape": v["specular_mask_shape"],
                            "bits": None if v["specular_mask_packed"] is None else torch.from_numpy(v["specular_mask_packed"]).to(dev)})
    return out


def prepare_kernel(view, win, size, mode):
    img = resample(view["image"], size, mode, crop=win)
    depth, valid = resample(view["depth"], size, "nearest", crop=win, value_scale=view["scale"], want_valid=True)
    mask = None if view["bits"] is None else resample(view["bits"], size, "nearest", crop=win, bits_shape=view["bits_shape"])
    return img, depth, valid, mask


def prepare_torch(view, win, size, mode):
    left, top, cw, ch = win
    img = (view["image"].permute(2, 0, 1).double() / 255.0).float()[:, top: top + ch, left: left + cw]
    depth = (view["depth"] * view["scale"])[top: top + ch, left: left + cw]
    if (ch, cw) != tuple(size):
        img = F.interpolate(img[None], size=size, mode=mode)[0]
        depth = F.interpolate(depth[None, None], size=size, mode="nearest")[0, 0]
    valid = (depth > 0).float()
    mask = None
    if view["bits"] is not None:
        h, w = view["bits_shape"]
        shifts = torch.arange(7, -1, -1, device=view["bits"].device, dtype=torch.uint8)
        bits = ((view["bits"][:, None] >> shifts) & 1).reshape(-1)[: h * w].reshape(h, w).float()
        bits = bits[top: top + ch, left: left + cw]
        if (ch, cw) != tuple(size):
            bits = F.interpolate(bits[None, None], size=size, mode="nearest")[0, 0]
        mask = bits > 0.5
    return img.contiguous(), depth.contiguous(), valid, mask


def timed(fn, views, passes):
    times = []
    for _ in range(passes):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for v in views:
            fn(v)
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return times


def bench_directory(tag, conf, root, args, dev, model):
    ds = posed_images.PosedImages(conf, root)
    res = {"pairs": len(ds)}
    warm = posed_images.PosedImages(conf, root)  # the first pairs once through everything: kernels, model, workspaces
    warm.items = warm.items[:2 * args.pair_batch]
    pipe = eval_pose_pairs.PosePairsPipeline({"estimator": "gfc_amd", "ransac_th": 1.0}, pair_batch=args.pair_batch)
    with tempfile.TemporaryDirectory() as exp:
        pipe.run(exp, model, posed_images.PosedPairFeeder(warm, dev), overwrite=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(1 for _ in posed_images.PosedPairFeeder(ds, dev))
    torch.cuda.synchronize()
    res["feeder_items_per_s"] = n / (time.perf_counter() - t0)
    with tempfile.TemporaryDirectory() as exp:
        t0 = time.perf_counter()
        pipe.run(exp, model, posed_images.PosedPairFeeder(ds, dev), overwrite=True)
        torch.cuda.synchronize()
        res["run_pairs_per_s"] = len(ds) / (time.perf_counter() - t0)
    views = device_views(ds, args.views, dev)
    h, w = views[0]["image"].shape[:2]
    win = endomapper_dense_window(h, w) if conf.get("crop_endomapper_dense") else (0, 0, w, h)
    pre = ds.preprocessor
    size = (win[3], win[2]) if pre.conf["resize"] is None else tuple(pre.get_new_image_size(win[3], win[2]))
    mode = "nearest" if pre.conf["resize"] is None else pre.conf["interpolation"]
    a, b = prepare_kernel(views[0], win, size, mode), prepare_torch(views[0], win, size, mode)
    res["max_abs_difference"] = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b) if x is not None)
    kern, ref = [], []
    timed(lambda v: prepare_kernel(v, win, size, mode), views, 1)
    timed(lambda v: prepare_torch(v, win, size, mode), views, 1)
    for _ in range(args.passes):  # alternated
        kern += timed(lambda v: prepare_kernel(v, win, size, mode), views, 1)
        ref += timed(lambda v: prepare_torch(v, win, size, mode), views, 1)
    res.update(source_hw=[h, w], window=list(win), size=list(size), mode=mode, views=len(views),
               prepare_kernel_ms_per_view=statistics.median(kern) / len(views),
               prepare_torch_ms_per_view=statistics.median(ref) / len(views),
               prepare_kernel_ms_spread=[min(kern) / len(views), max(kern) / len(views)],
               prepare_torch_ms_spread=[min(ref) / len(views), max(ref) / len(views)])
    print(tag, json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--images", type=int, default=32, help="distinct files per directory")
    ap.add_argument("--views", type=int, default=16, help="views of the preparation-only timing")
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--pair_batch", type=int, default=8)
    ap.add_argument("--max_num_keypoints", type=int, default=1024)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("posed_feed_bench needs a GPU: a CPU timing says nothing about the kernels")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    dev = torch.device("cuda", 0)
    pairs = [(i % args.images, (i * 7 + 1 + i // args.images) % args.images) for i in range(args.pairs)]
    pairs = [(a, b if b != a else (b + 1) % args.images) for a, b in pairs]
    model = build_model("synthetic", "synthetic", official=False, max_num_keypoints=args.max_num_keypoints).to(dev)
    out = {"pair_batch": args.pair_batch, "max_num_keypoints": args.max_num_keypoints, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        pr.write_dataset(root, "endomapper_dense1500", (540, 720), args.images, pairs, model="OPENCV_FISHEYE",
                         with_scene_info=True, seed=11)
        out["a"] = bench_directory("a", pr.CONF_A, root, args, dev, model)
    with tempfile.TemporaryDirectory() as root:
        pr.write_dataset(root, "megadepth1500", (1200, 1800), args.images, pairs, model="PINHOLE", seed=12)
        out["area"] = bench_directory("area", CONF_AREA, root, args, dev, model)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "posed_feed_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
