"""CPU restatement (torch + numpy) of what the posed-image reader computes -- helpers, no tests.

The reference's `datasets/posed_images.py` cannot be imported here (cv2, kornia and h5py are absent), so the reader and
the resample kernel are pinned to this text:
  * crop, then `F.interpolate(mode="nearest" | "area")` -- torch's own operators;
  * kornia's blur before a down-scale (kernel from `oracle.preprocess.gaussian_kernel1d`, reflect padding, horizontal
    pass then vertical, as `oracle.preprocess.kornia_resize`), whatever the interpolation mode;
  * `np.unpackbits` for the packed specular masks;
  * the item dictionary of `_read_view` / `__getitem__` (posed_images.py:219-302) built from the same files;
  * a writer of a tiny dataset directory (nothing of it is committed).
"""
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import preprocess as opp  # noqa: E402

# (h, w) -> (oh, ow) of the kernel tests; the sixth through the crop (left, top, width, height).  At the first six
# the float64 evaluation of torch's `nearest` rule gives torch's indices everywhere (dst * in / out is never close to
# an integer there); the seventh is the smallest found where the fp32 and float64 rules part on both axes.
SHAPES = [((37, 53), (16, 23), None), ((33, 47), (61, 90), None), ((7, 5), (3, 2), None), ((29, 31), (29, 17), None),
          ((9, 70), (1, 1), None), ((61, 53), (17, 21), (5, 3, 40, 30)), ((26, 30), (22, 22), None)]


def window(hw, crop):
    return (0, 0, hw[1], hw[0]) if crop is None else tuple(crop)


def crop_plane(x, crop):
    """x [..., H, W]; crop (left, top, width, height) or None."""
    if crop is None:
        return x
    left, top, cw, ch = crop
    return x[..., top: top + ch, left: left + cw]


def blur(x, size):
    """kornia's antialias blur of x [C,H,W] before a resize to `size` (identity unless some axis is down-scaled)."""
    h, w = x.shape[-2:]
    factors = (h / size[0], w / size[1])
    if max(factors) <= 1:
        return x
    sig = (max((factors[0] - 1.0) / 2.0, 0.001), max((factors[1] - 1.0) / 2.0, 0.001))
    ks = [int(max(2.0 * 2 * sig[0], 3)), int(max(2.0 * 2 * sig[1], 3))]
    ks = [k + 1 if k % 2 == 0 else k for k in ks]
    c = x.shape[0]
    ky, kx = opp.gaussian_kernel1d(ks[0], sig[0]), opp.gaussian_kernel1d(ks[1], sig[1])
    xp = F.pad(x[None], (ks[1] // 2, ks[1] // 2, ks[0] // 2, ks[0] // 2), mode="reflect")
    xp = F.conv2d(xp, kx.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)   # horizontal
    return F.conv2d(xp, ky.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)[0]  # vertical


def resample(x, size, mode, crop=None, antialias=False):
    """x float [C,H,W] -> [C,oh,ow]: crop, kornia's blur (antialias), F.interpolate."""
    x = crop_plane(x, crop)
    if tuple(x.shape[-2:]) == tuple(size):
        return x  # kornia's resize returns its input
    if antialias:
        x = blur(x, size)
    return F.interpolate(x[None], size=tuple(size), mode=mode)[0]


def area_f64(x, size, crop=None):
    """Float64 box means of adaptive average pooling, and the largest box of the shape."""
    x = crop_plane(x, crop).double()
    h, w = x.shape[-2:]
    oh, ow = size
    out = torch.empty(x.shape[:-2] + (oh, ow), dtype=torch.float64)
    biggest = 0
    for i in range(oh):
        y0, y1 = (i * h) // oh, -((-(i + 1) * h) // oh)
        for j in range(ow):
            x0, x1 = (j * w) // ow, -((-(j + 1) * w) // ow)
            out[..., i, j] = x[..., y0:y1, x0:x1].mean((-2, -1))
            biggest = max(biggest, (y1 - y0) * (x1 - x0))
    return out, biggest


def unpack(packed, hw):
    return torch.from_numpy(np.unpackbits(np.asarray(packed), count=hw[0] * hw[1]).reshape(hw).astype(bool))


def nearest_index(n_in, n_out, rule):
    """Source indices of an axis under torch's legacy `nearest` ("legacy": fp32 scale, floor(dst * scale)), under
    `nearest-exact` ("exact": floor((dst + 0.5) * scale)) and under the legacy rule evaluated in float64 ("f64")."""
    dst = np.arange(n_out)
    if rule == "legacy":
        scale = np.float32(n_in) / np.float32(n_out)
        idx = np.floor(dst.astype(np.float32) * scale).astype(np.int64)
    elif rule == "exact":
        scale = np.float32(n_in) / np.float32(n_out)
        idx = np.floor((dst.astype(np.float32) + np.float32(0.5)) * scale).astype(np.int64)
    else:
        idx = np.floor(dst.astype(np.float64) * (n_in / n_out)).astype(np.int64)
    return np.minimum(idx, n_in - 1)


ENDO_TARGET, ENDO_FIRST = (512, 672), (0, 35, 540, 675)  # (h, w); (top, left, h, w)


def endomapper_window(h, w):
    """image.py:77-103 as (left, top, width, height)."""
    if (h, w) == ENDO_TARGET:
        return 0, 0, w, h
    top, left, ch, cw = ENDO_FIRST
    if h < ch or w < left + cw:
        raise ValueError(f"Image too small for Endomapper dense crop: {(h, w)}.")
    return left + (cw - ENDO_TARGET[1]) // 2, top + (ch - ENDO_TARGET[0]) // 2, ENDO_TARGET[1], ENDO_TARGET[0]


# ---------------------------------------------------------------- a tiny dataset directory ----------------------------

def _texture(rng, h, w, c=3):
    base = torch.from_numpy(rng.random((1, c, h // 8 + 2, w // 8 + 2)).astype(np.float32))
    img = F.interpolate(base, size=(h, w), mode="bicubic", align_corners=False)[0]
    img = (img + 0.15 * torch.from_numpy(rng.random((1, h, w)).astype(np.float32))).clamp(0, 1)  # corners to detect
    return (img * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def _rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def write_dataset(data_root, scene, hw, n_images, pairs, model="PINHOLE", with_scene_info=False, seed=0, block=16,
                  seq="seq_000"):
    """<data_root>/<scene>/{images,depths}/<seq>/img<i>.{png,npz}, views.txt, pairs.txt (index pairs `pairs`), and with
    `with_scene_info` the fork's <data_root>/endomapper_dense/scene_info/<seq>.npz (depth scales, specular-mask paths: the
    first with the `endomapper_dense/` prefix the reader strips, the others without) plus the packed mask files.
    Depth: >= 0.5 or exactly 0 in `block` x `block` blocks, stored with a `mask` that zeroes further blocks.
    Returns the image names."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    h, w = hw
    root = Path(data_root) / scene
    (root / "images" / seq).mkdir(parents=True, exist_ok=True)
    (root / "depths" / seq).mkdir(parents=True, exist_ok=True)
    names, lines, mask_paths, scales = [], [], [], []
    base = _texture(rng, h + 32, w + 32)
    for i in range(n_images):
        name = f"{seq}/img{i}.png"
        names.append(name)
        oy, ox = (4 * i) % 29, (6 * i) % 31  # every image another crop of one canvas: true correspondences exist
        Image.fromarray(base[oy: oy + h, ox: ox + w]).save(root / "images" / name)
        bh, bw = -(-h // block), -(-w // block)
        keep = np.kron(rng.random((bh, bw)) > 0.25, np.ones((block, block), bool))[:h, :w]
        depth = (0.5 + 4.5 * rng.random((h, w))).astype(np.float32)
        depth[np.kron(rng.random((bh, bw)) > 0.85, np.ones((block, block), bool))[:h, :w]] = 0.0
        np.savez(root / "depths" / seq / f"img{i}.npz", depth=depth, mask=keep)
        R, t = _rotation(rng, 0.05 * (i + 1)), rng.normal(size=3) * 0.2
        f = 0.9 * w
        params = {"PINHOLE": [f, f * 1.01, w / 2 - 0.5, h / 2 + 0.25], "SIMPLE_RADIAL": [f, w / 2, h / 2, 0.03],
                  "OPENCV_FISHEYE": [f, f * 1.01, w / 2 - 0.5, h / 2 + 0.25, 0.02, -0.003, 0.001, -0.0002]}[model]
        lines.append(" ".join([name, *(repr(float(v)) for v in R.reshape(-1)), *(repr(float(v)) for v in t), model,
                               str(w), str(h), *(repr(float(v)) for v in params)]))
        if with_scene_info:
            rel = f"masks/{seq}/img{i}.npz"
            (root / "masks" / seq).mkdir(parents=True, exist_ok=True)
            mask = np.kron(rng.random((-(-h // 5), -(-w // 7))) > 0.7, np.ones((5, 7), bool))[:h, :w]
            np.savez(root / rel, mask_packbits=np.packbits(mask.reshape(-1)), mask_shape=np.array([h, w]))
            mask_paths.append(("endomapper_dense/" if i == 0 else "") + rel)
            scales.append(0.37 + 0.11 * i)
    (root / "views.txt").write_text("\n".join(lines) + "\n")
    (root / "pairs.txt").write_text("\n".join(f"{names[a]} {names[b]}" for a, b in pairs) + "\n")
    if with_scene_info:
        info = Path(data_root) / "endomapper_dense" / "scene_info"
        info.mkdir(parents=True, exist_ok=True)
        np.savez(info / f"{seq}.npz", image_names=np.array([n.split("/", 1)[1] for n in names]),
                 depth_scale_per_image=np.array(scales, dtype=np.float64), specular_mask_paths=np.array(mask_paths))
    return names


CONF_A = {"root": "", "image_dir": "{scene}/images", "depth_dir": "{scene}/depths", "views": "{scene}/views.txt",
          "view_groups": "{scene}/pairs.txt", "depth_format": "npz", "crop_endomapper_dense": True,
          "depth_scale_scene_info_dir": "endomapper_dense/scene_info", "read_specular_mask": True,
          "specular_scene_info_dir": "endomapper_dense/scene_info", "scene_list": ["endomapper_dense1500"]}
CONF_B = {"root": "", "image_dir": "{scene}/images", "depth_dir": "{scene}/depths", "views": "{scene}/views.txt",
          "view_groups": "{scene}/pairs.txt", "depth_format": "npz", "scene_list": ["megadepth1500"],
          "preprocessing": {"resize": 160, "side": "long"}}


# ---------------------------------------------------------------- the reference's items, restated ---------------------

def _parse(tokens):
    R = torch.from_numpy(np.array(tokens[:9]).astype(np.float32).reshape(3, 3))
    t = torch.from_numpy(np.array(tokens[9:12]).astype(np.float32))
    model, width, height = tokens[12], int(tokens[13]), int(tokens[14])
    p = np.array(tokens[15:]).astype(np.float32)
    if model == "SIMPLE_RADIAL":  # f, cx, cy, k -> fx, fy, cx, cy, k1, k2 = 0
        p = np.array([p[0], p[0], p[1], p[2], p[3], 0.0], dtype=np.float32)
    cam = torch.from_numpy(np.concatenate([np.array([width, height], dtype=np.float32), p]))
    return R, t, cam, model


def read_view(data_root, conf, scene, name, tokens, depth_scales=None, mask_paths=None):
    """`_read_view` (posed_images.py:219-276) on the host, tensors without the batch axis; camera and pose as plain
    tensors (`camera` [2 + 4 + k]: size, f, c, distortion; `R`, `t`)."""
    from PIL import Image

    root = Path(data_root) / conf["root"]
    pre = {"resize": None, "side": "long", "antialias": True, **conf.get("preprocessing", {})}
    R, t, cam, model = _parse(tokens)
    with Image.open(root / conf["image_dir"].format(scene=scene) / name) as im:
        img = opp.numpy_image_to_torch(np.asarray(im.convert("RGB")))
    raw_hw = tuple(img.shape[-2:])
    crop = endomapper_window(*raw_hw) if conf.get("crop_endomapper_dense") else None
    if crop is not None:
        img = crop_plane(img, crop)
        cam = torch.cat([torch.tensor([crop[2], crop[3]], dtype=torch.float32), cam[2:4],
                         cam[4:6] - torch.tensor([float(crop[0]), float(crop[1])]), cam[6:]])
    h, w = img.shape[-2:]
    size = (h, w) if pre["resize"] is None else tuple(opp.get_new_image_size(h, w, pre["resize"], pre["side"]))
    if pre["resize"] is not None:
        img = opp.kornia_resize(img, size, None, pre["antialias"])
    scales = torch.Tensor([img.shape[-1] / w, img.shape[-2] / h])
    view = {"image": img, "scales": scales, "image_size": torch.tensor([float(size[1]), float(size[0])]),
            "original_image_size": torch.tensor([float(w), float(h)]),
            "transform": torch.from_numpy(np.diag([np.float32(scales[0]), np.float32(scales[1]), 1.0])),
            "R": R, "t": t, "model": model, "name": name,
            "camera": torch.cat([cam[0:2] * scales, cam[2:4] * scales, cam[4:6] * scales, cam[6:]])}

    def plane(x):  # preprocessor(x, interpolation="nearest")["image"] after the crop rule of posed_images.py:237-264
        if crop is not None:
            if tuple(x.shape[-2:]) == raw_hw:
                x = crop_plane(x, crop)
            elif tuple(x.shape[-2:]) != (h, w):
                raise ValueError("shape mismatch")
        if pre["resize"] is None:
            return x
        ph, pw = x.shape[-2:]
        return resample(x[None], tuple(opp.get_new_image_size(ph, pw, pre["resize"], pre["side"])), "nearest",
                        antialias=pre["antialias"])[0]

    if conf.get("depth_dir"):
        with np.load(root / conf["depth_dir"].format(scene=scene) / f"{name.split('.')[0]}.npz") as z:
            depth = np.where(z["mask"].astype(bool), z["depth"].astype(np.float32), 0.0).astype(np.float32)
        depth = torch.Tensor(depth)
        if depth_scales is not None:
            depth = depth * float(depth_scales[name])
        view["depth"] = plane(depth)
        view["valid_depth"] = (view["depth"] > 0).float()
    if mask_paths is not None:
        with np.load(mask_paths[name]) as z:
            mask = unpack(z["mask_packbits"], tuple(int(v) for v in z["mask_shape"]))
        view["specular_mask"] = plane(mask.float()) > 0.5
    return view


def read_items(data_root, conf):
    """`__getitem__` (posed_images.py:278-302) for every line of pairs.txt of the conf's one scene."""
    data_root = Path(data_root)
    scene = conf["scene_list"][0]
    root = data_root / conf["root"]
    views = {ln.split(" ")[0]: ln.split(" ")[1:] for ln in (root / conf["views"].format(scene=scene)).read_text().splitlines()}
    depth_scales = mask_paths = None
    if conf.get("depth_scale_scene_info_dir"):
        depth_scales, mask_paths = {}, {}
        for seq in sorted({n.split("/", 1)[0] for n in views}):
            with np.load(data_root / conf["depth_scale_scene_info_dir"] / f"{seq}.npz", allow_pickle=True) as info:
                for i, n in enumerate(info["image_names"].tolist()):
                    depth_scales[f"{seq}/{n}"] = float(info["depth_scale_per_image"].astype(np.float32)[i])
                    p = str(info["specular_mask_paths"][i])
                    mask_paths[f"{seq}/{n}"] = root / scene / (p[len("endomapper_dense/"):] if p.startswith("endomapper_dense/") else p)
    items = []
    for line in (root / conf["view_groups"].format(scene=scene)).read_text().splitlines():
        names = line.split(" ")
        item = {f"view{i}": read_view(data_root, conf, scene, n, views[n], depth_scales, mask_paths)
                for i, n in enumerate(names)}
        item.update(name="/".join(n.replace("/", "-") for n in names), query_name=names[0], references=names[1:],
                    scene=scene, nviews=len(names))
        R0, t0, R1, t1 = item["view0"]["R"], item["view0"]["t"], item["view1"]["R"], item["view1"]["t"]
        R0i, t0i = R0.T, -(R0.T @ t0)
        item["T_0to1"] = (R1 @ R0i, t1 + R1 @ t0i)
        items.append(item)
    return items


def eval_items(items):
    """The restated items in the form `PosePairsPipeline.run_eval` takes (holders of one item)."""
    from glue_factory_colon_amd import geometry

    out = []
    for it in items:
        data = {"name": [it["name"]], "T_0to1": geometry.Pose.from_Rt(it["T_0to1"][0][None], it["T_0to1"][1][None])}
        for v in ("view0", "view1"):
            data[v] = {"camera": geometry.Camera(it[v]["camera"][None], model=it[v]["model"]), "scales": it[v]["scales"][None]}
            if "depth" in it[v]:
                data[v]["depth"] = it[v]["depth"][None]
        out.append(data)
    return out
