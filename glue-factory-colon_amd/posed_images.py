"""Posed-image directories -> loader items on the GPU -- counterpart of `gluefactory.datasets.posed_images`
(reference gluefactory/datasets/posed_images.py:35-305), the dataset behind the megadepth1500 and
endomapper_dense1500 benchmarks:

    <root>/<scene>/<image_dir>/   <depth_dir>/   views.txt   pairs.txt   [extra_data.txt]

`PosedImages` reads the lists (same configuration keys, same existence asserts, per-image depth scales and specular-mask
paths from the fork's scene-info archives) and `raw_item(i)` decodes one group of views ON THE HOST: uint8 images
(`image_io.read_image`), float32 depth, the specular mask still as `numpy.packbits` bytes, parsed poses and cameras.
`PosedPairFeeder` turns raw items into the batch-1 items the reference's DataLoader collates, with every pixel
operation on the GPU: the bytes are copied as they are and ONE `gfc_preprocess_resample` launch per plane applies the
Endomapper-dense crop window, the `/255` conversion, the depth scale, the `nearest` / `area` resample (with kornia's
blur when it down-scales), `valid_depth` and the bit unpacking -- no cropped or unpacked copy is made on the host.  An
image preprocessed with the default `bilinear` goes through `gfc_preprocess_resize`.

Unpinned (kornia, cv2 and h5py are absent, so the reference's class cannot be imported): the reader as a whole is
checked against a restatement (tests/posed_reference.py), not the reference's output; kornia's blur-then-nearest of a
resized depth map is a restatement too; JPEG and 16-bit PNG files are decoded by Pillow, not OpenCV.
"""
import ast
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import geometry, image_io
from .base_model import merge
from .image_preprocessor import (DEFAULT_CONF as PREPROCESSING_DEFAULT_CONF, RESAMPLE_MODES, ImagePreprocessor,
                                 endomapper_dense_window, resample, resize)

DEFAULT_CONF = {
    "root": "???",
    "image_dir": "???",
    "depth_dir": None,  # optional
    "crop_endomapper_dense": False,
    "depth_scale_scene_info_dir": None,
    "read_specular_mask": False,
    "specular_scene_info_dir": None,
    "views": "???",
    "extra_data": None,  # text file with extra data
    "extra_keys": [],
    "view_groups": None,
    "depth_format": "h5",
    "scene_list": None,
    "preprocessing": PREPROCESSING_DEFAULT_CONF,
    "batch_size": 1,
}


def names_to_pair(name0, name1, separator="/"):
    return separator.join((name0.replace("/", "-"), name1.replace("/", "-")))


def parse_pose_camera(tokens):
    """The tokens of a views.txt line after the image name: R (9, row-major), t (3), camera model, width, height,
    parameters -> (Pose, Camera), both float32 (posed_images.py:39-50)."""
    pose = geometry.Pose.from_Rt(torch.from_numpy(np.array(tokens[:9]).astype(np.float32).reshape(3, 3)),
                                 torch.from_numpy(np.array(tokens[9:12]).astype(np.float32)))
    camera = geometry.Camera.from_colmap({"model": tokens[12], "width": int(tokens[13]), "height": int(tokens[14]),
                                          "params": np.array(tokens[15:]).astype(np.float32)})
    return pose, camera.float()


def load_depth(path, dformat):
    """-> float32 [H,W] array (posed_images.py:53-72)."""
    if dformat == "png":  # 16-bit, 1/256 units
        from PIL import Image
        with Image.open(str(path)) as im:
            return np.asarray(im).astype(np.float32) / 256
    if dformat == "h5":
        try:
            import h5py
        except ImportError:
            from . import _hdf5
            return _hdf5.read_dataset(path, "/depth").astype(np.float32, copy=False)  # Hdf5Unavailable without the library
        with h5py.File(str(path), "r") as f:
            return f["/depth"].__array__().astype(np.float32, copy=False)
    if dformat == "npz":
        with np.load(str(path)) as data:
            depth = data["depth"].astype(np.float32, copy=False)
            if "mask" in data:
                mask = data["mask"].astype(bool, copy=False)
                if depth.shape != mask.shape:
                    raise ValueError(f"Depth/mask shape mismatch in {path}")
                depth = np.where(mask, depth, 0.0).astype(np.float32, copy=False)
        return depth
    raise ValueError(dformat)


def load_specular_mask(path):
    """-> (packed bytes as numpy.packbits made them of the flattened mask, (h, w)); the bits are unpacked by the
    resample kernel (posed_images.py:75-82 unpacks on the host)."""
    with np.load(str(path)) as data:
        if "mask_packbits" not in data or "mask_shape" not in data:
            raise KeyError(f"Specular mask array not found in {path}.")
        packed = np.ascontiguousarray(data["mask_packbits"], dtype=np.uint8).reshape(-1)
        h, w = data["mask_shape"].astype(np.int64).tolist()
    if packed.size != (h * w + 7) // 8:
        raise ValueError(f"Specular mask of {packed.size} bytes for shape {(h, w)} in {path}.")
    return packed, (int(h), int(w))


def _seq_maps(views):
    return sorted({str(name).split("/", 1)[0] for scene_views in views.values() for name in scene_views})


class PosedImages:
    default_conf = DEFAULT_CONF

    def __init__(self, conf, data_root="."):
        conf = dict(conf or {})
        self.conf = merge({k: v for k, v in DEFAULT_CONF.items() if k != "preprocessing"},
                          {k: v for k, v in conf.items() if k != "preprocessing"})
        for key in ("root", "image_dir", "views"):
            if self.conf[key] == "???":
                raise KeyError(f"posed_images: missing mandatory key {key!r}")
        self.preprocessor = ImagePreprocessor(conf.get("preprocessing"))
        self.conf["preprocessing"] = self.preprocessor.conf
        data_root = Path(data_root)
        self.root = data_root / self.conf["root"]
        assert self.root.exists(), self.root
        scene_list = self.conf["scene_list"]
        if isinstance(scene_list, str):
            self.scenes = (self.root / scene_list).read_text().rstrip("\n").split("\n")
        elif scene_list is not None:
            self.scenes = list(scene_list)
        else:
            self.scenes = sorted(s.name for s in self.root.glob("*"))
        self.views, self.extra_data, self.depth_scales, self.specular_masks = {}, {}, {}, {}
        self.items = []
        for scene in self.scenes:
            with open(str(self.root / self.conf["views"].format(scene=scene)), "r") as f:
                self.views[scene] = {line.rstrip().split(" ")[0]: line.rstrip().split(" ")[1:] for line in f}
            for imname in self.views[scene]:
                impath = self.get_image_path(scene, imname)
                assert impath.exists(), impath
                if self.conf["depth_dir"]:
                    depthpath = self.get_depth_path(scene, imname)
                    assert depthpath.exists(), depthpath
            if self.conf["extra_data"]:
                with open(str(self.root / self.conf["extra_data"].format(scene=scene)), "r") as f:
                    self.extra_data[scene] = {line.rstrip().split(" ")[0]: [ast.literal_eval(x) for x in line.rstrip().split(" ")[1:]]
                                              for line in f if not line.startswith("#")}
                for k in self.extra_data[scene]:
                    assert k in self.views[scene]
            if self.conf["view_groups"] is None:
                self.items += [[scene, imname] for imname in self.views[scene]]
            else:
                groups = (self.root / self.conf["view_groups"].format(scene=scene)).read_text().rstrip("\n").split("\n")
                self.items += [[scene] + p.split(" ") for p in groups]
        if self.conf["depth_scale_scene_info_dir"]:
            info_dir = data_root / self.conf["depth_scale_scene_info_dir"]
            for seq_map in _seq_maps(self.views):
                with np.load(str(info_dir / f"{seq_map}.npz"), allow_pickle=True) as info:
                    image_names = [str(x) for x in info["image_names"].tolist()]
                    scales = info["depth_scale_per_image"].astype(np.float32, copy=False)
                self.depth_scales.update({f"{seq_map}/{n}": float(scales[i]) for i, n in enumerate(image_names)})
        if self.conf["read_specular_mask"]:
            if not self.conf["specular_scene_info_dir"]:
                raise ValueError("specular_scene_info_dir must be set when read_specular_mask is True.")
            info_dir = data_root / self.conf["specular_scene_info_dir"]
            for seq_map in _seq_maps(self.views):
                with np.load(str(info_dir / f"{seq_map}.npz"), allow_pickle=True) as info:
                    image_names = [str(x) for x in info["image_names"].tolist()]
                    specular_paths = [str(x) for x in info["specular_mask_paths"].tolist()]
                # (as the reference: relative to the LAST scene's directory)
                self.specular_masks.update({
                    f"{seq_map}/{n}": self.root / scene / (Path(p).relative_to("endomapper_dense")
                                                           if Path(p).parts[:1] == ("endomapper_dense",) else Path(p))
                    for n, p in zip(image_names, specular_paths)})

    def get_image_path(self, scene, img_name):
        return self.root / self.conf["image_dir"].format(scene=scene) / img_name

    def get_depth_path(self, scene, img_name):
        return self.root / self.conf["depth_dir"].format(scene=scene) / f"{img_name.split('.')[0]}.{self.conf['depth_format']}"

    def __len__(self):
        return len(self.items)

    def raw_view(self, scene, name):
        """One view, decoded on the host; nothing is cropped, scaled, unpacked or resized here."""
        pose, camera = parse_pose_camera(self.views[scene][name])
        view = {"name": name, "image": image_io.read_image(self.get_image_path(scene, name)), "T_w2cam": pose,
                "camera": camera, "depth": None, "depth_scale": None, "specular_mask_packed": None,
                "specular_mask_shape": None, "extra": {}}
        if self.conf["depth_dir"]:
            view["depth"] = load_depth(self.get_depth_path(scene, name), self.conf["depth_format"])
            if self.conf["depth_scale_scene_info_dir"]:
                view["depth_scale"] = float(self.depth_scales[name])
        if self.conf["read_specular_mask"]:
            view["specular_mask_path"] = self.specular_masks[name]
            view["specular_mask_packed"], view["specular_mask_shape"] = load_specular_mask(self.specular_masks[name])
        if self.conf["extra_data"]:
            view["extra"] = dict(zip(self.conf["extra_keys"], self.extra_data[scene][name]))
        return view

    def raw_item(self, i):
        scene, *names = self.items[i]
        return {"scene": scene, "names": names, "views": [self.raw_view(scene, n) for n in names],
                "depth_paths": [self.get_depth_path(scene, n) if self.conf["depth_dir"] else None for n in names]}

    def feeder(self, device="cuda", num_workers=4):
        return PosedPairFeeder(self, device, num_workers=num_workers)


class PosedPairFeeder:
    """Iterable of the batch-1 loader items of a `PosedImages` list, tensors on the GPU.  Per view: `image` [1,C,h,w],
    `depth`, `valid_depth` [1,h,w] float32 and `specular_mask` [1,h,w] bool when the dataset has them, `camera`
    (`Camera.crop(left_top, (w, h))` then `.scale(scales)`, posed_images.py:223-228) and `T_w2cam` as holders of one item
    on the host, `scales` / `image_size` / `original_image_size` [1,2] float32 on the device and `transform` [1,3,3] on
    the host as `HostImageFeeder` yields them, `name` and the `extra_keys`.  At the top level `name`, `query_name`,
    `references`, `scene` (strings as the DataLoader collates them: lists of one), `nviews` and `T_0to{i}`.

    `num_workers` reader threads decode the files of the next items (Pillow and numpy release the interpreter lock while
    they read and inflate); the host arrays of `depth` items are copied from pinned memory on a copy stream ahead of the
    consumer; the kernels run on the consumer's stream behind the copies' event."""

    def __init__(self, dataset, device="cuda", depth=4, num_workers=4):
        self.dataset, self.depth, self.num_workers = dataset, max(1, int(depth)), max(0, int(num_workers))
        self.pre = dataset.preprocessor
        if self.pre.conf["square_pad"]:
            raise NotImplementedError("square_pad on the posed-image path")
        self.device = torch.device(device if device != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self.crop = bool(dataset.conf["crop_endomapper_dense"])

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        return self._iterate(self._raws(range(len(self.dataset))))

    def _raws(self, indices):
        """`dataset.raw_item` of `indices` in order, up to 2 x num_workers items decoded ahead by the reader threads."""
        if self.num_workers == 0:
            yield from (self.dataset.raw_item(i) for i in indices)
            return
        with ThreadPoolExecutor(self.num_workers) as pool:
            ahead = deque()
            for i in indices:
                ahead.append(pool.submit(self.dataset.raw_item, i))
                if len(ahead) >= 2 * self.num_workers:
                    yield ahead.popleft().result()
            while ahead:
                yield ahead.popleft().result()

    def shard(self, rank, world, group=1):
        """(index, item) of this rank's round-robin share (sharding.round_robin_shard); only its files are read."""
        from .sharding import round_robin_shard
        idx = list(round_robin_shard(len(self.dataset), int(rank), int(world), max(1, int(group))))
        return zip(idx, self._iterate(self._raws(idx)))

    def _iterate(self, raws):
        copy_stream = torch.cuda.Stream(self.device)
        pending = deque()
        it = iter(raws)
        exhausted = False
        while True:
            while not exhausted and len(pending) < self.depth:
                try:
                    pending.append(self._stage(next(it), copy_stream))
                except StopIteration:
                    exhausted = True
            if not pending:
                return
            yield self._finish(pending.popleft())

    def _window(self, shape_hw, raw_hw, img_hw, what):
        """The window of a depth map / mask of `shape_hw` (posed_images.py:237-264): the image's crop when it has the
        raw image's shape, all of it when it has the cropped image's, else the reference's ValueError."""
        h, w = shape_hw
        if not self.crop:
            return 0, 0, w, h
        if tuple(shape_hw) == tuple(raw_hw):
            return endomapper_dense_window(h, w)
        if tuple(shape_hw) != tuple(img_hw):
            raise ValueError(f"{what}: {tuple(shape_hw)} vs image {tuple(img_hw)}.")
        return 0, 0, w, h

    def _stage(self, raw, copy_stream):
        """Checks the shapes and issues the host-to-device copies of one item on the copy stream."""
        staged = []
        with torch.cuda.stream(copy_stream):
            for view, depth_path in zip(raw["views"], raw["depth_paths"]):
                img = view["image"]
                raw_hw = (int(img.shape[0]), int(img.shape[1]))
                win = endomapper_dense_window(*raw_hw) if self.crop else (0, 0, raw_hw[1], raw_hw[0])
                img_hw = (win[3], win[2])
                rec = {"win": win, "dev": self._h2d(img)}
                if view["depth"] is not None:
                    d = view["depth"]
                    if d.ndim != 2:
                        raise ValueError(f"Depth of shape {d.shape} in {depth_path}")
                    rec["dwin"] = self._window(d.shape, raw_hw, img_hw, f"Depth shape mismatch for {depth_path}")
                    rec["ddev"] = self._h2d(d)
                if view["specular_mask_packed"] is not None:
                    rec["mwin"] = self._window(view["specular_mask_shape"], raw_hw, img_hw,
                                               f"Specular mask shape mismatch for {view['specular_mask_path']}")
                    rec["mdev"] = self._h2d(view["specular_mask_packed"])
                staged.append(rec)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return raw, staged, done

    def _h2d(self, array):
        return torch.from_numpy(np.ascontiguousarray(array)).pin_memory().to(self.device, non_blocking=True)

    def _finish(self, staged):
        raw, recs, done = staged
        main = torch.cuda.current_stream(self.device)
        main.wait_event(done)
        conf = self.pre.conf
        item = {}
        for i, (view, rec) in enumerate(zip(raw["views"], recs)):
            left, top, cw, ch = rec["win"]
            size = (ch, cw) if conf["resize"] is None else tuple(self.pre.get_new_image_size(ch, cw))
            dev = rec["dev"]
            dev.record_stream(main)
            mode = conf["interpolation"]
            if conf["resize"] is None:
                img = resample(dev, size, "nearest", crop=rec["win"])  # conversion (+ crop) only
            elif mode in RESAMPLE_MODES:
                if conf["align_corners"] is not None:
                    raise ValueError(f"align_corners option can only be set with the interpolating modes (got {mode!r})")
                img = resample(dev, size, mode, crop=rec["win"], antialias=conf["antialias"])
            elif mode == "bilinear":
                if (left, top, cw, ch) != (0, 0, dev.shape[1], dev.shape[0]):
                    dev = dev[top: top + ch, left: left + cw].contiguous()  # (on the device)
                img = resize(dev, size, conf["align_corners"], conf["antialias"])
            else:
                raise NotImplementedError(f"interpolation {mode!r}: 'bilinear', 'nearest' and 'area' are built")
            scales = torch.tensor([size[1] / cw, size[0] / ch], dtype=torch.float32)
            meta = torch.tensor([size[1] / cw, size[0] / ch, size[1], size[0], cw, ch], dtype=torch.float32)
            meta = meta.to(self.device, non_blocking=True)
            camera = view["camera"]
            if self.crop:
                camera = camera.crop((float(left), float(top)), (cw, ch))
            out = {"image": img[None], "scales": meta[0:2][None], "image_size": meta[2:4][None],
                   "original_image_size": meta[4:6][None],
                   "transform": torch.from_numpy(np.diag([np.float32(size[1] / cw), np.float32(size[0] / ch), 1.0]))[None],
                   "T_w2cam": view["T_w2cam"][None], "camera": camera.scale(scales)[None], "name": [view["name"]]}
            if "ddev" in rec:
                out["depth"], out["valid_depth"] = self._plane(rec["ddev"], rec["dwin"], size, main, want_valid=True,
                                                               value_scale=view["depth_scale"] or 1.0)
            if "mdev" in rec:
                out["specular_mask"] = self._plane(rec["mdev"], rec["mwin"], size, main,
                                                   bits_shape=view["specular_mask_shape"])
            for k, v in view["extra"].items():
                out[k] = [v] if isinstance(v, str) else torch.as_tensor([v])
            item[f"view{i}"] = out
        names = raw["names"]
        item.update({"name": ["/".join(n.replace("/", "-") for n in names)], "query_name": [names[0]],
                     "references": [[n] for n in names[1:]], "scene": [raw["scene"]], "nviews": torch.tensor([len(names)])})
        for i in range(1, len(names)):
            item[f"T_0to{i}"] = item[f"view{i}"]["T_w2cam"] @ item["view0"]["T_w2cam"].inv()
        return item

    def _plane(self, dev, win, size, main, **kwargs):
        """A depth map or mask through the preprocessor with "nearest" (posed_images.py:245-248,265-268): its own
        target size from its own window, which must be the image's."""
        dev.record_stream(main)
        conf = self.pre.conf
        own = (win[3], win[2]) if conf["resize"] is None else tuple(self.pre.get_new_image_size(win[3], win[2]))
        assert tuple(own) == tuple(size), (own, size)
        if conf["resize"] is not None and conf["align_corners"] is not None:
            raise ValueError("align_corners option can only be set with the interpolating modes (got 'nearest')")
        out = resample(dev, size, "nearest", crop=win, antialias=conf["resize"] is not None and conf["antialias"], **kwargs)
        return (out[0][None], out[1][None]) if isinstance(out, tuple) else out[None]
