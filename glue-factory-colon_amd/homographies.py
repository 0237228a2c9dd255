"""Homography pairs generated on the GPU -- counterpart of `gluefactory.datasets.homographies` (reference
gluefactory/datasets/homographies.py: `HomographyDataset` / `_Dataset`) and of the sampler it draws from
(gluefactory/geometry/homography.py:17-128), the data side of the fork's EndoPatches1800 benchmark
(gluefactory/eval/endopatches1800.py).

  * the sampler (`create_center_patch`, `check_convex`, `sample_homography_corners`, `compute_homography`): numpy,
    float64, the reference's operations in the reference's order, so that a seed yields the reference's homography
    (tests/golden/endopatches_homographies.npz holds the reference's own draws).  A seeded view draws from
    `numpy.random.RandomState(seed)`: the stream `fork_rng(seed)` gives the reference's global generator.
  * `HomographyPairs`: the reference's configuration keys, image lists, test schedule (sources x homography levels x
    photometric levels, one seed per item), saved-benchmark layout (`source_names.txt`, `<dir>/attribs.txt`,
    `<dir>/source.png`, `<dir>/h<i>_p<j>.png`, `<dir>/H_<dir>_h<i>_p<j>.txt`) and errors.
  * `warp_perspective`: `gfc_warp_perspective` (csrc/warp.hip) -- where the reference calls cv2.warpPerspective on the
    host twice per pair (homographies.py:37-44), ONE launch warps every view of every item of a source.  UNPINNED:
    OpenCV is absent here; the rule restates its INTER_LINEAR / BORDER_CONSTANT 0 arithmetic and is held to the float64
    restatement of tests/warp_reference.py, not to OpenCV's output.  The destination -> source matrix is
    `numpy.linalg.inv(H)` in float64 (OpenCV inverts with its own 3x3 routine: last-bit differences, unpinned too).
  * `HomographyPairFeeder`: a source is decoded once on the host, uploaded once, and all its views of a batch come out
    of one kernel call; in a scheduled benchmark view 0 of a source's items is ONE image (its difficulty is 0, so every
    draw is multiplied by zero whatever the seed) and is declared shared through `view_key`.

Photometric augmentation: `identity` only.  The reference's `lg` and `dark` are albumentations pipelines (absent here,
seeded through their own generator): generating with them raises NotImplementedError; a saved benchmark
(`read_dataset_from_disk`) carries their result in its files and is read whatever the photometric key says.
"""
import os
from pathlib import Path

import numpy as np
import torch

from . import _native as nat
from .base_model import merge
from .image_io import image_size, read_image

# ---- the sampler (gluefactory/geometry/homography.py:17-128) ------------------------------------------------------


def create_center_patch(shape, patch_shape=None):
    """Corners (x, y) of the `patch_shape` rectangle centred in `shape` = (width, height), truncated to integers, in
    the order (left, bottom), (left, top), (right, top), (right, bottom)."""
    width, height = shape
    pwidth, pheight = shape if patch_shape is None else patch_shape
    x0, y0 = int((width - pwidth) / 2), int((height - pheight) / 2)
    x1, y1 = int((width + pwidth) / 2), int((height + pheight) / 2)
    return np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]])


def check_convex(patch, min_convexity=0.05):
    """True when every corner of the polygon [N,2] turns the same way by more than `min_convexity`."""
    n = patch.shape[0]
    for i in range(n):
        (xa, ya), (xb, yb), (xc, yc) = patch[(i - 1) % n], patch[i], patch[(i + 1) % n]
        if (xb - xa) * (yc - yb) - (xc - xb) * (yb - ya) > -min_convexity:
            return False
    return True


def compute_homography(pts1_, pts2_, shape):
    """The homography through four correspondences pts1_ -> pts2_ (each [4,2], scaled by `shape` reversed): the 8 x 8
    direct linear system solved with numpy.linalg.solve, last entry 1.  The system keeps the dtype numpy gives the
    reference's rows (fp32 corners make an fp32 solve), which is part of what a seed yields."""
    scale = np.array(shape[::-1], dtype=np.float32)[None]
    pts1, pts2 = pts1_ * scale, pts2_ * scale
    rows, rhs = [], []
    for p, q in zip(pts1, pts2):
        rows.append([p[0], p[1], 1, 0, 0, 0, -p[0] * q[0], -p[1] * q[0]])
        rows.append([0, 0, 0, p[0], p[1], 1, -p[0] * q[1], -p[1] * q[1]])
        rhs += [q[0], q[1]]
    a_mat = np.stack(rows, axis=0)
    p_mat = np.transpose(np.stack([rhs], axis=0))
    h = np.transpose(np.linalg.solve(a_mat, p_mat))
    return np.reshape(np.concatenate([h, np.ones_like(h[:, :1])], axis=1), [3, 3])


def warp_points(points, homography):
    """points [N,2] through `homography` (not its inverse): homogeneous product, |w| < 1e-8 replaced by 1e-8."""
    pts = np.concatenate([points, np.ones([points.shape[0], 1], dtype=np.float32)], -1)
    warped = np.transpose(np.tensordot(pts, np.transpose(homography[None]), axes=[[1], [0]]), [2, 0, 1])
    warped[np.abs(warped[:, :, 2]) < 1e-8, 2] = 1e-8
    return (warped[:, :, :2] / warped[:, :, 2:])[0]


def sample_homography_corners(shape, patch_shape, difficulty=1.0, translation=0.4, n_angles=10, max_angle=90,
                              min_convexity=0.05, rng=np.random):
    """One random homography image -> patch (homography.py:40-107), `rng` a RandomState or the numpy.random module.
    Draws, in this order: uniform [4,2] corner offsets until the quadrilateral is convex; two shuffles of the candidate
    angles (with n_angles > 0 and difficulty > 0); one uniform translation (with translation > 0).
    -> (H float64 [3,3], the image's corners, those corners through H, patch_shape)."""
    max_angle = max_angle / 180.0 * np.pi
    width, height = shape
    min_pts1 = create_center_patch(shape, (width * (1 - difficulty), height * (1 - difficulty)))
    full = create_center_patch(shape)
    pts2 = create_center_patch(patch_shape)
    scale = min_pts1 - full
    while True:
        pts1 = full + rng.uniform(0.0, 1.0, size=(4, 2)) * scale
        if check_convex(pts1 / np.array(shape), min_convexity):
            break
    pts1 = pts1 - np.mean(pts1, axis=0, keepdims=True)
    pts1 = pts1 + np.mean(min_pts1, axis=0, keepdims=True)
    if n_angles > 0 and difficulty > 0:
        angles = np.linspace(-max_angle * difficulty, max_angle * difficulty, n_angles)
        rng.shuffle(angles)
        rng.shuffle(angles)
        angles = np.concatenate([[0.0], angles], axis=0)
        center = np.mean(pts1, axis=0, keepdims=True)
        rot = np.reshape(np.stack([np.cos(angles), -np.sin(angles), np.sin(angles), np.cos(angles)], axis=1), [-1, 2, 2])
        rotated = np.matmul(np.tile(np.expand_dims(pts1 - center, axis=0), [n_angles + 1, 1, 1]), rot) + center
        for i in range(1, n_angles):  # the reference's range: the candidate 0 (no rotation) and the last are never taken
            inside = rotated[i] / np.array(shape)
            if np.all((inside >= 0.0) & (inside < 1.0)):
                pts1 = rotated[i]
                break
    if translation > 0:
        trans = rng.uniform(-np.min(pts1, axis=0), shape - np.max(pts1, axis=0))[None]
        pts1 += trans * translation * difficulty
    H = compute_homography(pts1, pts2, [1.0, 1.0])
    return H, full, warp_points(full, H), patch_shape


def sample_view(size, homography_conf, rng):
    """`sample_homography` (datasets/homographies.py:37-44) without the pixels: `size` (w, h) of the source image.
    -> {"H": float64 (what the warp uses), "H_": float32, "coords": float32 [4,2], "image_size": float32 [2]}."""
    H, _, coords, _ = sample_homography_corners(tuple(size), **homography_conf, rng=rng)
    return {"H": H, "H_": H.astype(np.float32), "coords": coords.astype(np.float32),
            "image_size": np.array(homography_conf["patch_shape"], dtype=np.float32)}


# ---- the kernel ---------------------------------------------------------------------------------------------------


def warp_perspective(src, src_index, matrices, size, crop=None, gray=False):
    """`gfc_warp_perspective`: B perspective warps in one launch (UNPINNED against OpenCV: module docstring).
    src: uint8 [S,H,W,C] / [H,W,C] / [H,W] decoded images, or float32 [S,C,H,W] / [C,H,W] planes, on the GPU, C 1 or 3;
    src_index: int32 [B] on the GPU (which source each item warps); matrices: float64 [B,3,3] on the GPU, DESTINATION ->
    SOURCE (the inverse of the sampler's H); size (OH, OW); crop (left, top, cw, ch): the window that IS the image
    (default: the whole plane); gray: [B,1,OH,OW] = 0.299 r + 0.587 g + 0.114 b.  -> float32 [B,C,OH,OW]."""
    nat.require_cuda(src, "src")
    if src.dtype == torch.uint8:
        if src.ndim == 2:
            src = src[None, :, :, None]
        elif src.ndim == 3:
            src = src[None]
        kind, (s, h, w, c) = nat.GFC_RS_U8_HWC, src.shape
    elif src.dtype == torch.float32:
        if src.ndim == 3:
            src = src[None]
        kind, (s, c, h, w) = nat.GFC_RS_F32_CHW, src.shape
    else:
        raise ValueError(f"src: uint8 [S,H,W,C] or float32 [S,C,H,W] expected, got {src.dtype}")
    if src.ndim != 4:
        raise ValueError(f"src: 4 dimensions expected, got {tuple(src.shape)}")
    if src_index.dtype != torch.int32 or matrices.dtype != torch.float64:
        raise ValueError("src_index must be int32 and matrices float64")
    b = int(src_index.numel())
    if tuple(matrices.shape) != (b, 3, 3):
        raise ValueError(f"matrices: {(b, 3, 3)} expected, got {tuple(matrices.shape)}")
    left, top, cw, ch = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty((max(b, 0), 1 if gray else c, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=src.device)
    nat.call("gfc_warp_perspective", src.contiguous(), kind, s, c, h, w, left, top, cw, ch, src_index.contiguous(),
             matrices.contiguous(), b, 1 if gray else 0, out, oh, ow)
    return out


# ---- the dataset --------------------------------------------------------------------------------------------------


class HomographyPairs:
    """The reference's `homographies` dataset as a list of pair descriptions (no pixels): `len()`, `meta(i)`,
    `geometry(i)`, `feeder()` (the pixels, on the GPU), `save_dataset()`.  `split` names the image list ("train" /
    "val" / "test"); the test split carries the benchmark schedule or the saved benchmark."""

    default_conf = {
        "data_dir": "revisitop1m", "image_dir": "jpg/", "image_list": "revisitop1m.txt", "check_file_exists": False,
        "glob": ["*.jpg", "*.png", "*.jpeg", "*.JPG", "*.PNG"],
        "train_size": 100, "val_size": 10, "test_size": 0, "shuffle_seed": 0,
        "grayscale": False, "triplet": False, "right_only": False, "left_view_difficulty": None,
        "right_view_difficulty": None, "reseed": False, "seed": 0, "test_seed": 0, "test_sequences": None,
        "test_homography_levels": None, "test_photometric_levels": None, "test_source_dir": None,
        "test_image_list": None, "save_dataset": False, "read_dataset_from_disk": False,
        "saved_dataset_dir": "endopatches1800", "crop_vignette": False, "vignette_crop_coords": None,
        "homography": {"difficulty": 0.8, "translation": 1.0, "max_angle": 60, "n_angles": 10,
                       "patch_shape": [640, 480], "min_convexity": 0.05},
        "photometric": {"name": "dark", "p": 0.75},
        "load_features": {"do": False},
        "pin_memory": True,  # decoded sources in pinned host memory: their copies to the GPU are asynchronous
    }

    def __init__(self, conf=None, data_root=None, split="test"):
        self.conf = conf = merge(self.default_conf, dict(conf or {}))
        self.split = split
        if conf["read_dataset_from_disk"] and conf["test_source_dir"] is not None:
            raise ValueError("test_source_dir and read_dataset_from_disk are mutually exclusive.")
        if conf["triplet"]:
            raise NotImplementedError("triplet: only pairs are generated here")
        if conf["load_features"].get("do"):
            raise NotImplementedError("load_features.do: cached features are not read by this dataset")
        self.data_root = Path(os.environ.get("GFC_DATA_PATH", ".") if data_root is None else data_root)
        data_dir = self.data_root / conf["data_dir"]
        if not data_dir.exists():
            raise FileNotFoundError(data_dir)  # (no download is attempted: the images must be on the machine)
        self.data_dir = data_dir
        self.images = self._image_lists(data_dir)
        self.image_dir = data_dir / split if (data_dir / split).exists() else data_dir / conf["image_dir"]
        self.image_names = list(self.images[split])
        self.items, self.saved_root = None, None
        if split == "test":
            if conf["read_dataset_from_disk"]:
                self.saved_root = self.data_root / conf["saved_dataset_dir"]
                self.items = self._load_saved_items()
            elif self._has_schedule():
                self.items = self._build_test_schedule()
        if self.saved_root is None:  # generation: the photometric key matters
            for pconf in ([it["photometric_conf"] for it in self.items] if self.items is not None else [conf["photometric"]]):
                if pconf["name"] != "identity":
                    raise NotImplementedError(
                        f"photometric.name {pconf['name']!r}: the reference's 'lg' and 'dark' are albumentations "
                        "pipelines with their own random generator, which this package does not have.  Either generate "
                        "with `photometric.name: identity`, or read a benchmark the reference saved "
                        "(`read_dataset_from_disk: true`, `saved_dataset_dir`)")
        if self.items is not None:
            self.image_names = [it["name"] for it in self.items]
        self._sizes, self._geometry, self._view0 = {}, {}, {}
        if self.items is not None and self.saved_root is None and conf["save_dataset"]:
            self.save_dataset()

    # -- image lists (homographies.py:102-207) --

    def _glob(self, folder, recursive=True):
        patterns = [self.conf["glob"]] if isinstance(self.conf["glob"], str) else self.conf["glob"]
        found = []
        for g in patterns:
            found += list(folder.glob(("**/" if recursive else "") + g))
        return found

    def _folder_images(self, folder):
        return sorted(p.relative_to(folder).as_posix() for p in self._glob(folder))

    def _image_lists(self, data_dir):
        conf = self.conf
        train_dir, val_dir, test_dir = data_dir / "train", data_dir / "val", data_dir / "test"
        if train_dir.exists() and val_dir.exists():
            train, val = self._folder_images(train_dir), self._folder_images(val_dir)
            test = self._folder_images(test_dir) if test_dir.exists() else []
            if conf["test_sequences"] is not None:
                keep = set(conf["test_sequences"])
                test = [n for n in test if self._parse_test_sequence(n) in keep]
            if conf["shuffle_seed"] is not None:
                np.random.RandomState(conf["shuffle_seed"]).shuffle(train)
                np.random.RandomState(conf["shuffle_seed"] + 1).shuffle(val)
            if conf["train_size"] > 0:
                train = train[: conf["train_size"]]
            if conf["val_size"] > 0:
                val = val[: conf["val_size"]]
            return {"train": train, "val": val, "test": test}
        image_dir = data_dir / conf["image_dir"]
        listed = conf["image_list"]
        if listed is None:
            images = self._folder_images(image_dir)
            if not images:
                raise ValueError(f"Cannot find any image in folder: {image_dir}.")
        elif isinstance(listed, (str, Path)):
            path = data_dir / listed
            if not path.exists():
                raise FileNotFoundError(f"Cannot find image list {path}.")
            images = path.read_text().rstrip("\n").split("\n")
        elif isinstance(listed, (list, tuple)):
            images = list(listed)
        else:
            raise ValueError(listed)
        if listed is not None and conf["check_file_exists"]:
            for image in images:
                if not (image_dir / image).exists():
                    raise FileNotFoundError(image_dir / image)
        if conf["shuffle_seed"] is not None:
            np.random.RandomState(conf["shuffle_seed"]).shuffle(images)
        n_train, n_val = conf["train_size"], conf["val_size"]
        return {"train": images[:n_train], "val": images[n_train: n_train + n_val], "test": []}

    @staticmethod
    def _parse_test_sequence(name):
        """"Seq_003_000123.png" -> "Seq_003": the stem up to its last "_" when digits follow it, else None."""
        prefix, sep, suffix = Path(name).stem.rpartition("_")
        return prefix if sep and suffix.isdigit() else None

    def _has_schedule(self):
        c = self.conf
        return (c["test_size"] > 0 and c["test_sequences"] is not None and c["test_homography_levels"] is not None
                and c["test_photometric_levels"] is not None)

    # -- the test schedule (homographies.py:290-449) --

    def _level(self, base, level, key):
        conf = merge(base, {})
        if isinstance(level, (int, float)):
            conf[key] = float(level)
        else:
            conf.update(merge(level, {}))
        return conf

    def _build_test_schedule(self):
        conf = self.conf
        by_sequence = {}
        for name in self.image_names:
            seq = self._parse_test_sequence(name)
            if seq is not None:
                by_sequence.setdefault(seq, []).append(name)
        h_levels, p_levels = list(conf["test_homography_levels"]), list(conf["test_photometric_levels"])
        n_variants = len(h_levels) * len(p_levels)
        if conf["test_size"] <= 0 or conf["test_size"] % n_variants != 0:
            raise ValueError("test_size must be a positive multiple of "
                             "len(test_homography_levels) * len(test_photometric_levels).")
        items = []
        for source_idx, image_name in enumerate(self._select_test_sources(by_sequence)):
            source_dir = Path(image_name).stem
            for hi, h_level in enumerate(h_levels):
                h_conf = self._level(conf["homography"], h_level, "difficulty")
                for pi, p_level in enumerate(p_levels):
                    p_conf = self._level(conf["photometric"], p_level, "p")
                    variant = f"h{hi}_p{pi}.png"
                    idx = len(items)
                    items.append({
                        "idx": idx, "name": f"{source_dir}/{variant}", "source_name": image_name,
                        "source_dir": source_dir, "scene": self._parse_test_sequence(image_name) or "",
                        "seed": conf["test_seed"] + idx, "variant_name": variant,
                        "homography_file": f"H_{source_dir}_{Path(variant).stem}.txt", "homography_idx": hi,
                        "homography_level": float(h_conf["difficulty"]), "photometric_idx": pi,
                        "photometric_level": float(p_conf["p"]), "homography_conf": h_conf, "photometric_conf": p_conf,
                        "source_idx": source_idx})
        return items

    def _select_test_sources(self, by_sequence):
        conf = self.conf
        n_variants = len(conf["test_homography_levels"]) * len(conf["test_photometric_levels"])
        if conf["test_source_dir"] is not None:
            names = self._read_source_dir(conf["test_source_dir"])
            missing = [n for n in names if n not in self.image_names]
            if missing:
                raise ValueError(f"Unknown test images in {conf['test_source_dir']}: {missing[:5]}")
        elif conf["test_image_list"] is not None:
            names = self._read_source_list(conf["test_image_list"])
            missing = [n for n in names if n not in self.image_names]
            if missing:
                raise ValueError(f"Unknown test images in {conf['test_image_list']}: {missing[:5]}")
        else:
            sequences = list(conf["test_sequences"])
            n_sources = conf["test_size"] // n_variants
            if n_sources % len(sequences) != 0:
                raise ValueError("test_size must select the same number of sources per sequence.")
            per_sequence = n_sources // len(sequences)
            names = []
            for seq_idx, seq in enumerate(sequences):
                seq_images = sorted(by_sequence.get(seq, []))
                if len(seq_images) < per_sequence:
                    raise ValueError(f"Not enough test images in sequence {seq}: "
                                     f"need {per_sequence}, found {len(seq_images)}.")
                order = np.random.RandomState(conf["test_seed"] + seq_idx).permutation(len(seq_images))[:per_sequence]
                names.extend(seq_images[i] for i in order)
        expected = conf["test_size"] // n_variants
        if len(names) != expected:
            raise ValueError(f"Expected {expected} test sources, found {len(names)}.")
        if len(set(names)) != len(names):
            raise ValueError("test source list contains duplicates.")
        return names

    def _read_source_dir(self, path_conf):
        path = Path(path_conf)
        if not path.is_absolute():
            path = self.data_root / path
        if not path.exists():
            raise FileNotFoundError(f"Cannot find test source dir {path_conf}.")
        names = []
        for seq in self.conf["test_sequences"]:
            seq_dir = path / seq
            if not seq_dir.exists():
                raise FileNotFoundError(f"Cannot find sequence dir {seq_dir}.")
            found = self._glob(seq_dir, recursive=False)
            if not found:
                raise ValueError(f"No images found in {seq_dir}.")
            names.extend(sorted(p.name for p in found))
        return names

    def _read_source_list(self, path_conf):
        path = Path(path_conf)
        if not path.is_absolute():
            for candidate in (self.data_root / self.conf["data_dir"] / path, self.data_root / path):
                if candidate.exists():
                    path = candidate
                    break
        if not path.exists():
            raise FileNotFoundError(f"Cannot find test image list {path_conf}.")
        return [line for line in path.read_text().splitlines() if line.strip()]

    # -- the saved benchmark (homographies.py:533-701) --

    @staticmethod
    def _attrib_line(image_name, source_name, scene, kind, h_idx, h_level, p_idx, p_level):
        return f"{image_name} {source_name} {scene} {kind} {h_idx} {h_level:.6f} {p_idx} {p_level:.6f}"

    def _load_saved_items(self):
        root = self.saved_root
        manifest = root / "source_names.txt"
        if not manifest.exists():
            raise FileNotFoundError(f"Cannot find saved EndoPatches manifest at {manifest}.")
        items = []
        for source_name in (line for line in manifest.read_text().splitlines() if line.strip()):
            source_dir = Path(source_name).stem
            attribs = root / source_dir / "attribs.txt"
            if not attribs.exists():
                raise FileNotFoundError(f"Cannot find attribs file {attribs}.")
            for line in attribs.read_text().splitlines():
                if not line.strip():
                    continue
                image_name, source_name_line, scene, kind, hi, h_level, pi, p_level = line.split(" ")
                if kind == "source":
                    continue
                items.append({"idx": len(items), "name": f"{source_dir}/{image_name}", "scene": scene,
                              "source_name": source_name_line, "source_dir": source_dir, "variant_name": image_name,
                              "homography_file": f"H_{source_dir}_{Path(image_name).stem}.txt",
                              "homography_idx": int(hi), "homography_level": float(h_level),
                              "photometric_idx": int(pi), "photometric_level": float(p_level)})
        return items

    def save_dataset(self, root=None, pairs=None):
        """Write the scheduled benchmark in the reference's layout (`_save_test_dataset`): per source directory
        `source.png` (view 0 of its first item), every item's `view1` as `<variant>.png`, `H_0to1` through
        numpy.savetxt(fmt="%.18e"), `attribs.txt`; `source_names.txt` at the top.  PNGs are 8-bit,
        clip(image * 255, 0, 255) truncated.  pairs: the items' pair dicts in list order (default: `self.feeder()`,
        i.e. the GPU warps)."""
        if self.items is None or self.saved_root is not None:
            raise ValueError("save_dataset needs a generated test schedule")
        root = self.data_root / self.conf["saved_dataset_dir"] if root is None else Path(root)
        root.mkdir(parents=True, exist_ok=True)
        attribs, source_names = {}, []
        n = 0
        for item, data in zip(self.items, self.feeder() if pairs is None else pairs):
            directory = root / item["source_dir"]
            directory.mkdir(parents=True, exist_ok=True)
            if item["source_dir"] not in attribs:
                _save_png(directory / "source.png", data["view0"]["image"])
                source_names.append(item["source_name"])
                attribs[item["source_dir"]] = [self._attrib_line("source.png", item["source_name"], item["scene"],
                                                                 "source", -1, 0.0, -1, 0.0)]
            _save_png(directory / item["variant_name"], data["view1"]["image"])
            H = data["H_0to1"]
            H = H.detach().cpu().numpy() if torch.is_tensor(H) else np.asarray(H)
            np.savetxt(directory / item["homography_file"], H.reshape(3, 3), fmt="%.18e")
            attribs[item["source_dir"]].append(self._attrib_line(
                item["variant_name"], item["source_name"], item["scene"], "variant", item["homography_idx"],
                item["homography_level"], item["photometric_idx"], item["photometric_level"]))
            n += 1
        if n != len(self.items):
            raise ValueError(f"save_dataset: {n} pairs for {len(self.items)} items")
        for source_dir, lines in attribs.items():
            (root / source_dir / "attribs.txt").write_text("\n".join(lines) + "\n")
        (root / "source_names.txt").write_text("\n".join(source_names) + "\n")
        return root

    # -- items --

    def __len__(self):
        return len(self.items) if self.items is not None else len(self.image_names)

    def source_name(self, idx):
        return self.image_names[idx] if self.items is None else self.items[idx]["source_name"]

    def window(self, h, w):
        """(left, top, cw, ch) of the vignette crop in an h x w image (homographies.py:714-718: `img[y1:y2, x1:x2]`,
        clamped to the image as the slice is); the whole image without `crop_vignette` / coordinates."""
        coords = self.conf["vignette_crop_coords"]
        if not self.conf["crop_vignette"] or coords is None:
            return 0, 0, w, h
        x1, x2, y1, y2 = (int(v) for v in coords)
        if min(x1, x2, y1, y2) < 0:
            raise ValueError(f"vignette_crop_coords {coords}: negative coordinates are not supported")
        x1, x2, y1, y2 = min(x1, w), min(x2, w), min(y1, h), min(y2, h)
        if x2 <= x1 or y2 <= y1:
            raise ValueError(f"vignette_crop_coords {coords} leave nothing of a {w} x {h} image")
        return x1, y1, x2 - x1, y2 - y1

    def _source_hw(self, name):
        if name not in self._sizes:
            self._sizes[name] = image_size(self.image_dir / name)
        return self._sizes[name]

    def geometry(self, idx, hw=None):
        """The two views of item `idx` without pixels (homographies.py:703-786): -> {"view0", "view1"} (`sample_view`
        records) and "H_0to1" float32 [3,3] = compute_homography(coords0, coords1, [1, 1]).  hw: the source's (h, w)
        when the caller has decoded it (default: from the file header).  A scheduled item draws view 0 from
        RandomState(2 seed) with difficulty 0 and view 1 from RandomState(2 seed + 1); otherwise both views draw in
        turn from RandomState(conf.seed + idx) with `reseed`, else from numpy's global generator."""
        if self.saved_root is not None:
            raise ValueError("a saved benchmark has no sampler: its homographies are files")
        conf = self.conf
        seeded = self.items is not None or conf["reseed"]  # then an item is a function of its index: drawn once
        if seeded and idx in self._geometry:
            return self._geometry[idx]
        h, w = self._source_hw(self.source_name(idx)) if hw is None else hw
        _, _, cw, ch = self.window(h, w)
        if self.items is not None:
            item = self.items[idx]
            left = {**item["homography_conf"], "difficulty": 0.0}
            # view 0 has a stream of its own and difficulty 0: every draw is multiplied by zero, so the view is a
            # function of the image size and the settings alone -- sampled once per (size, settings), not per item
            key = (cw, ch, repr(sorted(left.items())))
            if key not in self._view0:
                self._view0[key] = sample_view((cw, ch), left, np.random.RandomState(item["seed"] * 2))
            v0 = self._view0[key]
            v1 = sample_view((cw, ch), dict(item["homography_conf"]), np.random.RandomState(item["seed"] * 2 + 1))
        else:
            rng = np.random.RandomState(conf["seed"] + idx) if conf["reseed"] else np.random
            left, right = dict(conf["homography"]), dict(conf["homography"])
            if conf["right_only"]:
                left["difficulty"] = 0.0
            if conf["left_view_difficulty"] is not None:
                left["difficulty"] = conf["left_view_difficulty"]
            if conf["right_view_difficulty"] is not None:
                right["difficulty"] = conf["right_view_difficulty"]
            v0 = sample_view((cw, ch), left, rng)
            v1 = sample_view((cw, ch), right, rng)
        H = compute_homography(v0["coords"], v1["coords"], [1, 1])
        out = {"view0": v0, "view1": v1, "H_0to1": H.astype(np.float32)}
        if seeded:
            self._geometry[idx] = out
        return out

    def meta(self, idx):
        """Item `idx` without its pixels, un-batched, on the host: what `HPatchesPipeline.run_eval` reads beside the
        cached predictions (`H_0to1`, `name`, `scene`, `view0.image_size`, the views' `scales` = 1)."""
        one = torch.ones(2, dtype=torch.float32)
        if self.saved_root is not None:
            item = self.items[idx]
            directory = self.saved_root / item["source_dir"]
            H = np.loadtxt(directory / item["homography_file"]).astype(np.float32)
            sizes = [image_size(directory / "source.png"), image_size(directory / item["variant_name"])]
            name, scene = item["name"], item["scene"]
        else:
            geo = self.geometry(idx)
            H = geo["H_0to1"]
            pw, ph = (int(v) for v in geo["view0"]["image_size"])
            sizes = [(ph, pw), (ph, pw)]
            item = None if self.items is None else self.items[idx]
            name, scene = (self.image_names[idx], "") if item is None else (item["name"], item["scene"])
        views = {f"view{i}": {"scales": one, "image_size": torch.tensor([float(w), float(h)])}
                 for i, (h, w) in enumerate(sizes)}
        return {"H_0to1": torch.from_numpy(H), "name": name, "scene": scene, "idx": idx,
                "source_name": self.source_name(idx), **views}

    def read_source(self, name, directory=None, grayscale=False):
        """Decoded uint8 image as a host tensor, straight into pinned memory with `pin_memory` (as `HPatches._read`)."""
        path = (self.image_dir if directory is None else directory) / name
        if not (self.conf["pin_memory"] and torch.cuda.is_available()):
            return torch.from_numpy(read_image(path, grayscale))
        holder = []

        def alloc(nbytes):
            holder.append(torch.empty(nbytes, dtype=torch.uint8, pin_memory=True))
            return holder[0].numpy()

        arr = read_image(path, grayscale, alloc)
        return holder[0].view(arr.shape)

    def __getitem__(self, idx):
        """Raw item of a SAVED benchmark (homographies.py:671-701) for `HostImageFeeder`: decoded uint8 `source.png` /
        variant, `H_0to1` [1,3,3] float32 from its text file."""
        if self.saved_root is None:
            raise TypeError("generated pairs have no host-side pixels: iterate `feeder()`")
        item = self.items[idx]
        directory = self.saved_root / item["source_dir"]
        gray = self.conf["grayscale"]
        H = np.loadtxt(directory / item["homography_file"]).astype(np.float32)
        return {"H_0to1": torch.from_numpy(H)[None], "scene": item["scene"], "idx": torch.tensor([item["idx"]]),
                "name": item["name"], "source_name": item["source_name"],
                "view0": {"image": self.read_source("source.png", directory, gray)},
                "view1": {"image": self.read_source(item["variant_name"], directory, gray)}}

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def view_key(self, item, i):
        """The name of the image of view i, or None: view 0 of a scheduled (or saved) source is one image for all its
        items -- its difficulty is 0, so every draw is multiplied by zero whatever the seed -- and is extracted once."""
        if i != 0 or self.items is None:
            return None
        name = item["source_name"]
        return ("view0", name[0] if isinstance(name, (list, tuple)) else name)

    def feeder(self, device="cuda", batch=32, num_workers=2, depth=64):
        """The loader for `export_predictions`.  Generated pairs: `HomographyPairFeeder` (`batch` = the consumer's pair
        batch: all views of a source inside one batch come from one kernel call).  A saved benchmark: its files through
        `HostImageFeeder` (conversion only, no resize), `source.png` copied once per source."""
        if self.saved_root is None:
            return HomographyPairFeeder(self, device=device, batch=batch, num_workers=num_workers)
        from .image_preprocessor import HostImageFeeder

        return HostImageFeeder(self, {"resize": None}, device=device, depth=depth, view_key=self.view_key, keep=4)


def _save_png(path, image):
    """`_save_png` of the reference (homographies.py:533-547): CHW / HW float image -> 8-bit PNG of
    clip(image * 255, 0, 255) truncated (fp32 product, as the reference's)."""
    from PIL import Image

    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    image = np.asarray(image)
    if image.ndim == 4:
        image = image[0]
    if image.ndim == 3:
        image = image.transpose(1, 2, 0)
    u8 = np.clip(image * 255.0, 0, 255).astype(np.uint8)
    if u8.ndim == 3 and u8.shape[-1] == 1:
        u8 = u8[..., 0]
    Image.fromarray(np.ascontiguousarray(u8)).save(str(path), format="PNG")


class HomographyPairFeeder:
    """Pairs of a `HomographyPairs` list rendered on the GPU.  The list is walked `batch` consecutive items at a time;
    every source is decoded once on the host (reader threads, pinned memory) and uploaded once -- one that a batch border
    cuts stays on the device for the next batch --, and inside a batch ONE
    `gfc_warp_perspective` call renders all distinct views of all its items (views with the same matrix -- view 0 of a
    scheduled source -- are one image).  Yields batch-1 pair dicts shaped like `HPatchesFeeder`'s: `view0/1.image`
    [1,C,h,w] float32, `image_size` [1,2], `scales` [1,2] = 1 (device), `H_0to1` [1,3,3] float32, `name`, `scene`,
    `source_name` (lists of one string), `idx` [1]."""

    def __init__(self, dataset, device="cuda", batch=32, num_workers=2):
        self.dataset, self.batch, self.num_workers = dataset, max(1, int(batch)), int(num_workers)
        self.device = torch.device(device if device != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self.warp = warp_perspective  # (tests count the calls through this attribute)
        self.h2d_bytes = 0

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        return self._iterate(range(len(self.dataset)))

    def shard(self, rank, world, group=1):
        from .sharding import round_robin_shard
        idx = list(round_robin_shard(len(self.dataset), int(rank), int(world), max(1, int(group))))
        return zip(idx, self._iterate(idx))

    def _sources(self, chunks):
        """(chunk, its source names in order, {name: decoded host tensor}) per chunk -- decoded are only the sources the
        previous chunk did not hold (a source cut by a chunk border stays on the device: `_iterate`); with reader
        threads the next chunks' files are read while this one is rendered."""
        ds = self.dataset
        seeded = ds.items is not None or ds.conf["reseed"]

        def load(name, chunk):
            u8 = ds.read_source(name)
            if seeded:  # an item's homographies depend on its index alone: drawn here, ahead of the consumer, and kept
                for i in chunk:
                    if ds.source_name(i) == name:
                        ds.geometry(i, (int(u8.shape[0]), int(u8.shape[1])))
            return u8

        def plan():
            held = ()
            for chunk in chunks:
                names = list(dict.fromkeys(ds.source_name(i) for i in chunk))
                yield chunk, names, [n for n in names if n not in held]
                held = names

        if self.num_workers <= 0:
            for chunk, names, fresh in plan():
                yield chunk, names, {n: load(n, chunk) for n in fresh}
            return
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(self.num_workers, thread_name_prefix="gfc-homography-read") as ex:
            def submit(entry):
                chunk, names, fresh = entry
                return chunk, names, fresh, [ex.submit(load, n, chunk) for n in fresh]

            it = plan()
            pending = deque(submit(e) for _, e in zip(range(2), it))
            while pending:
                chunk, names, fresh, futures = pending.popleft()
                nxt = next(it, None)
                if nxt is not None:
                    pending.append(submit(nxt))
                yield chunk, names, {n: f.result() for n, f in zip(fresh, futures)}

    def _iterate(self, indices):
        ds, dev = self.dataset, self.device
        indices = list(indices)
        chunks = [indices[i: i + self.batch] for i in range(0, len(indices), self.batch)]
        copy_stream = torch.cuda.Stream(dev)
        one = torch.ones((1, 2), dtype=torch.float32, device=dev)
        sizes = {}
        resident = {}  # the previous chunk's sources on the device: one cut by the chunk border is not uploaded again
        for chunk, names, decoded in self._sources(chunks):
            main = torch.cuda.current_stream(dev)
            rendered, held = {}, {}
            for name in names:
                if name in decoded:
                    with torch.cuda.stream(copy_stream):
                        src = decoded[name].to(dev, non_blocking=True)
                    self.h2d_bytes += decoded[name].numel()
                else:
                    src = resident[name]
                held[name] = src
                h, w = int(src.shape[0]), int(src.shape[1])
                mats, slot_of, slots = [], {}, {}
                for i in chunk:
                    if ds.source_name(i) != name:
                        continue
                    geo = ds.geometry(i, (h, w))
                    pair = []
                    for tag in ("view0", "view1"):
                        m = np.linalg.inv(geo[tag]["H"])  # destination -> source, float64
                        key = m.tobytes()
                        if key not in slot_of:
                            slot_of[key] = len(mats)
                            mats.append(m)
                        pair.append(slot_of[key])
                    slots[i] = (pair, geo)
                if ds.items is not None and len({pair[0] for pair, _ in slots.values()}) != 1:
                    raise RuntimeError(f"{name}: view 0 differs between the items of a scheduled source")
                pw, ph = (int(v) for v in next(iter(slots.values()))[1]["view0"]["image_size"])
                host_m = torch.from_numpy(np.stack(mats))
                if dev.type == "cuda" and ds.conf["pin_memory"]:
                    host_m = host_m.pin_memory()
                with torch.cuda.stream(copy_stream):
                    dev_m = host_m.to(dev, non_blocking=True)
                    index = torch.zeros(len(mats), dtype=torch.int32, device=dev)
                main.wait_stream(copy_stream)
                for t in (src, dev_m, index):
                    t.record_stream(main)
                images = self.warp(src, index, dev_m, (ph, pw), crop=ds.window(h, w), gray=bool(ds.conf["grayscale"]))
                if (pw, ph) not in sizes:
                    sizes[(pw, ph)] = torch.tensor([[float(pw), float(ph)]], device=dev)
                rendered[name] = (images, slots, sizes[(pw, ph)])
            resident = held
            for i in chunk:
                name = ds.source_name(i)
                images, slots, size = rendered[name]
                (s0, s1), geo = slots[i]
                item = None if ds.items is None else ds.items[i]
                yield {"name": [name if item is None else item["name"]], "scene": ["" if item is None else item["scene"]],
                       "source_name": [name], "idx": torch.tensor([i if item is None else item["idx"]]),
                       "H_0to1": torch.from_numpy(geo["H_0to1"])[None],
                       "view0": {"image": images[s0][None], "image_size": size, "scales": one},
                       "view1": {"image": images[s1][None], "image_size": size, "scales": one}}
