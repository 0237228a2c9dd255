"""Endomapper sparse maps -- counterpart of gluefactory/datasets/endomapper.py (`views: 2`), the dataset of
CudaSift+lightglue_endomapper.yaml and py_cudasift+lightglue_endomapper_dense.yaml.

A map is `<data_root>/<data_dir>/<npz_subpath>/<seq>_map*.npz`: CudaSift key points, descriptors, scales and orientations
per image, a sparse depth and a 3D-point id per key point, poses, cameras (dicts read by `Camera.from_npz`) and an
overlap matrix.  No extractor runs on this data: every view carries its features as `cache`.

`Endomapper(conf, data_root, split)` holds the reference's `default_conf`, its map filter (`min_images_per_map`,
`min_3D_points_per_map`), `sample_new_items` (fixed `*_pairs` files, overlap bins drawn with
`np.random.RandomState(seed)`, the `has_enough_samples` rule, `sort_by_overlap`, the final shuffle) and `_read_view`
(degrees to radians, `keypoint_scores = |score| * scale`, truncation to `max_num_features` that prefers `valid_3D` points,
the `pad_to_length` mode of every key, the optional key-frame image with its zero fallback).
A split is a list of sequence names or a file name resolved against `seq_lists_dir` (default `<data_root>/<data_dir>`;
the reference keeps its lists inside its package, they are not copied here).
ONE deviation: the padding draws use a CPU torch generator seeded `conf.seed + idx`, in the reference's order of draws
(view 0: x column, y column, descriptors; then view 1).  That is the reference's stream under `reseed: true`; without
`reseed` the reference draws from the unseeded global generator.
`num_neg` and `views: 1` raise NotImplementedError (untested in the reference, they read attributes it never fills);
`views: 3` raises as the reference does.
`feeder(device, num_workers, batch)` yields batch-1 pair dicts with `view*.cache` on the device: the npz of a map is
opened once per map, a view is read and truncated once however many pairs hold it, and a view that needs no padding is
uploaded once per batch (`view_key` names it; a padded view gets the pads of its own pair and is uploaded with them).
"""
import logging
from collections.abc import Iterable
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from .base_model import Conf, merge
from .geometry import Camera, Pose

logger = logging.getLogger(__name__)
CACHE_KEYS = ("keypoints", "descriptors", "sparse_depth", "scales", "oris", "keypoint_scores", "point3D_ids",
              "valid_depth_mask", "valid_3D_mask")


def sample_n(data, num, seed=None):
    if len(data) > num:
        return data[np.random.RandomState(seed).choice(len(data), num, replace=False)]
    return data


def pad_to_length(x, length, pad_dim=-2, mode="zeros", bounds=(None, None), generator=None):
    """gluefactory/models/utils/misc.py:19-62 with the draws taken from `generator`."""
    shape = list(x.shape)
    d = x.shape[pad_dim]
    assert d <= length
    if d == length:
        return x
    shape[pad_dim] = length - d
    low, high = bounds
    key = mode.lower() if isinstance(mode, str) else mode
    if key in ("zeros", "false") or key is False:
        xn = torch.zeros(*shape, dtype=x.dtype)
    elif key == "ones":
        xn = torch.ones(*shape, dtype=x.dtype)
    elif key == "minus_one":
        xn = torch.full(shape, -1, dtype=x.dtype)
    elif key == "random":
        low = low if low is not None else x.min()
        high = high if high is not None else x.max()
        xn = torch.empty(*shape).uniform_(float(low), float(high), generator=generator)
    elif key == "random_c":  # the bounds are the fallback for an empty sequence
        xn = torch.cat([torch.empty(*shape[:-1], 1).uniform_(float(x[..., i].min() if d > 0 else low),
                                                             float(x[..., i].max() if d > 0 else high),
                                                             generator=generator)
                        for i in range(shape[-1])], dim=-1)
    else:
        raise ValueError(mode)
    return torch.cat([x, xn], dim=pad_dim)


class Endomapper:
    default_conf = {
        # paths
        "data_dir": "Endomapper_CUDASIFT",
        "npz_subpath": "processed_npz",
        "seq_lists_dir": None,  # where split and pairs FILES are looked up; None: <data_root>/<data_dir>
        # Training
        "train_split": "train_seqs_maps.txt",
        "train_num_per_scene": 500,
        # Validation
        "val_split": "val_seqs_maps.txt",
        "val_num_per_scene": None,
        "val_pairs": None,
        # Overfit (val-like) split
        "overfit_split": None,
        "overfit_num_per_scene": None,
        "overfit_pairs": None,
        # Test
        "test_split": "test_seqs_maps.txt",
        "test_num_per_scene": None,
        "test_pairs": None,
        # data sampling
        "views": 2,
        "min_overlap": 0.3,
        "max_overlap": 1.0,
        "num_overlap_bins": 1,
        "sort_by_overlap": False,
        "triplet_enforce_overlap": False,
        "p_rotate": 0.0,
        "reseed": False,
        "seed": 0,
        "read_image": False,
        "grayscale": False,
        # CudaSift features
        "max_num_features": 2048,
        "min_images_per_map": 10,
        "min_3D_points_per_map": 50,
    }

    def __init__(self, conf, data_root, split="val", load_sample=True):
        self.conf = conf = Conf(merge(self.default_conf, conf or {}))
        self.data_root = Path(data_root)
        self.root = self.data_root / conf.data_dir
        if not self.root.exists():
            raise FileExistsError(f"Endomapper Dataset not found in {self.root} ")
        if conf.views == 3:
            raise NotImplementedError("Triplet Dataset not implemented for Endomapper")
        if conf.views != 2:
            raise NotImplementedError("endomapper: views: 1 is untested in the reference and not built")
        self.lists = Path(conf.seq_lists_dir) if conf.seq_lists_dir else self.root
        self.split = split
        split_conf = conf[split + "_split"]
        if isinstance(split_conf, (str, Path)):
            seqs = (self.lists / split_conf).read_text().rstrip("\n").split("\n")
        elif isinstance(split_conf, Iterable):
            seqs = list(split_conf)
        else:
            raise ValueError(f"Unknown split configuration: {split_conf}.")
        npz_dir = self.root / conf.npz_subpath
        candidates = []
        for seq in sorted(set(seqs)):
            files = sorted(npz_dir.glob(f"{seq}_map*.npz"))
            if not files:
                logger.warning("No maps found for sequence %s in %s", seq, npz_dir)
            candidates += [f.stem for f in files]
        self.image_names, self.image_sizes, self.poses, self.overlap_matrix = {}, {}, {}, {}
        self.seq, self.map_id, self.seqs_maps = {}, {}, []
        for seq_map in candidates:
            path = npz_dir / f"{seq_map}.npz"
            try:
                with np.load(str(path), allow_pickle=True) as z:
                    if z["image_names"].shape[0] < conf.min_images_per_map or \
                            z["point3D_ids"].shape[0] < conf.min_3D_points_per_map:
                        continue
                    self.image_names[seq_map], self.image_sizes[seq_map] = z["image_names"], z["image_sizes"]
                    self.poses[seq_map] = z["poses"]
                    self.map_id[seq_map] = str(np.asarray(z["map_id"]).item())
                    self.seq[seq_map] = str(np.asarray(z["seq"]).item())
                    self.overlap_matrix[seq_map] = z["overlap_matrix"].astype(np.float32, copy=False)
            except Exception:
                logger.warning("Cannot load seq_map data for %s at %s", seq_map, path)
                continue
            self.seqs_maps.append(seq_map)
        if not self.seqs_maps:
            raise ValueError("No Endomapper sequences loaded for split.")
        if load_sample:
            self.sample_new_items(conf.seed)
            assert len(self.items) > 0

    def get_dataset(self, split):
        return self if split == self.split else Endomapper(self.conf, self.data_root, split)

    def sample_new_items(self, seed):
        conf, split = self.conf, self.split
        self.items = []
        num_pos = conf[split + "_num_per_scene"]
        if isinstance(num_pos, Iterable):
            raise NotImplementedError("endomapper: num_neg (negative pairs) is untested in the reference and not built")
        if split != "train" and conf[split + "_pairs"] is not None:  # fixed validation or test pairs
            assert num_pos is None
            for line in (self.lists / conf[split + "_pairs"]).read_text().rstrip("\n").split("\n"):
                seq = line.split("/")[0]
                im0 = str(line.split("/")[1].split("_")[1].strip(".png"))
                im1 = str(line.split("/")[1].split("_")[-1].strip(".png"))
                if seq not in self.image_names:
                    continue
                idx0 = np.where(self.image_names[seq] == im0)[0]
                idx1 = np.where(self.image_names[seq] == im1)[0]
                if len(idx0) == 0 or len(idx1) == 0:
                    continue
                self.items.append((seq, im0, im1, self.overlap_matrix[seq][idx0[0], idx1[0]]))
        else:
            for seq_map in self.seqs_maps:
                mat = self.overlap_matrix[seq_map]
                if num_pos is not None:  # a subset of the pairs, binned by overlap
                    num_bins = conf.num_overlap_bins
                    assert num_bins > 0
                    width = (conf.max_overlap - conf.min_overlap) / num_bins
                    num_per_bin = num_pos // num_bins
                    pairs_all = []
                    for k in range(num_bins):
                        lo = conf.min_overlap + k * width
                        pairs_all.append(np.stack(np.where((mat > lo) & (mat <= lo + width)), -1))
                    enough = [len(p) >= num_per_bin * 2 for p in pairs_all]
                    if not any(enough):
                        logger.warning("Skipping %s: no bins with enough pairs for sampling.", seq_map)
                        continue
                    if not all(enough):
                        logger.warning("Sampling %s with bins %s.", seq_map,
                                       ",".join(str(i + 1) for i, keep in enumerate(enough) if keep))
                    per_bin = num_pos // max(1, sum(enough))
                    pairs = np.concatenate([sample_n(p, per_bin, seed) for p, keep in zip(pairs_all, enough) if keep], 0)
                else:
                    pairs = np.stack(np.where((mat > conf.min_overlap) & (mat <= conf.max_overlap)), -1)
                names = self.image_names[seq_map]
                self.items.extend((seq_map, names[i], names[j], mat[i, j]) for i, j in pairs)
        if conf.sort_by_overlap:
            self.items.sort(key=lambda i: i[-1], reverse=True)
        else:
            np.random.RandomState(seed).shuffle(self.items)

    def __len__(self):
        return len(self.items)

    # ---- one view -------------------------------------------------------------------------------------------------
    def _read_features(self, seq_map, image_name, npz=None):
        """The truncated, unpadded features of a view and what does not depend on the pair."""
        conf = self.conf
        idx = np.where(self.image_names[seq_map] == image_name)[0][0]
        z = npz if npz is not None else np.load(str(self.root / conf.npz_subpath / f"{seq_map}.npz"), allow_pickle=True)
        try:
            scales = torch.from_numpy(z["scales_per_image"][idx]).float()
            cache = {
                "keypoints": torch.from_numpy(z["keypoints_per_image"][idx]).float(),
                "descriptors": torch.from_numpy(z["descriptors_per_image"][idx]).float(),
                "sparse_depth": torch.from_numpy(z["depths_per_image"][idx]).float(),
                "scales": scales,
                "oris": torch.from_numpy(z["orientations_per_image"][idx]).float() * (torch.pi / 180.0),
                "keypoint_scores": torch.from_numpy(np.abs(z["scores_per_image"][idx])).float() * scales,
                "point3D_ids": torch.from_numpy(z["point3D_ids_per_image"][idx]),
                "valid_depth_mask": torch.from_numpy(z["valid_depth_mask_per_image"][idx]).bool(),
                "valid_3D_mask": torch.from_numpy(z["valid_3d_mask_per_image"][idx]).bool(),
            }
            camera = Camera.from_npz(z["cameras"][int(np.asarray(z["camera_indices"][idx]).item())]).float()
        finally:
            if npz is None:
                z.close()
        assert len({v.shape[0] for v in cache.values()}) == 1, "Feature arrays have mismatched lengths."
        limit = conf.max_num_features
        if limit is None:
            raise ValueError("max_num_features must be not None")
        n = cache["keypoints"].shape[0]
        if n > limit:  # truncate, the valid_3D key points first
            valid_idx = torch.where(cache["valid_3D_mask"])[0]
            invalid_idx = torch.where(~cache["valid_3D_mask"])[0]
            scores = cache["keypoint_scores"]
            if len(valid_idx) >= limit:
                indices = valid_idx[torch.topk(scores[valid_idx], limit).indices]
            else:
                rest = invalid_idx[torch.topk(scores[invalid_idx], limit - len(valid_idx)).indices]
                indices = torch.cat([valid_idx, rest], 0)
            cache = {k: v[indices] for k, v in cache.items()}
        name = str(self.image_names[seq_map][idx])
        image_size = torch.tensor(self.image_sizes[seq_map][idx]).float()
        view = {"name": name, "seq_map": seq_map,
                "T_w2cam": Pose.from_4x4mat(self.poses[seq_map][idx].astype(np.float32, copy=False)), "camera": camera,
                "image_size": image_size}
        if conf.read_image and self.split != "train":
            view["name"] = name = f"Keyframe_{name}.png"
            path = self.root / self.seq[seq_map] / "output" / "3D_maps" / self.map_id[seq_map] / "keyframes" / name
            image = None
            if path.exists():
                try:
                    from .image_io import load_image

                    image = load_image(path, grayscale=conf.grayscale)
                except Exception:
                    logger.warning("Failed to load image at %s, using dummy.", path)
            else:
                logger.warning("Image not found at %s, using dummy.", path)
            if image is None:
                image = torch.zeros((1 if conf.grayscale else 3, int(image_size[1]), int(image_size[0])))
            view["image"] = image
        return cache, view

    def _pad(self, cache, image_size, generator):
        n = self.conf.max_num_features
        out = dict(cache)
        out["keypoints"] = pad_to_length(cache["keypoints"], n, -2, "random_c", (0, float(min(image_size))), generator)
        out["descriptors"] = pad_to_length(cache["descriptors"], n, -2, "random", generator=generator)
        for k in ("scales", "oris", "keypoint_scores"):
            out[k] = pad_to_length(cache[k], n, -1, "zeros")
        for k in ("sparse_depth", "point3D_ids"):
            out[k] = pad_to_length(cache[k], n, -1, "minus_one")
        for k in ("valid_depth_mask", "valid_3D_mask"):
            out[k] = pad_to_length(cache[k], n, -1, False)
        return out

    def _read_view(self, seq_map, image_name, generator=None, npz=None, features=None):
        cache, view = features if features is not None else self._read_features(seq_map, image_name, npz)
        return {"cache": self._pad(cache, view["image_size"], generator), **view}

    def getitem(self, idx, read=None):
        """The reference's item (CPU tensors, unbatched).  read(seq_map, name) -> (cache, view): a shared reader."""
        seq_map, name0, name1, overlap = self.items[idx]
        g = torch.Generator().manual_seed(int(self.conf.seed) + int(idx))
        read = read or (lambda s, n: None)
        data0 = self._read_view(seq_map, name0, g, features=read(seq_map, name0))
        data1 = self._read_view(seq_map, name1, g, features=read(seq_map, name1))
        return {"view0": data0, "view1": data1, "T_0to1": data1["T_w2cam"] @ data0["T_w2cam"].inv(),
                "T_1to0": data0["T_w2cam"] @ data1["T_w2cam"].inv(), "overlap_0to1": overlap,
                "names": f"{seq_map}/{data0['name']}_{data1['name']}", "idx": idx}

    __getitem__ = getitem

    def view_key(self, item, i):
        """The name of a view that is the same tensor in every pair of a batch: one that needed no padding."""
        return item[f"view{i}"].get("shared_key")

    def feeder(self, device="cuda", num_workers=2, batch=32):
        return EndomapperFeeder(self, device, num_workers, batch)


class EndomapperFeeder:
    """Batch-1 pair dicts with `view*.cache` on the device, `batch` pairs prepared at a time."""

    def __init__(self, dataset, device, num_workers, batch):
        self.dataset, self.device = dataset, torch.device(device)
        self.num_workers, self.batch = max(1, int(num_workers)), max(1, int(batch))
        self.npz_opened = self.views_read = self.views_uploaded = 0

    def __len__(self):
        return len(self.dataset)

    def _up(self, t):
        return t.to(self.device, non_blocking=True)

    def __iter__(self):
        ds = self.dataset
        limit = ds.conf.max_num_features
        with ThreadPoolExecutor(self.num_workers, thread_name_prefix="gfc-endomapper-read") as pool:
            for first in range(0, len(ds), self.batch):
                ids = range(first, min(first + self.batch, len(ds)))
                wanted = {}  # (seq_map, name) in order of first use
                for i in ids:
                    s, n0, n1, _ = ds.items[i]
                    wanted.setdefault((s, n0))
                    wanted.setdefault((s, n1))
                by_map = {}
                for s, n in wanted:
                    by_map.setdefault(s, []).append(n)

                def read_map(s):
                    with np.load(str(ds.root / ds.conf.npz_subpath / f"{s}.npz"), allow_pickle=True) as z:
                        return [((s, n), ds._read_features(s, n, npz=z)) for n in by_map[s]]

                features = dict(kv for part in pool.map(read_map, by_map) for kv in part)
                self.npz_opened += len(by_map)
                self.views_read += len(features)
                shared = {}  # views without padding: uploaded once
                for i in ids:
                    item = ds.getitem(i, read=lambda s, n: features[(s, n)])
                    for v in ("view0", "view1"):
                        view = item[v]
                        key = (view["seq_map"], view["name"])
                        full = features[(view["seq_map"], ds.items[i][1 if v == "view0" else 2])][0]["keypoints"].shape[0] == limit
                        if full and key in shared:
                            cache = shared[key]
                        else:
                            cache = {k: self._up(t)[None] for k, t in view["cache"].items()}
                            self.views_uploaded += 1
                            if full:
                                shared[key] = cache
                        item[v] = {**view, "cache": cache, "image_size": self._up(view["image_size"])[None],
                                   "shared_key": key if full else None}
                        if "image" in view:
                            item[v]["image"] = self._up(view["image"])[None]
                    item["overlap_0to1"] = float(item["overlap_0to1"])
                    yield item
