"""Generate tests/golden/endomapper_items.npz by running the REFERENCE's own Endomapper dataset class on CPU.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_golden_hpatches.py, whose
empty `kornia` / `cv2` modules and `_standins` it shares by importing it; an empty `seaborn` module is added the same
way: the reference's dataset module imports its plotting helpers at module level).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_endomapper.py

What is called: gluefactory.datasets.endomapper._PairDataset, with `DATA_PATH` and `seq_lists_path` of that module
pointed at the tree tests/endomapper_reference.write_tree generates in a temporary directory.
Recorded: the item list (seq_map, name0, name1, overlap) of the three configurations endomapper_reference.CONFS (every
pair, ten per map over three overlap bins of which one is too small, a pairs file), and for two items of `all` -- the
first that holds image 000000 and the first that holds 000001 of Seq_001_map0, the two truncation branches -- and one
item of Seq_001_map1 (no padding) every cache tensor of both views with `reseed: true`, the pads included, plus camera,
pose, image size, T_0to1, T_1to0, overlap and names.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden_hpatches as mh  # noqa: E402,F401  (sets up sys.modules / sys.path for the reference)

sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
from omegaconf import OmegaConf  # noqa: E402
from pathlib import Path  # noqa: E402

from gluefactory.datasets import endomapper as ref  # noqa: E402

import endomapper_reference as er  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = er.write_tree(tmp)
        ref.DATA_PATH = Path(tmp)
        ref.seq_lists_path = root
        datasets = {}
        for name, conf in er.CONFS.items():
            full = OmegaConf.merge(OmegaConf.create(ref.Endomapper.default_conf), OmegaConf.create(conf))
            ds = datasets[name] = ref._PairDataset(full, "val")
            out[f"{name}_seq_map"] = np.array([it[0] for it in ds.items])
            out[f"{name}_name0"] = np.array([str(it[1]) for it in ds.items])
            out[f"{name}_name1"] = np.array([str(it[2]) for it in ds.items])
            out[f"{name}_overlap"] = np.array([it[3] for it in ds.items], dtype=np.float32)
            print(name, len(ds.items), "items, maps", sorted(set(out[f"{name}_seq_map"])), ds.items[:2])
        ds = datasets["all"]

        def first(seq_map, image):
            return next(i for i, it in enumerate(ds.items) if it[0] == seq_map and image in (str(it[1]), str(it[2])))

        picks = [first("Seq_001_map0", "000000"), first("Seq_001_map0", "000001"), first("Seq_001_map1", "000004")]
        assert len(set(picks)) == 3
        out["view_items"] = np.array(picks)
        for i in picks:
            item = ds[i]
            out[f"item{i}_T_0to1"], out[f"item{i}_T_1to0"] = item["T_0to1"]._data.numpy(), item["T_1to0"]._data.numpy()
            out[f"item{i}_overlap"], out[f"item{i}_names"] = np.float32(item["overlap_0to1"]), np.array(item["names"])
            for v in ("view0", "view1"):
                view = item[v]
                for k, t in view["cache"].items():
                    out[f"item{i}_{v}_{k}"] = t.numpy()
                out[f"item{i}_{v}_camera"], out[f"item{i}_{v}_T_w2cam"] = view["camera"]._data.numpy(), view["T_w2cam"]._data.numpy()
                out[f"item{i}_{v}_image_size"], out[f"item{i}_{v}_name"] = view["image_size"].numpy(), np.array(view["name"])
                assert view["camera"].model == "OPENCV_FISHEYE" and "image" not in view
                print(i, v, view["name"], {k: tuple(t.shape) for k, t in view["cache"].items()},
                      "valid_3D", int(view["cache"]["valid_3D_mask"].sum()))
    path = os.path.join(HERE, "endomapper_items.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
