"""Restatement of the EndoPatches test schedule (reference gluefactory/datasets/homographies.py:209-216 `_parse_test_sequence`,
:290-397 `_build_test_schedule` / `_select_test_sources`) as plain functions over lists of names, written apart from
glue_factory_colon_amd.homographies: tests/test_endopatches_host.py holds the module to it.

schedule(test_names, conf, listed=None) -> [(item name, seed, source name, scene, homography level, photometric level)]
in item order.  `test_names`: the test split's file names after the sequence filter; `listed`: the source names a
`test_source_dir` / `test_image_list` gives (None: the per-sequence permutation).  Raises ValueError with the
reference's messages.
"""
from pathlib import Path

import numpy as np


def sequence_of(name):
    stem = Path(name).stem
    if "_" not in stem:
        return None
    head, tail = stem.rsplit("_", 1)
    return head if tail.isdigit() else None


def sources(test_names, conf, listed=None, listed_from=None):
    n_variants = len(conf["test_homography_levels"]) * len(conf["test_photometric_levels"])
    wanted = conf["test_size"] // n_variants
    if listed is not None:
        unknown = [n for n in listed if n not in test_names]
        if unknown:
            raise ValueError(f"Unknown test images in {listed_from}: {unknown[:5]}")
        chosen = list(listed)
    else:
        seqs = list(conf["test_sequences"])
        if wanted % len(seqs):
            raise ValueError("test_size must select the same number of sources per sequence.")
        each = wanted // len(seqs)
        chosen = []
        for k, seq in enumerate(seqs):
            pool = sorted(n for n in test_names if sequence_of(n) == seq)
            if len(pool) < each:
                raise ValueError(f"Not enough test images in sequence {seq}: need {each}, found {len(pool)}.")
            chosen += [pool[j] for j in np.random.RandomState(conf["test_seed"] + k).permutation(len(pool))[:each]]
    if len(chosen) != wanted:
        raise ValueError(f"Expected {wanted} test sources, found {len(chosen)}.")
    if len(set(chosen)) != len(chosen):
        raise ValueError("test source list contains duplicates.")
    return chosen


def schedule(test_names, conf, listed=None, listed_from=None):
    h_levels, p_levels = list(conf["test_homography_levels"]), list(conf["test_photometric_levels"])
    n_variants = len(h_levels) * len(p_levels)
    if conf["test_size"] <= 0 or conf["test_size"] % n_variants:
        raise ValueError("test_size must be a positive multiple of "
                         "len(test_homography_levels) * len(test_photometric_levels).")
    out = []
    for src in sources(test_names, conf, listed, listed_from):
        for i, hl in enumerate(h_levels):
            for j, pl in enumerate(p_levels):
                out.append((f"{Path(src).stem}/h{i}_p{j}.png", conf["test_seed"] + len(out), src, sequence_of(src) or "",
                            float(hl), float(pl)))
    return out


def make_tree(root, sequences=("Seq_003", "Seq_016"), per_sequence=3, hw=(48, 64), name="frames", flat=False):
    """A generated image tree `<root>/<name>/{train,val,test}`: `per_sequence` PNG frames of `hw` per sequence in test/
    (smooth colour patterns with some texture, or one flat grey with `flat`), one frame in train/ and val/.
    -> the sorted test file names."""
    from PIL import Image

    h, w = hw
    names = []
    yy, xx = np.mgrid[0:h, 0:w]
    for split in ("train", "val", "test"):
        (Path(root) / name / split).mkdir(parents=True, exist_ok=True)
    for s, seq in enumerate(sequences):
        for k in range(per_sequence):
            g = np.random.RandomState(17 * s + k)
            if flat:
                img = np.full((h, w, 3), 90 + 10 * s + k, np.uint8)
            else:
                base = np.stack([127 + 120 * np.sin(xx / (3.0 + c + k) + s) * np.cos(yy / (2.5 + s + c)) for c in range(3)], -1)
                img = np.clip(base + g.randint(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)
            fname = f"{seq}_{k:06d}.png"
            Image.fromarray(img).save(Path(root) / name / "test" / fname)
            names.append(fname)
    for split in ("train", "val"):
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(Path(root) / name / split / "Seq_000_000000.png")
    return sorted(names)
