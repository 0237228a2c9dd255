"""A generated Endomapper tree (seeded, a few hundred KB) and the configurations the fixture
tests/golden/endomapper_items.npz was recorded with -- shared by tests/golden/make_golden_endomapper.py (which runs the
reference's `_PairDataset` on it), the host and GPU tests and tools/sparse_map_bench.py.

  Seq_001_map0   12 images; image 000000 has 90 features, 70 of them valid_3D (more valid points than max_num_features
                 = 64: the top-k among the valid ones), image 000001 has 80 features, 30 valid (all valid ones plus the
                 best invalid ones), the others 40..63 (padded).  Overlaps uniform in (0, 0.75) plus four pairs at 0.9:
                 with three bins over (0.3, 1.0] the top bin is too small for `val_num_per_scene: 10`.
  Seq_001_map1   11 images of exactly 64 features: no padding, views shared between pairs as one tensor.
  Seq_002_map0   5 images: dropped by `min_images_per_map: 10`.
  Seq_003        in the split list, no map.
Key points lie on a textured plane seen by a moving OPENCV_FISHEYE camera, so ids, depths and poses are consistent and
the labels find matches.
"""
from pathlib import Path

import numpy as np

DATA_DIR = "Endomapper_CUDASIFT"
LIMIT = 64
BASE_CONF = {"data_dir": DATA_DIR, "val_split": "val_seqs_maps.txt", "max_num_features": LIMIT, "reseed": True,
             "seed": 3, "min_overlap": 0.3, "max_overlap": 1.0}
CONFS = {"all": {**BASE_CONF, "val_num_per_scene": None},
         "ten": {**BASE_CONF, "val_num_per_scene": 10, "num_overlap_bins": 3},
         "pairs": {**BASE_CONF, "val_pairs": "val_pairs.txt"}}
CAMERA = {"model": "OPENCV_FISHEYE", "width": 320, "height": 240,
          "params": np.array([150.0, 150.0, 160.0, 120.0, 0.01, -0.002, 0.0005, 0.0])}
W, H = 320, 240


def _rot(w):
    th = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-12)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def _project(p_cam):
    """OPENCV_FISHEYE (Kannala-Brandt) of camera points [n,3] -> pixels [n,2]."""
    fx, fy, cx, cy, k1, k2, k3, k4 = CAMERA["params"]
    x, y = p_cam[:, 0] / p_cam[:, 2], p_cam[:, 1] / p_cam[:, 2]
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    thd = th * (1 + k1 * th**2 + k2 * th**4 + k3 * th**6 + k4 * th**8)
    s = np.where(r > 1e-8, thd / np.maximum(r, 1e-8), 1.0)
    return np.stack([fx * x * s + cx, fy * y * s + cy], -1)


def _map(rng, seq, map_id, n_images, counts, n_points=150, high_pairs=0):
    pts = np.stack([rng.uniform(-1.2, 1.2, n_points), rng.uniform(-0.9, 0.9, n_points),
                    2.0 + 0.2 * rng.standard_normal(n_points)], -1)
    point_desc = rng.standard_normal((n_points, 128)).astype(np.float32)
    per = {k: [] for k in ("keypoints", "descriptors", "depths", "scales", "orientations", "scores", "point3D_ids",
                           "valid_depth_mask", "valid_3d_mask")}
    poses = []
    for i in range(n_images):
        R, t = _rot(0.04 * rng.standard_normal(3)), 0.08 * rng.standard_normal(3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        poses.append(T)
        n, n_valid = counts[i]
        cam = pts @ R.T + t
        px = _project(cam)
        inside = np.where((px[:, 0] > 2) & (px[:, 0] < W - 2) & (px[:, 1] > 2) & (px[:, 1] < H - 2))[0]
        chosen = rng.permutation(inside)[:n_valid]
        n_valid = len(chosen)
        kp = np.concatenate([px[chosen] + 0.3 * rng.standard_normal((n_valid, 2)),
                             np.stack([rng.uniform(2, W - 2, n - n_valid), rng.uniform(2, H - 2, n - n_valid)], -1)])
        depth = np.concatenate([cam[chosen, 2], np.full(n - n_valid, -1.0)])
        has_depth = np.concatenate([rng.uniform(size=n_valid) > 0.1, np.zeros(n - n_valid, bool)])
        desc = np.concatenate([point_desc[chosen] + 0.2 * rng.standard_normal((n_valid, 128)),
                               rng.standard_normal((n - n_valid, 128))]).astype(np.float32)
        order = rng.permutation(n)
        per["keypoints"].append(kp[order].astype(np.float32))
        per["descriptors"].append((desc / np.linalg.norm(desc, axis=1, keepdims=True))[order])
        per["depths"].append(np.where(has_depth, depth, -1.0)[order].astype(np.float32))
        per["scales"].append(rng.uniform(1.0, 6.0, n).astype(np.float32))
        per["orientations"].append(rng.uniform(0.0, 360.0, n).astype(np.float32))
        per["scores"].append((rng.uniform(0.5, 20.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32))
        per["point3D_ids"].append(np.concatenate([chosen + 1000, np.full(n - n_valid, -1)])[order].astype(np.int64))
        per["valid_depth_mask"].append(has_depth[order])
        per["valid_3d_mask"].append(np.concatenate([np.ones(n_valid, bool), np.zeros(n - n_valid, bool)])[order])
    overlap = rng.uniform(0.01, 0.75, (n_images, n_images)).astype(np.float32)
    np.fill_diagonal(overlap, 0.0)
    for q in range(high_pairs):
        overlap[q, q + 2] = 0.9

    def ragged(items):
        out = np.empty(len(items), dtype=object)
        for i, it in enumerate(items):
            out[i] = it
        return out

    cameras = np.empty(1, dtype=object)
    cameras[0] = CAMERA
    return {"image_names": np.array([f"{i:06d}" for i in range(n_images)]),
            "image_sizes": np.tile(np.array([[W, H]]), (n_images, 1)), "camera_ids": np.zeros(n_images, np.int64),
            "camera_indices": np.zeros(n_images, np.int64), "cameras": cameras, "poses": np.stack(poses),
            "intrinsics": np.tile(CAMERA["params"][None], (n_images, 1)), "map_id": np.array(map_id), "seq": np.array(seq),
            "point3D_ids": np.arange(n_points) + 1000, "point3D_coords": pts, "overlap_matrix": overlap,
            **{k + "_per_image": ragged(v) for k, v in per.items()}}


def write_tree(data_root, seed=7):
    """-> <data_root>/Endomapper_CUDASIFT with three maps, the split list and a pairs file."""
    rng = np.random.RandomState(seed)
    root = Path(data_root) / DATA_DIR
    (root / "processed_npz").mkdir(parents=True, exist_ok=True)
    counts0 = [(90, 70), (80, 30)] + [(int(n), int(0.6 * n)) for n in rng.randint(40, 64, 10)]
    np.savez(root / "processed_npz" / "Seq_001_map0.npz", **_map(rng, "Seq_001", "0", 12, counts0, high_pairs=4))
    np.savez(root / "processed_npz" / "Seq_001_map1.npz", **_map(rng, "Seq_001", "1", 11, [(LIMIT, 40)] * 11))
    np.savez(root / "processed_npz" / "Seq_002_map0.npz", **_map(rng, "Seq_002", "0", 5, [(50, 30)] * 5))
    (root / "val_seqs_maps.txt").write_text("Seq_001\nSeq_002\nSeq_003\n")
    (root / "val_pairs.txt").write_text("Seq_001_map0/p_000000_000001.png\nSeq_001_map1/p_000003_000007.png\n"
                                        "Seq_009_map0/p_000000_000001.png\nSeq_001_map0/p_000002_000099.png\n"
                                        "Seq_001_map0/p_000005_000002.png\n")
    return root
