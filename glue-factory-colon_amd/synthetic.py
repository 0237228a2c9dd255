"""Synthetic image pairs of the shape BASELINE.json's metric is quoted on.

SURVEY.md 8(d): white noise gives degenerate heat-maps, so images are band-limited
noise (a coarse random field bicubically up-sampled by 8 plus a little fine noise);
view1 is view0 shifted by a known (dx, dy) with border replication so that ground
truth correspondences exist.
"""
import torch
import torch.nn.functional as F


def synthetic_images(n: int, height: int = 480, width: int = 640, seed: int = 1234, device="cpu"):
    """[n,1,H,W] float32 in [0,1]; generated on CPU for reproducibility, then moved."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    ch, cw = (height + 7) // 8, (width + 7) // 8
    coarse = torch.rand((n, 1, ch, cw), generator=g)
    img = F.interpolate(coarse, scale_factor=8, mode="bicubic", align_corners=False)[..., :height, :width]
    img = img + 0.1 * torch.rand((n, 1, height, width), generator=g)
    return img.clamp_(0.0, 1.0).contiguous().to(device)


def shift_image(img: torch.Tensor, dx: int, dy: int):
    """view1[y, x] = view0[y - dy, x - dx] with border replication."""
    n, c, h, w = img.shape
    ys = (torch.arange(h, device=img.device) - dy).clamp_(0, h - 1)
    xs = (torch.arange(w, device=img.device) - dx).clamp_(0, w - 1)
    return img[:, :, ys][:, :, :, xs].contiguous()


def synthetic_pairs(n_pairs: int, height: int = 480, width: int = 640, seed: int = 1234, dx: int = 16, dy: int = 8,
                    device="cpu"):
    v0 = synthetic_images(n_pairs, height, width, seed, device="cpu")
    v1 = shift_image(v0, dx, dy)
    return v0.to(device), v1.to(device)


HPATCHES_LIKE_SHAPES = [(480, 640), (480, 613), (640, 480), (725, 480), (480, 656)]  # (h, w): short side 480


def hpatches_shaped_pairs(n_pairs: int, seed: int = 4000, device="cpu", per_sequence: int = 5, shared_view0: bool = False):
    """`n_pairs` loader items shaped like the HPatches evaluation list (BASELINE config 3; datasets/hpatches.py:94-112:
    RGB, short side resized to 480, arbitrary long side, batch 1, `scales` = new / original size): sequences of
    `per_sequence` pairs share view 0's image shape (the sequence's reference image), view 1's shape changes from item
    to item.  Both views are crops of one band-limited canvas displaced by (24, 16) pixels, so that true
    correspondences exist.  shared_view0: like the real list (datasets/hpatches.py:98-99 reads image 1 of the sequence as
    view 0 of every one of its five pairs) all pairs of a sequence carry THE SAME view-0 image, and their view 1 is
    another crop of the sequence's canvas; items then also carry `scene` (the sequence name, as the reference's items do)."""
    items = []
    for i in range(n_pairs):
        s0 = HPATCHES_LIKE_SHAPES[(i // per_sequence) % len(HPATCHES_LIKE_SHAPES)]
        s1 = HPATCHES_LIKE_SHAPES[(i * 2 + 1) % len(HPATCHES_LIKE_SHAPES)]
        canvas = synthetic_images(1, 760, 680, seed=seed + (i // per_sequence if shared_view0 else i))[0, 0]
        off1 = (16 + 4 * (i % per_sequence), 24 + 6 * (i % per_sequence)) if shared_view0 else (16, 24)
        views = {}
        for tag, (h, w), (y, x), up in (("view0", s0, (0, 0), 2.0), ("view1", s1, off1, 1.5)):
            g = canvas[y:y + h, x:x + w]
            rgb = torch.stack([g * 0.8, g, g * 0.9], 0).clamp(0, 1)
            rgb = ((rgb * 255).round() / 255).float()[None]  # what a decoded uint8 image gives
            ow, oh = int(w * up), int(h * up)
            views[tag] = {"image": rgb.to(device), "image_size": torch.tensor([[float(w), float(h)]], device=device),
                          "scales": torch.tensor([[w / ow, h / oh]], dtype=torch.float32, device=device),
                          "original_image_size": torch.tensor([[float(ow), float(oh)]], device=device)}
        items.append({"name": [f"synth{i // per_sequence}/{i % per_sequence + 2}.ppm"], "scene": [f"synth{i // per_sequence}"],
                      **views})
    return items


# (h, w) of decoded images whose short side 480 resize (ImagePreprocessor resize=480, side="short") gives
# HPATCHES_LIKE_SHAPES, in the same order
HPATCHES_LIKE_ORIGINALS = [(960, 1280), (960, 1226), (1280, 960), (1088, 720), (720, 984)]


def hpatches_like_host_images(n_pairs: int, seed: int = 4000, per_sequence: int = 5, pin: bool = True,
                              shared_view0: bool = False):
    """`n_pairs` RAW loader items as the HPatches dataset holds them right after decoding (datasets/hpatches.py:94-96:
    cv2.imread -> RGB uint8 [H,W,3]), at original sizes HPATCHES_LIKE_ORIGINALS, in (pinned) host memory: the input of
    image_preprocessor.HostImageFeeder.  Same sequence structure and image content as `hpatches_shaped_pairs` (the
    band-limited canvas is up-sampled bicubically to the original size and quantised to bytes).  shared_view0: the five pairs
    of a sequence carry the same view-0 image (one tensor), as in the real list; items then carry `scene`."""
    items = []
    ref_view = {}
    for i in range(n_pairs):
        j0 = (i // per_sequence) % len(HPATCHES_LIKE_SHAPES)
        j1 = (i * 2 + 1) % len(HPATCHES_LIKE_SHAPES)
        canvas = synthetic_images(1, 760, 680, seed=seed + (i // per_sequence if shared_view0 else i))[0, 0]
        off1 = (16 + 4 * (i % per_sequence), 24 + 6 * (i % per_sequence)) if shared_view0 else (16, 24)
        views = {}
        for tag, j, (y, x) in (("view0", j0, (0, 0)), ("view1", j1, off1)):
            if shared_view0 and tag == "view0" and i // per_sequence in ref_view:
                views[tag] = {"image": ref_view[i // per_sequence]}
                continue
            h, w = HPATCHES_LIKE_SHAPES[j]
            oh, ow = HPATCHES_LIKE_ORIGINALS[j]
            g = F.interpolate(canvas[None, None, y:y + h, x:x + w], size=(oh, ow), mode="bicubic", align_corners=False)[0, 0]
            rgb = torch.stack([g * 0.8, g, g * 0.9], -1).clamp(0, 1)
            u8 = (rgb * 255).round().to(torch.uint8).contiguous()
            views[tag] = {"image": u8.pin_memory() if pin else u8}
            if shared_view0 and tag == "view0":
                ref_view[i // per_sequence] = views[tag]["image"]
        items.append({"name": f"synth{i // per_sequence}/{i % per_sequence + 2}.ppm", "scene": f"synth{i // per_sequence}", **views})
    return items


# ---- posed pairs with depth (pose / depth evaluation: eval_utils, eval_pose_pairs) ------------------------------------
POSED_CAMERA_COEFFS = {"PINHOLE": (), "RADIAL": (-0.12, 0.02), "OPENCV": (-0.12, 0.02, 0.002, -0.001),
                       "OPENCV_FISHEYE": (-0.02, 0.005, -0.001, 0.0002)}
POSED_NOISE_PX = (0.3, 2.0, 4.0, 8.0)


def _kb4_tan_theta(rd, k):
    """float64 numpy: tan(theta) of theta (1 + k1 theta^2 + ... + k4 theta^8) = rd (Newton, 50 rounds)."""
    import numpy as np

    th = rd.copy()
    for _ in range(50):
        t2 = th * th
        val = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - rd
        slope = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
        th = th - val / slope
    return np.tan(th)


def posed_pixel_to_ray(cam, model, xy):
    """float64 numpy [..., 2] pixels -> [..., 3] points on the z = 1 plane, by the evaluation's own camera convention:
    normalise by the intrinsics; only the fisheye model removes its distortion."""
    import numpy as np

    n = (xy - cam[4:6]) / cam[2:4]
    if model == "OPENCV_FISHEYE":
        rd = np.linalg.norm(n, axis=-1, keepdims=True)
        n = n * np.where(rd > 1e-12, _kb4_tan_theta(rd, cam[6:10]) / np.maximum(rd, 1e-300), 1.0)
    return np.concatenate([n, np.ones_like(n[..., :1])], -1)


def posed_point_to_pixel(cam, model, p3d):
    """float64 numpy [..., 3] points in the camera frame (z > 0) -> [..., 2] pixels through the camera model."""
    import numpy as np

    u = p3d[..., :2] / p3d[..., 2:]
    r2 = (u * u).sum(-1, keepdims=True)
    if model == "OPENCV_FISHEYE":
        r = np.sqrt(r2)
        th = np.arctan(r)
        t2 = th * th
        k = cam[6:10]
        rd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
        u = u * np.where(r > 1e-12, rd / np.maximum(r, 1e-300), 1.0)
    elif model in ("RADIAL", "OPENCV"):
        d = u * (1 + cam[6] * r2 + cam[7] * r2 * r2)
        if model == "OPENCV":
            uv = u[..., :1] * u[..., 1:]
            d = d + 2 * cam[8:10] * uv + cam[8:10][::-1] * (r2 + 2 * u * u)
        u = d
    return u * cam[2:4] + cam[4:6]


def posed_plane_pairs(n: int, h: int = 96, w: int = 128, seed: int = 0, model: str = "PINHOLE", num_keypoints=(257, 130),
                      coeffs=None):
    """`n` analytic posed pairs for the pose / depth evaluation: a tilted plane seen by two cameras of `model`
    (geometry.CAMERA_MODELS).  Per-pixel depth of both views comes from the intersection of each pixel centre's ray
    with the plane in float64 (stored as float32); a few rectangular holes carry depth 0.  Key points: about 70 % of
    the smaller view's points are planted correspondences (a point of view 0 inside a hole-free area, its exact image in
    view 1 through plane, pose and camera model, displaced by 0.3, 2, 4 or 8 px in turn), the rest are unrelated
    points; view 1's points are shuffled.  The predicted matches are the planted ones, every tenth of them pointed at a
    wrong partner, and every unrelated seventh point matched at random.  `coeffs` replaces the model's distortion
    coefficients (POSED_CAMERA_COEFFS).

    Returns (items, preds): items[i] is a loader item of batch 1 in the reference's layout (`name`, `T_0to1` a Pose,
    `view0/1` = {`camera`: Camera, `depth` [1,h,w]}); preds[i] the un-batched record of the pair (`keypoints0/1`,
    `matches0/1`, `matching_scores0/1`), as the prediction cache holds it.  Seeded, CPU."""
    import numpy as np

    from .geometry import Camera, Pose

    rng = np.random.default_rng(seed)
    M, N = num_keypoints
    coeffs = tuple(POSED_CAMERA_COEFFS[model] if coeffs is None else coeffs)
    items, preds = [], []
    pix = np.stack(np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5), -1)  # [h,w,2] pixel centres
    for i in range(n):
        cams = []
        for _ in range(2):
            f = (0.55 if model == "OPENCV_FISHEYE" else 0.8) * w * rng.uniform(0.95, 1.05)
            cams.append(np.array([w, h, f, f * rng.uniform(0.98, 1.02), w / 2 + rng.uniform(-2, 2), h / 2 + rng.uniform(-2, 2),
                                  *coeffs] + [0.0] * (4 - len(coeffs))))
        # plane normal . X = dist in the frame of camera 0; camera 1 = small rotation + translation
        normal = np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), 1.0])
        normal /= np.linalg.norm(normal)
        dist = rng.uniform(2.0, 3.0)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad(rng.uniform(2.0, 6.0))
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        t = np.array([rng.uniform(0.1, 0.3) * rng.choice([-1, 1]), rng.uniform(-0.1, 0.1), rng.uniform(-0.08, -0.02)])
        # the same plane in the frame of camera 1: normal1 . X1 = dist1
        normal1, dist1 = R @ normal, dist + (R @ normal) @ t
        depths = []
        for c, nrm, dd in ((cams[0], normal, dist), (cams[1], normal1, dist1)):
            depth = dd / (posed_pixel_to_ray(c, model, pix) @ nrm)
            for _ in range(3):  # holes
                hh, hw = rng.integers(h // 12 + 2, h // 5 + 3), rng.integers(w // 12 + 2, w // 5 + 3)
                y0, x0 = rng.integers(0, h - hh), rng.integers(0, w - hw)
                depth[y0:y0 + hh, x0:x0 + hw] = 0.0
            depths.append(depth.astype(np.float32))
        # planted correspondences
        n_plant = int(0.7 * min(M, N))
        kp0 = np.stack([rng.uniform(1.0, w - 1.0, 4 * M), rng.uniform(1.0, h - 1.0, 4 * M)], -1)
        ray = posed_pixel_to_ray(cams[0], model, kp0)
        X1 = (ray * (dist / (ray @ normal))[:, None]) @ R.T + t
        img = posed_point_to_pixel(cams[1], model, X1)
        d0_at = depths[0][np.clip(kp0[:, 1].astype(int), 0, h - 1), np.clip(kp0[:, 0].astype(int), 0, w - 1)]
        ok = (img[:, 0] > 9) & (img[:, 0] < w - 10) & (img[:, 1] > 9) & (img[:, 1] < h - 10) & (d0_at > 0)
        keep = np.nonzero(ok)[0][:n_plant]
        n_plant = len(keep)
        phi = rng.uniform(0, 2 * np.pi, n_plant)
        noise = np.asarray(POSED_NOISE_PX)[np.arange(n_plant) % 4][:, None] * np.stack([np.cos(phi), np.sin(phi)], -1)
        k0 = np.concatenate([kp0[keep], np.stack([rng.uniform(0.5, w - 0.5, M - n_plant),
                                                  rng.uniform(0.5, h - 0.5, M - n_plant)], -1)])
        k1 = np.concatenate([img[keep] + noise, np.stack([rng.uniform(0.5, w - 0.5, N - n_plant),
                                                          rng.uniform(0.5, h - 0.5, N - n_plant)], -1)])
        perm = rng.permutation(N)  # k1_shuffled[q] = k1[perm[q]]
        where = np.argsort(perm)   # planted partner j sits at where[j]
        m0 = np.full(M, -1, dtype=np.int64)
        m0[:n_plant] = where[:n_plant]
        wrong = np.arange(0, n_plant, 10)
        m0[wrong] = where[(wrong + 3) % max(n_plant, 1)]
        extra = np.arange(n_plant, M, 7)
        m0[extra] = rng.integers(0, N, len(extra))
        # a match list is one-to-one: a later duplicate of a partner becomes unmatched
        _, first = np.unique(m0, return_index=True)
        dup = np.ones(M, bool)
        dup[first] = False
        m0[dup & (m0 > -1)] = -1
        m1 = np.full(N, -1, dtype=np.int64)
        m1[m0[m0 > -1]] = np.nonzero(m0 > -1)[0]
        T = np.concatenate([R.reshape(9), t])
        items.append({"name": [f"plane_{model.lower()}_{seed}_{i}"],
                      "T_0to1": Pose(torch.from_numpy(T[None]).float()),
                      "view0": {"camera": Camera(torch.from_numpy(cams[0][None]).float(), model=model),
                                "depth": torch.from_numpy(depths[0][None])},
                      "view1": {"camera": Camera(torch.from_numpy(cams[1][None]).float(), model=model),
                                "depth": torch.from_numpy(depths[1][None])}})
        preds.append({"keypoints0": torch.from_numpy(k0).float(), "keypoints1": torch.from_numpy(k1[perm]).float(),
                      "matches0": torch.from_numpy(m0), "matches1": torch.from_numpy(m1),
                      "matching_scores0": torch.from_numpy((m0 > -1).astype(np.float32)),
                      "matching_scores1": torch.from_numpy((m1 > -1).astype(np.float32))})
    return items, preds


POSED_RELIEF_NOISE_PX = (0.0, 0.1, 0.2, 0.1)


def posed_relief_pairs(n: int, h: int = 96, w: int = 128, seed: int = 0, model: str = "PINHOLE", num_keypoints=(257, 130),
                       off_plane_share: float = 0.3):
    """`n` analytic posed pairs for the robust relative-pose estimator: a dominant tilted plane plus `off_plane_share`
    of the planted points at other depths (0.5 to 1.5 times the plane's depth along their ray).  A purely planar scene
    (`posed_plane_pairs`) leaves the relative pose two-fold ambiguous for any estimator; the relief removes that.  No
    depth maps.  Key points and matches as in `posed_plane_pairs`: about 70 % of the smaller view's points are planted
    correspondences (the exact image in view 1 through pose and camera model, displaced by 0, 0.1, 0.2 or 0.1 px in
    turn), the rest unrelated points; view 1's points are shuffled; every tenth planted match points at a wrong
    partner and every unrelated seventh point is matched at random.

    Returns (items, preds) in the layout of `posed_plane_pairs`, `view0/1` = {`camera`} only.  Seeded, CPU."""
    import numpy as np

    from .geometry import Camera, Pose

    rng = np.random.default_rng([seed, 31])
    M, N = num_keypoints
    coeffs = tuple(POSED_CAMERA_COEFFS[model])
    items, preds = [], []
    for i in range(n):
        cams = []
        for _ in range(2):
            f = (0.55 if model == "OPENCV_FISHEYE" else 0.8) * w * rng.uniform(0.95, 1.05)
            cams.append(np.array([w, h, f, f * rng.uniform(0.98, 1.02), w / 2 + rng.uniform(-2, 2), h / 2 + rng.uniform(-2, 2),
                                  *coeffs] + [0.0] * (4 - len(coeffs))))
        normal = np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), 1.0])
        normal /= np.linalg.norm(normal)
        dist = rng.uniform(2.0, 3.0)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad(rng.uniform(2.0, 6.0))
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        t = np.array([rng.uniform(0.1, 0.3) * rng.choice([-1, 1]), rng.uniform(-0.1, 0.1), rng.uniform(-0.08, -0.02)])
        n_plant = int(0.7 * min(M, N))
        kp0 = np.stack([rng.uniform(1.0, w - 1.0, 4 * M), rng.uniform(1.0, h - 1.0, 4 * M)], -1)
        ray = posed_pixel_to_ray(cams[0], model, kp0)
        depth = dist / (ray @ normal)
        off = rng.uniform(0, 1, 4 * M) < off_plane_share
        depth = np.where(off, depth * rng.uniform(0.5, 1.5, 4 * M), depth)
        X1 = (ray * depth[:, None]) @ R.T + t
        img = posed_point_to_pixel(cams[1], model, X1)
        ok = (img[:, 0] > 9) & (img[:, 0] < w - 10) & (img[:, 1] > 9) & (img[:, 1] < h - 10) & (X1[:, 2] > 0.1)
        keep = np.nonzero(ok)[0][:n_plant]
        n_plant = len(keep)
        phi = rng.uniform(0, 2 * np.pi, n_plant)
        noise = np.asarray(POSED_RELIEF_NOISE_PX)[np.arange(n_plant) % 4][:, None] * np.stack([np.cos(phi), np.sin(phi)], -1)
        k0 = np.concatenate([kp0[keep], np.stack([rng.uniform(0.5, w - 0.5, M - n_plant),
                                                  rng.uniform(0.5, h - 0.5, M - n_plant)], -1)])
        k1 = np.concatenate([img[keep] + noise, np.stack([rng.uniform(0.5, w - 0.5, N - n_plant),
                                                          rng.uniform(0.5, h - 0.5, N - n_plant)], -1)])
        perm = rng.permutation(N)  # k1_shuffled[q] = k1[perm[q]]
        where = np.argsort(perm)   # planted partner j sits at where[j]
        m0 = np.full(M, -1, dtype=np.int64)
        m0[:n_plant] = where[:n_plant]
        wrong = np.arange(0, n_plant, 10)
        m0[wrong] = where[(wrong + 3) % max(n_plant, 1)]
        extra = np.arange(n_plant, M, 7)
        m0[extra] = rng.integers(0, N, len(extra))
        _, first = np.unique(m0, return_index=True)  # one-to-one: a later duplicate of a partner becomes unmatched
        dup = np.ones(M, bool)
        dup[first] = False
        m0[dup & (m0 > -1)] = -1
        m1 = np.full(N, -1, dtype=np.int64)
        m1[m0[m0 > -1]] = np.nonzero(m0 > -1)[0]
        T = np.concatenate([R.reshape(9), t])
        items.append({"name": [f"relief_{model.lower()}_{seed}_{i}"],
                      "T_0to1": Pose(torch.from_numpy(T[None]).float()),
                      "view0": {"camera": Camera(torch.from_numpy(cams[0][None]).float(), model=model)},
                      "view1": {"camera": Camera(torch.from_numpy(cams[1][None]).float(), model=model)}})
        preds.append({"keypoints0": torch.from_numpy(k0).float(), "keypoints1": torch.from_numpy(k1[perm]).float(),
                      "matches0": torch.from_numpy(m0), "matches1": torch.from_numpy(m1),
                      "matching_scores0": torch.from_numpy((m0 > -1).astype(np.float32)),
                      "matching_scores1": torch.from_numpy((m1 > -1).astype(np.float32))})
    return items, preds
