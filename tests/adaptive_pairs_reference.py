"""Host helper (test infrastructure): the inputs and oracle traces shared by the tests of the batched adaptive path
(`LightGlue._forward_adaptive_pairs`, `gfc_lg_adaptive_step`).

Four synthetic 240 x 320 pairs, the oracle's SuperPoint (open variant) at 512 key points per image, pair i cut to its
first SHAPES[i] points: counts that cross wave (64) and workgroup (256) boundaries on both sides and are all different.
`traced(depth, width, prune_z)` runs `adaptive_reference.trace` (the oracle's match_adaptive loop with its
intermediates) on every pair and adds `adaptive_reference.bands` -- everything a GPU test excuses is decided here, on
the oracle alone.
"""
import functools

import torch

import adaptive_reference as ar
from oracle import superpoint as osp

SHAPES = ((300, 257), (190, 333), (65, 64), (512, 129))
SIZE = (320.0, 240.0)
# (depth_confidence, width_confidence, prune_z): two early-stop settings on the pruning weights, and pruning alone
CONFIGS = ((0.85, 0.95, 1.5), (0.89, 0.95, 1.5), (-1.0, 0.95, 0.84))


@functools.lru_cache(maxsize=1)
def inputs():
    """[{keypoints0 [1,m,2], keypoints1 [1,n,2], descriptors0 [1,m,256], descriptors1 [1,n,256], size [1,2]}] x 4"""
    from glue_factory_colon_amd import synthetic, weights

    v0, v1 = synthetic.synthetic_pairs(4, 240, 320, seed=77)
    sd = weights.superpoint_open_state_dict(0)
    feats = [osp.extract(sd, v, variant="open", nms_radius=3, max_num_keypoints=512, detection_threshold=0.0)
             for v in (v0, v1)]
    out = []
    for i, (m, n) in enumerate(SHAPES):
        d = {"size": torch.tensor([SIZE])}
        for side, cut in ((0, m), (1, n)):
            kp, de = feats[side]["keypoints"][i], feats[side]["descriptors"][i]
            assert len(kp) == 512
            d[f"keypoints{side}"] = kp[None, :cut].contiguous()
            d[f"descriptors{side}"] = de[None, :cut].contiguous()
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def traced(depth, width, prune_z):
    """Per pair (layers, final, bands) of the oracle under one configuration."""
    sd = ar.state_dict(prune_z)
    out = []
    for d in inputs():
        layers, final, _, _ = ar.trace(sd, d["keypoints0"], d["keypoints1"], d["descriptors0"], d["descriptors1"],
                                       d["size"], d["size"], depth_confidence=depth, width_confidence=width,
                                       filter_threshold=ar.FILTER_THRESHOLD)
        out.append((layers, final, ar.bands(layers, depth, width)))
    return out


# ---- 128-d inputs (the input projection of both adaptive paths) --------------------------------------------------
PAIRS_128 = (2, 1)        # the two smallest shapes: (65, 64) and (190, 333)
CONFIG_128 = (0.9, 0.9)   # (depth_confidence, width_confidence) on the prune_z of CONFIGS[0]


@functools.lru_cache(maxsize=1)
def inputs128():
    """The pairs PAIRS_128 of inputs() with every descriptor cut to its first 128 channels and re-normalised."""
    out = []
    for p in PAIRS_128:
        d = dict(inputs()[p])
        for side in (0, 1):
            de = d[f"descriptors{side}"][..., :128]
            d[f"descriptors{side}"] = torch.nn.functional.normalize(de, dim=-1).contiguous()
        out.append(d)
    return out


def state_dict128():
    from glue_factory_colon_amd import weights

    return weights.lightglue_adaptive_state_dict(0, prune_z=CONFIGS[0][2], input_dim=128)


@functools.lru_cache(maxsize=1)
def traced128():
    """Per pair of inputs128() (layers, final, bands) of the oracle under CONFIG_128, weights with an input_proj."""
    depth, width = CONFIG_128
    sd = state_dict128()
    out = []
    for d in inputs128():
        layers, final, _, _ = ar.trace(sd, d["keypoints0"], d["keypoints1"], d["descriptors0"], d["descriptors1"],
                                       d["size"], d["size"], depth_confidence=depth, width_confidence=width,
                                       filter_threshold=ar.FILTER_THRESHOLD)
        out.append((layers, final, ar.bands(layers, depth, width)))
    return out


# ---- add_scale_ori: nothing pruned, nothing stopped, so that oracle.lightglue.match is the reference ----------------
SCALE_ORI_SHAPE = (65, 64)
SCALE_ORI_WIDTH = 1 - 1e-3   # keep threshold 1e-3: far below every matchability of these inputs (checked on the host)


@functools.lru_cache(maxsize=1)
def scale_ori_case():
    """(inputs, oracle output with its per-layer rows): pair 0 of tests/golden/scale_ori.npz cut to SCALE_ORI_SHAPE
    points, through oracle.lightglue.match with scale_ori0/1 on weights.lightglue_state_dict(0, add_scale_ori=True)."""
    import os

    import numpy as np

    from glue_factory_colon_amd import weights
    from oracle import lightglue as olg

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scale_ori.npz"))
    d = {"size": torch.from_numpy(z["image_size"][:1])}
    for side, cut in ((0, SCALE_ORI_SHAPE[0]), (1, SCALE_ORI_SHAPE[1])):
        for k in ("keypoints", "descriptors", "scales", "oris"):
            d[f"{k}{side}"] = torch.from_numpy(z[f"{k}{side}"][:1, :cut]).contiguous()
        d[f"scale_ori{side}"] = torch.stack([d[f"scales{side}"].reshape(1, cut), d[f"oris{side}"].reshape(1, cut)], -1)
    sd = weights.lightglue_state_dict(0, add_scale_ori=True)
    ref = olg.match(sd, d["keypoints0"], d["keypoints1"], d["descriptors0"], d["descriptors1"], d["size"], d["size"],
                    filter_threshold=ar.FILTER_THRESHOLD, return_layers=True, scale_ori0=d["scale_ori0"],
                    scale_ori1=d["scale_ori1"])
    return d, sd, ref
