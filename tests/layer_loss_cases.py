"""Inputs of the per-layer loss fixture, regenerated bit for bit from a seed by the fixture maker
(tests/golden/make_layer_loss_golden.py, which runs the reference on them) and by the tests, so that the descriptors
(0.6 MB) are not stored a second time; the fixture keeps the seed it settled on and a checksum of what it was made from.

Two batches of planted correspondences: side 1 is a permuted subset of side 0 plus noise, with unmatched points on both
sides; the labels are the planted ones with some -1 (unmatched) and some -2 (ignore).
  a  B = 2, 130 + 65 key points, `gt_assignment` present
  b  B = 1,  97 + 120 key points, no `gt_assignment`; side 0 has NO unmatched point (its 7 spare points are ignored), so
     num_neg0 = 0 there and the two clamps of weight_loss (losses.py:13-14) act on their own
"""
import torch

SIZE = (640.0, 480.0)
CASES = {"a": {"b": 2, "m": 130, "n": 65, "planted": 48, "ignored_pairs": 5, "ignored_single": 4, "assignment": True},
         "b": {"b": 1, "m": 97, "n": 120, "planted": 90, "ignored_pairs": 6, "ignored_single": 7, "assignment": False}}
N_LAYERS = 9
SAMPLE_ROWS = 16


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def make_case(name, seed, noise=0.25):
    """-> {keypoints0/1 [B,M/N,2], descriptors0/1 [B,M/N,256], size [B,2], gt_matches0/1 int64, gt_assignment bool or
    None}, float32, on the CPU."""
    c = CASES[name]
    b, m, n, k = c["b"], c["m"], c["n"], c["planted"]
    g = torch.Generator().manual_seed(seed * 1000 + (17 if name == "a" else 29))
    size = torch.tensor(SIZE)
    kp0 = torch.rand((b, m, 2), generator=g) * (size - 1)
    kp1 = torch.rand((b, n, 2), generator=g) * (size - 1)
    d0 = _unit(torch.randn((b, m, 256), generator=g))
    d1 = _unit(torch.randn((b, n, 256), generator=g))
    gt0 = torch.full((b, m), -1, dtype=torch.long)
    gt1 = torch.full((b, n), -1, dtype=torch.long)
    for q in range(b):
        src = torch.randperm(m, generator=g)   # side-0 points: the first k are planted
        dst = torch.randperm(n, generator=g)   # their partners on side 1
        i, j = src[:k], dst[:k]
        d1[q, j] = _unit(d0[q, i] + noise / 16.0 * torch.randn((k, 256), generator=g))
        kp1[q, j] = (kp0[q, i] + 6.0 * torch.randn((k, 2), generator=g)).clamp(min=0).minimum(size - 1)
        gt0[q, i], gt1[q, j] = j, i
        ign = c["ignored_pairs"]  # planted pairs the labels ignore
        gt0[q, i[:ign]], gt1[q, j[:ign]] = -2, -2
        spare = c["ignored_single"]  # unplanted side-0 points the labels ignore
        gt0[q, src[k:k + spare]] = -2
        gt1[q, dst[k:k + 3]] = -2
    ga = None
    if c["assignment"]:
        ga = torch.zeros((b, m, n), dtype=torch.bool)
        bi, ii = torch.nonzero(gt0 > -1, as_tuple=True)
        ga[bi, ii, gt0[bi, ii]] = True
    return {"keypoints0": kp0, "keypoints1": kp1, "descriptors0": d0, "descriptors1": d1,
            "size": size[None].expand(b, 2).contiguous(), "gt_matches0": gt0, "gt_matches1": gt1, "gt_assignment": ga}


def input_checksum(case):
    """float64 sums that pin the regenerated inputs to the ones the fixture was made from."""
    return torch.stack([case[k].double().sum() for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1",
                                                          "gt_matches0", "gt_matches1")])


def sample_rows(name):
    """The SAMPLE_ROWS rows (of the B*M / B*N rows of a side) whose descriptors the fixture stores per layer."""
    c = CASES[name]
    g = torch.Generator().manual_seed(5)
    return (torch.randperm(c["b"] * c["m"], generator=g)[:SAMPLE_ROWS].sort().values,
            torch.randperm(c["b"] * c["n"], generator=g)[:SAMPLE_ROWS].sort().values)
