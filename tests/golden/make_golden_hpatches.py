"""Generate tests/golden/hpatches_metrics.npz by running the REFERENCE's own homography evaluation code.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_golden_pose.py); the tests
read the committed .npz, never the reference.  The reference's geometry package imports `kornia` and `cv2` at module
level without using them on this path: two EMPTY modules of those names are put into sys.modules right here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hpatches.py [--seed S]

What is called: gt_matches_from_homography, sym_homography_error, homography_corner_error and warp_points_torch.
gluefactory/eval/utils.py cannot be imported (it imports kornia's find_homography_dlt by name), so the six metrics are
assembled from those functions exactly as its eval_matches_homography does (eval/utils.py:141-185).  For the same reason
the weighted DLT has NO reference vectors: kornia is absent, parity with its solver stays unpinned.

Cases (key i of case c is `<name>_<c>`): uniform key points in 640 x 480, kp1[perm[:k]] = warp(kp0[:k]) + 1.2 px noise,
every 7th match removed, every 11th shifted to a wrong index.
  0  130 x 67   mild affine homography
  1  130 x 67   H[2,:2] != 0
  2  300 x 257  a scale change (0.7) with H[2,:2] != 0, and twins on both sides: kp1[dup1[1]] repeats kp1[dup1[0]],
                the true partner of kp0[dup_row]; kp0[dup0[1]] repeats kp0[dup0[0]], a key point with a partner
  3  300 x 257  mild homography
  4  5 x 4      H = identity, kp0[0] = (0, 0), kp1[0] = (3, 0): the warp of the origin is 0 / (1 + 1e-5) = 0 and d0 = 9
                in ANY binary floating-point arithmetic, d1 = (3 / 1.00001)^2 < 9, so dist == pos_th^2 exactly: the one
                case that tells `<` from `<=`.  It sits on the threshold by construction, so it is the one case the
                "nothing undecided" condition does not apply to.
Outputs per case: the reference's float32 results (gt_matches0/1, err, metrics, warp_fwd, warp_inv, corner_err) and the
same on `.double()` inputs (suffix _f64).  The script walks seeds from --seed until, in cases 0-3, float32 and float64
agree on every integer and tests/hpatches_reference.py finds nothing undecided.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GFC_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for _name in ("kornia", "cv2"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gluefactory.geometry.gt_generation import gt_matches_from_homography  # noqa: E402
from gluefactory.geometry.homography import (  # noqa: E402
    homography_corner_error,
    sym_homography_error,
    warp_points_torch,
)

import hpatches_reference as hr  # noqa: E402

torch.set_grad_enabled(False)
SHAPES = ((130, 67), (130, 67), (300, 257), (300, 257))
SIZE = torch.tensor([640.0, 480.0])


def homography(g, c):
    H = torch.eye(3)
    H[:2, :2] += 0.1 * torch.randn((2, 2), generator=g)
    H[:2, 2] = 20 * torch.randn(2, generator=g)
    if c == 2:
        H[:2, :2] *= 0.7
    if c in (1, 2):
        H[2, :2] = 1e-4 * torch.randn(2, generator=g) + torch.tensor([1e-4, -1e-4])
    return H


def make_case(seed, c):
    g = torch.Generator().manual_seed(seed * 10 + c)
    M, N = SHAPES[c]
    k = min(M, N)
    H = homography(g, c)
    kp0 = torch.rand((M, 2), generator=g) * SIZE
    kp1 = torch.rand((N, 2), generator=g) * SIZE
    perm = torch.randperm(N, generator=g)
    noise = 1.2 * torch.randn((M, 2), generator=g)
    proj = warp_points_torch(kp0[None], H[None], inverse=False)[0] + noise
    kp1[perm[:k]] = proj[:k]
    m0 = torch.full((M,), -1, dtype=torch.long)
    m0[:k] = perm[:k]
    m0[::7] = -1
    m0[1::11] = torch.where(m0[1::11] > -1, (m0[1::11] + 1) % N, m0[1::11])
    dup0 = dup1 = (-1, -1)
    if c == 2:
        # twins: another slot takes a copy of one end of a true correspondence, so that the two copies tie exactly
        # (of correspondences with less than 1 px of noise and an untouched match, so that they are ground-truth matches)
        good = [r for r in range(30, k - 1) if float(noise[r].norm()) < 1.0 and r % 7 != 0 and (r - 1) % 11 != 0]
        i = good[0]                                   # kp0[i] <-> kp1[perm[i]]; every slot of kp1 is taken (M > N):
        j, j2 = int(perm[i]), int(perm[k - 1])        # the partner of kp0[k-1] gives way (that match becomes a wrong one)
        kp1[j2] = kp1[j]
        dup1 = (min(j, j2), max(j, j2))
        i2, i3 = good[1], M - 1                       # kp0[M-1] has no partner (M > N): it repeats kp0[i2]
        kp0[i3] = kp0[i2]
        dup0 = (i2, i3)
    return {"H": H, "kp0": kp0, "kp1": kp1, "matches0": m0, "dup0": torch.tensor(dup0), "dup1": torch.tensor(dup1),
            "dup_row": torch.tensor(i if c == 2 else -1)}


def exact_case():
    kp0 = torch.tensor([[0.0, 0.0], [100.0, 50.0], [200.0, 80.0], [300.0, 300.0], [50.0, 400.0]])
    kp1 = torch.tensor([[3.0, 0.0], [100.5, 50.0], [200.0, 82.0], [500.0, 100.0]])
    return {"H": torch.eye(3), "kp0": kp0, "kp1": kp1, "matches0": torch.tensor([0, 1, 2, -1, 3]),
            "dup0": torch.tensor((-1, -1)), "dup1": torch.tensor((-1, -1)), "dup_row": torch.tensor(-1)}


def run_reference(case, dtype):
    H, kp0, kp1, m0 = case["H"].to(dtype), case["kp0"].to(dtype), case["kp1"].to(dtype), case["matches0"]
    sel = m0 > -1
    pts0, pts1 = kp0[sel], kp1[m0[sel]]
    err = sym_homography_error(pts0, pts1, H)
    gt = gt_matches_from_homography(kp0[None], kp1[None], H[None], pos_th=3.0, neg_th=3.0)

    def recall(m, gt_m):
        mask = (gt_m > -1).float()
        return ((m == gt_m) * mask).sum(1) / (1e-8 + mask.sum(1))

    def precision(m, gt_m):
        mask = ((m > -1) & (gt_m >= -1)).float()
        return ((m == gt_m) * mask).sum(1) / (1e-8 + mask.sum(1))

    metrics = [(err < 1).float().mean().nan_to_num().item(), (err < 3).float().mean().nan_to_num().item(),
               pts0.shape[0], (kp0.shape[0] + kp1.shape[0]) / 2.0, recall(m0[None], gt["matches0"])[0].item(),
               precision(m0[None], gt["matches0"])[0].item()]
    H_off = H + torch.tensor([[0, 0, 1.5], [0, 0, -2.5], [0, 0, 0.0]], dtype=dtype)
    return {"gt_matches0": gt["matches0"][0], "gt_matches1": gt["matches1"][0], "err": err,
            "metrics": torch.tensor(metrics, dtype=torch.float64),
            "warp_fwd": warp_points_torch(kp0[None], H[None], inverse=False)[0],
            "warp_inv": warp_points_torch(kp1[None], H[None], inverse=True)[0],
            "corner_err": homography_corner_error(H_off, H, SIZE.to(dtype))}


def undecided(case):
    H, kp0, kp1 = case["H"].double(), case["kp0"].double(), case["kp1"].double()
    g = hr.gt_matches(kp0, kp1, H)
    _, und = hr.match_errors(kp0, kp1, case["matches0"], H)
    return int(g["undecided0"].sum()) + int(g["undecided1"].sum()) + int(und.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    out = {}
    for c in range(len(SHAPES) + 1):
        seed = args.seed
        while True:
            case = make_case(seed, c) if c < len(SHAPES) else exact_case()
            r32, r64 = run_reference(case, torch.float32), run_reference(case, torch.float64)
            same = all(torch.equal(r32[k], r64[k]) for k in ("gt_matches0", "gt_matches1"))
            same = same and all(torch.equal(r32["err"] < t, r64["err"] < t) for t in (1, 3))
            if c == len(SHAPES) or (same and undecided(case) == 0):
                break
            seed += 1
        assert same, c
        if c == 2:  # the twins are the true correspondence: the LOWER index carries the match on both sides
            (i_lo, i_hi), (j_lo, j_hi) = case["dup0"].tolist(), case["dup1"].tolist()
            g0, g1 = r32["gt_matches0"], r32["gt_matches1"]
            i = int(case["dup_row"])
            assert g0[i] == j_lo and g1[j_lo] == i and g1[j_hi] == -2, (g0[i], g1[j_lo], g1[j_hi])
            assert g0[i_lo] > -1 and g1[g0[i_lo]] == i_lo and g0[i_hi] == -2, (g0[i_lo], g0[i_hi])
        print(f"case {c}: seed {seed}, gt0 match/unmatched/ignore "
              f"{[int((r32['gt_matches0'] == v).sum()) if v < 0 else int((r32['gt_matches0'] > -1).sum()) for v in (0, -1, -2)]}, "
              f"metrics {r32['metrics'].tolist()}")
        out[f"seed_{c}"] = np.int64(seed)
        for k, v in case.items():
            out[f"{k}_{c}"] = v.numpy()
        for k, v in r32.items():
            out[f"{k}_{c}"] = v.numpy()
        for k in ("err", "warp_fwd", "warp_inv", "corner_err", "metrics"):
            out[f"{k}_f64_{c}"] = r64[k].numpy()
    path = os.path.join(HERE, "hpatches_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
