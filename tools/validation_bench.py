"""Time the validation pass's label + loss + metrics step against the same arithmetic as torch operations.

    python tools/validation_bench.py --out profiles      ->  profiles/validation_bench.json

Per shape, alternating in one process on the same GPU (medians of device-event timings, ms per batch):
  hip_sparse   gfc_gt_matches_homography without the dense outputs + gfc_lg_validation_metrics on the sparse labels
  hip_dense    the same with `assignment` / `reward` written and the loss reading `gt_assignment`
  torch        gt_matches_from_homography + NLLLoss + row_norm + matcher_metrics written as the reference writes them
               (float32, the M x N matrices materialised) -- the form tests/validation_reference.py restates per pair
Shapes: the homography configuration (B = 128, 512 + 512 points, matchers.homography_matcher) and the MegaDepth one
(B = 32, 2048 + 2048 points, matchers.depth_matcher with th_epi 5 on synthetic posed plane pairs of 480 x 640; there
both forms take their O(M) projections from gfc_eval_pose_project and differ in the M x N part: matching, the epi_th
rule, reward, loss).
The two forms are compared on the labels before anything is timed (equal but for a handful of near-threshold points).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hpatches_cases as hc  # noqa: E402

from glue_factory_colon_amd.homography_matcher import gt_matches_from_homography  # noqa: E402
from glue_factory_colon_amd.losses import validation_metrics  # noqa: E402


def torch_labels(kp0, kp1, H, pos_th, neg_th):
    def warp(kp, Hm):
        h = torch.cat([kp, torch.ones_like(kp[..., :1])], -1) @ Hm.transpose(-1, -2)
        return h[..., :2] / (h[..., 2:] + 1e-5)

    k01, k10 = warp(kp0, H), warp(kp1, torch.linalg.inv(H))
    d0 = ((k01.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2).sum(-1)
    d1 = ((kp0.unsqueeze(-2) - k10.unsqueeze(-3)) ** 2).sum(-1)
    dist = torch.max(d0, d1)
    reward = (dist < pos_th**2).float() - (dist > neg_th**2).float()
    min0, min1 = dist.min(-1).indices, dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < pos_th**2)
    m0 = torch.where(positive.any(-1), min0, torch.full_like(min0, -2))
    m1 = torch.where(positive.any(-2), min1, torch.full_like(min1, -2))
    m0 = torch.where(d0.min(-1).values > neg_th**2, torch.full_like(m0, -1), m0)
    m1 = torch.where(d1.min(-2).values > neg_th**2, torch.full_like(m1, -1), m1)
    return m0, m1, positive, reward


def torch_loss(la, g0, g1, positive, m0, s0, balancing=0.5):
    m, n = g0.shape[1], g1.shape[1]
    w = torch.zeros_like(la)
    w[:, :m, :n] = positive.float()
    w[:, :m, -1] = (g0 == -1).float()
    w[:, -1, :n] = (g1 == -1).float()
    sc = la * w
    nneg0, nneg1 = w[:, :m, -1].sum(-1).clamp(min=1.0), w[:, -1, :n].sum(-1).clamp(min=1.0)
    npos = w[:, :m, :n].sum((-1, -2)).clamp(min=1.0)
    nll_pos = -sc[:, :m, :n].sum((-1, -2)) / npos
    nll_neg = -(sc[:, :m, -1].sum(-1) + sc[:, -1, :n].sum(-1)) / (nneg0 + nneg1)
    row_norm = la.exp()[:, :-1].sum(2).mean(1)
    tp = m0 == g0

    def ratio(mask):
        return (tp * mask).sum(1) / (1e-8 + mask.sum(1))

    rmask, pmask = (g0 > -1).float(), ((m0 > -1) & (g0 >= -1)).float()
    order = torch.argsort(-s0)
    sp, sr, st = pmask.gather(-1, order), rmask.gather(-1, order), tp.gather(-1, order)
    p_pts = torch.cumsum(st * sp, -1) / (1e-8 + torch.cumsum(sp, -1))
    r_pts = torch.cumsum(st * sr, -1) / (1e-8 + sr.sum(-1)[:, None])
    ap = ((r_pts[..., 1:] - r_pts[..., :-1]) * p_pts[:, None, -1]).sum(-1)
    return torch.stack([nll_pos, nll_neg, npos, (nneg0 + nneg1) / 2, balancing * nll_pos + (1 - balancing) * nll_neg,
                        row_norm, ratio(rmask), ratio(pmask), ratio((g0 >= -1).float()), ap], 1)


def torch_depth_labels(kp0, kp1, k01, k10, vis0, vis1, valid0, valid1, F, pos_th, neg_th, epi_th):
    """gt_generation.py:666-716 from the projections on."""
    d0 = ((k01.unsqueeze(-2) - kp1.unsqueeze(-3)) ** 2).sum(-1)
    d1 = ((kp0.unsqueeze(-2) - k10.unsqueeze(-3)) ** 2).sum(-1)
    inf = d0.new_tensor(float("inf"))
    dist = torch.where(vis0.unsqueeze(-1) & vis1.unsqueeze(-2), torch.max(d0, d1), inf)
    min0, min1 = dist.min(-1).indices, dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < pos_th**2)
    m0 = torch.where(positive.any(-1), min0, torch.full_like(min0, -2))
    m1 = torch.where(positive.any(-2), min1, torch.full_like(min1, -2))
    m0 = torch.where((d0.min(-1).values > neg_th**2) & valid0, torch.full_like(m0, -1), m0)
    m1 = torch.where((d1.min(-2).values > neg_th**2) & valid1, torch.full_like(m1, -1), m1)
    p0 = torch.cat([kp0, torch.ones_like(kp0[..., :1])], -1)
    p1 = torch.cat([kp1, torch.ones_like(kp1[..., :1])], -1)
    num = torch.einsum("...mi,...ij,...nj->...nm", p1, F, p0).abs()
    F_p0 = torch.einsum("...ij,...nj->...ni", F, p0)
    Ft_p1 = torch.einsum("...ij,...mi->...mj", F, p1)
    epi = (num / (F_p0[..., None, 0] ** 2 + F_p0[..., None, 1] ** 2 + 1e-15).sqrt()
           + num / (Ft_p1[..., None, :, 0] ** 2 + Ft_p1[..., None, :, 1] ** 2 + 1e-15).sqrt()) / 2
    epi = torch.where((m0.unsqueeze(-1) == -2) & (m1.unsqueeze(-2) == -2), epi, inf)
    m0 = torch.where(~valid0 & (epi.min(-1).values > epi_th), torch.full_like(m0, -1), m0)
    m1 = torch.where(~valid1 & (epi.min(-2).values > epi_th), torch.full_like(m1, -1), m1)
    return m0, m1, positive, (dist < pos_th**2).float() - (epi > epi_th).float()


def bench_depth_shape(b, m, n, epi_th, rounds, iters, h=480, w=640):
    from glue_factory_colon_amd import eval_utils, geometry, synthetic
    from glue_factory_colon_amd.depth_matcher import fundamental_matrix, gt_matches_from_pose_depth

    base = 4
    items, preds = synthetic.posed_plane_pairs(base, h, w, seed=7, model="PINHOLE", num_keypoints=(m, n))
    rep = b // base

    def cat(f):
        return torch.cat([f(it, pr) for it, pr in zip(items, preds)] * rep, 0).cuda()

    kp0, kp1 = cat(lambda it, pr: pr["keypoints0"][None].float()), cat(lambda it, pr: pr["keypoints1"][None].float())
    m0 = cat(lambda it, pr: pr["matches0"][None])
    cam0 = geometry.Camera(cat(lambda it, pr: it["view0"]["camera"]._data.reshape(1, -1)), model="PINHOLE")
    cam1 = geometry.Camera(cat(lambda it, pr: it["view1"]["camera"]._data.reshape(1, -1)), model="PINHOLE")
    T = geometry.Pose(cat(lambda it, pr: it["T_0to1"]._data.reshape(1, -1)))
    depth0, depth1 = cat(lambda it, pr: it["view0"]["depth"].reshape(1, h, w)), cat(lambda it, pr: it["view1"]["depth"].reshape(1, h, w))
    data = {"view0": {"camera": cam0, "depth": depth0}, "view1": {"camera": cam1, "depth": depth1}, "T_0to1": T}
    g = torch.Generator().manual_seed(1)
    la = (torch.randn((b, m + 1, n + 1), generator=g) * 2 - 3).clamp(max=0).cuda()
    s0 = torch.rand((b, m), generator=g).cuda() * (m0 > -1)
    c0, _ = geometry.camera_args(cam0, b, kp0.device)
    c1, _ = geometry.camera_args(cam1, b, kp0.device)
    T01, T10 = geometry.pose_args(T, b, kp0.device)

    def hip(dense):
        gt = gt_matches_from_pose_depth(kp0, kp1, data, 3.0, 5.0, epi_th=epi_th, dense=dense)
        return gt, validation_metrics(la, gt["matches0"], gt["matches1"], gt.get("assignment"), m0, s0)

    def ref():
        _, valid0, k01, vis0 = eval_utils.pose_project(kp0, depth0, cam0, cam1, geometry.Pose(T01))
        _, valid1, k10, vis1 = eval_utils.pose_project(kp1, depth1, cam1, cam0, geometry.Pose(T10))
        g0, g1, positive, reward = torch_depth_labels(kp0, kp1, k01, k10, vis0, vis1, valid0, valid1,
                                                      fundamental_matrix(c0, c1, T01), 3.0, 5.0, epi_th)
        return (g0, g1, positive, reward), torch_loss(la, g0, g1, positive, m0, s0)

    (gt, out), ((g0, g1, positive, reward), _) = hip(True), ref()
    differ = int((gt["matches0"] != g0).sum()) + int((gt["matches1"] != g1).sum())
    assert differ <= 1e-3 * b * (m + n), differ
    reward_differ = int((gt["reward"] != reward).sum())
    assert reward_differ <= 1e-4 * reward.numel(), reward_differ
    tout = torch_loss(la, gt["matches0"], gt["matches1"], gt["assignment"], m0, s0)
    forms = {"hip_sparse": lambda: hip(False), "hip_dense": lambda: hip(True), "torch": ref}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(time_ms(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"B": b, "M": m, "N": n, "pos_th": 3.0, "neg_th": 5.0, "th_epi": epi_th, "image": [w, h],
            "label_rows_that_differ": differ, "reward_elements_that_differ": reward_differ,
            "unmatched_ignore_matched0": [int((gt["matches0"] == -1).sum()), int((gt["matches0"] == -2).sum()),
                                          int((gt["matches0"] > -1).sum())],
            "max_abs_loss_difference": float((out - tout).abs().max()), "median_ms": med,
            "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
            "torch_over_hip_sparse": med["torch"] / med["hip_sparse"], "torch_over_hip_dense": med["torch"] / med["hip_dense"]}


def time_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def bench_shape(b, m, n, pos_th, neg_th, rounds, iters):
    case = hc.metric_case(3, b, m, n)
    kp0, kp1, H, m0 = (case[k].cuda() for k in ("kp0", "kp1", "H", "m0"))
    g = torch.Generator().manual_seed(1)
    la = (torch.randn((b, m + 1, n + 1), generator=g) * 2 - 3).clamp(max=0).cuda()
    s0 = torch.rand((b, m), generator=g).cuda() * (m0 > -1)

    def hip(dense):
        gt = gt_matches_from_homography(kp0, kp1, H, pos_th, neg_th, dense=dense)
        return gt, validation_metrics(la, gt["matches0"], gt["matches1"], gt.get("assignment"), m0, s0)

    def ref():
        g0, g1, positive, reward = torch_labels(kp0, kp1, H, pos_th, neg_th)
        return (g0, g1, positive, reward), torch_loss(la, g0, g1, positive, m0, s0)

    (gt, out), ((g0, g1, positive, _), tout) = hip(True), ref()
    differ = int((gt["matches0"] != g0).sum()) + int((gt["matches1"] != g1).sum())
    assert differ <= 1e-3 * b * (m + n), differ  # float32 twice: only near-threshold points may differ
    tout = torch_loss(la, gt["matches0"], gt["matches1"], gt["assignment"], m0, s0)  # the loss on the SAME labels
    forms = {"hip_sparse": lambda: hip(False), "hip_dense": lambda: hip(True), "torch": ref}
    for fn in forms.values():  # warm every form at this shape
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(time_ms(fn, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"B": b, "M": m, "N": n, "pos_th": pos_th, "neg_th": neg_th, "label_rows_that_differ": differ,
            "max_abs_loss_difference": float((out - tout).abs().max()),
            "median_ms": med, "min_ms": {k: min(v) for k, v in times.items()},
            "max_ms": {k: max(v) for k, v in times.items()},
            "torch_over_hip_sparse": med["torch"] / med["hip_sparse"], "torch_over_hip_dense": med["torch"] / med["hip_dense"]}


def bench_run(pair_batch=32, frames=64, hw=(600, 800), patch=(640, 480), keypoints=512):
    """`ValidationPipeline.run` on generated pairs (the val split of a generated `homographies` tree, identity
    photometric): pairs per second of the second pass, host clock around a pass that ends in a synchronise."""
    import shutil
    import tempfile
    import time

    import endopatches_reference as er
    from glue_factory_colon_amd import validate
    from glue_factory_colon_amd.registry import get_dataset

    root = tempfile.mkdtemp(prefix="gfc_validation_bench_")
    try:
        names = er.make_tree(root, per_sequence=frames // 2, hw=hw)
        for n in names:
            shutil.copy(os.path.join(root, "frames", "test", n), os.path.join(root, "frames", "val", n))
        ds = get_dataset("homographies")({"data_dir": "frames", "photometric": {"name": "identity"}, "reseed": True,
                                          "val_size": frames, "homography": {"patch_shape": list(patch)}}, root, split="val")
        vp = validate.ValidationPipeline({"extractor": {"max_num_keypoints": keypoints}}, pair_batch=pair_batch)
        secs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = vp.run(ds.feeder(batch=pair_batch))
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return {"pairs": res["num_pairs"], "pair_batch": pair_batch, "image": list(patch), "max_num_keypoints": keypoints,
                "seconds_per_pass": secs, "pairs_per_s": res["num_pairs"] / min(secs[1:]),
                "means": {k: v for k, v in res.items() if k != "num_pairs"}}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validation_bench needs the GPU: nothing is measured without one")
    res = {"what": __doc__.split("\n\n")[0], "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "iters_per_timing": args.iters,
           "shapes": {"homography_b128_512": bench_shape(128, 512, 512, 3.0, 3.0, args.rounds, args.iters),
                      "megadepth_b32_2048_th_epi5": bench_depth_shape(32, 2048, 2048, 5.0, args.rounds, args.iters)},
           "validate_run": bench_run()}
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "validation_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"shapes": res["shapes"], "validate_run": res["validate_run"]}, indent=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
