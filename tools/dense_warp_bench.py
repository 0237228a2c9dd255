"""Time the dense-warp ground truth (csrc/gt_dense_warp.hip) against the same arithmetic as float32 torch operations.

    python tools/dense_warp_bench.py --out profiles      ->  profiles/dense_warp_bench.json

Alternating in one process on the same GPU, medians of device-event timings (ms per batch), on the inputs of
tests/dense_warp_reference.make_case (fields of 560 x 560, the training configuration's internal size):
  cycle_dist   gfc_dense_cycle_error at B = 32 against cycle_dist of the reference as torch operations (the transposed
               copy of the field, F.grid_sample, de-normalisation, pixel grid, norm).  Its bytes -- q_to_ref read once
               (8 B per pixel), ref_to_q read once (8 B) and the error written (4 B) -- over its time, against the HBM
               peak of 8.0 TB/s.
  labels       sampling plus labels at B = 32 and B = 1, 2048 + 2048 key points, the configuration's six thresholds, no
               dense outputs, in three forms:
                 taps    gfc_gt_sample_dense_warp with the cycle error at the taps (x 2), gfc_gt_matches_roma
                 field   gfc_dense_cycle_error (x 2) first, then the same two entries sampling the fields
                 torch   cycle_dist twice plus the arithmetic of gt_matches_from_roma as torch operations
The forms are compared on matches0/1 before anything is timed.  ratio_* = other / taps: above 1 the tap form is faster.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_warp_reference as dr  # noqa: E402

from glue_factory_colon_amd import dense_warp  # noqa: E402

HBM_PEAK = 8.0e12
FIELD = (560, 560)
IMG0, IMG1 = (480, 640), (448, 608)
POS, NEG, PC, PCY, NC, NCY = dr.SETTINGS[0][:6]


def denorm(c, hw):
    return torch.stack([(c[..., 0] + 1) / 2 * (hw[1] - 1), (c[..., 1] + 1) / 2 * (hw[0] - 1)], -1)


def torch_cycle_dist(q, r):
    s = F.grid_sample(r.permute(0, 3, 1, 2), q, align_corners=False).permute(0, 2, 3, 1)
    h, w = q.shape[1:3]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=q.dtype, device=q.device), torch.arange(w, dtype=q.dtype, device=q.device),
                            indexing="ij")
    grid = torch.stack([xs, ys], -1)[None] + 0.5
    return torch.linalg.norm(grid - denorm(s, (h, w)), dim=-1)


def torch_sample(kp, dense, q_hw):
    c = torch.stack([kp[..., 0] / (q_hw[1] - 1) * 2 - 1, kp[..., 1] / (q_hw[0] - 1) * 2 - 1], -1)
    d = dense[:, None] if dense.ndim == 3 else dense.permute(0, 3, 1, 2)
    return F.grid_sample(d, c[:, None], align_corners=False)[:, :, 0].transpose(1, 2)


def torch_labels(c):
    """cycle_dist twice plus gt_matches_from_roma's arithmetic without the dense outputs -> (m0, m1)."""
    e0, e1 = torch_cycle_dist(c["warp0"], c["warp1"]), torch_cycle_dist(c["warp1"], c["warp0"])
    p01 = denorm(torch_sample(c["kp0"], c["warp0"], IMG0), IMG1)
    p10 = denorm(torch_sample(c["kp1"], c["warp1"], IMG1), IMG0)
    c0, c1 = torch_sample(c["kp0"], c["certainty0"], IMG0)[..., 0], torch_sample(c["kp1"], c["certainty1"], IMG1)[..., 0]
    y0, y1 = torch_sample(c["kp0"], e0, IMG0)[..., 0], torch_sample(c["kp1"], e1, IMG1)[..., 0]
    v0, v1 = c["scores0"] > 0, c["scores1"] > 0
    vp0 = v0 & torch.isfinite(p01).all(-1) & torch.isfinite(c0) & (c0 > PC) & torch.isfinite(y0) & (y0 < PCY)
    vp1 = v1 & torch.isfinite(p10).all(-1) & torch.isfinite(c1) & (c1 > PC) & torch.isfinite(y1) & (y1 < PCY)
    d0 = ((p01.unsqueeze(-2) - c["kp1"].unsqueeze(-3)) ** 2).sum(-1)
    d1 = ((c["kp0"].unsqueeze(-2) - p10.unsqueeze(-3)) ** 2).sum(-1)
    inf = d0.new_tensor(float("inf"))
    dist = torch.where(vp0.unsqueeze(-1) & vp1.unsqueeze(-2), torch.maximum(d0, d1), inf)
    min0, min1 = dist.min(-1).indices, dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < POS ** 2)
    pos0, pos1 = positive.any(-1), positive.any(-2)
    far0 = vp0 & (torch.where(vp1.unsqueeze(-2), d0, inf).min(-1).values > NEG ** 2)
    far1 = vp1 & (torch.where(vp0.unsqueeze(-1), d1, inf).min(-2).values > NEG ** 2)
    un0 = v0 & torch.isfinite(c0) & torch.isfinite(y0) & (c0 < NC) & (y0 > NCY)
    un1 = v1 & torch.isfinite(c1) & torch.isfinite(y1) & (c1 < NC) & (y1 > NCY)
    m0 = torch.where(pos0, min0, torch.full_like(min0, -2))
    m1 = torch.where(pos1, min1, torch.full_like(min1, -2))
    m0 = torch.where((far0 | un0) & ~pos0, torch.full_like(m0, -1), m0)
    m1 = torch.where((far1 | un1) & ~pos1, torch.full_like(m1, -1), m1)
    return m0, m1


def timed(forms, reps):
    times = {k: [] for k in forms}
    for _ in range(3):
        for f in forms.values():
            f()
    for _ in range(reps):
        for k, f in forms.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            f()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    return {k: statistics.median(v) for k, v in times.items()}


def load(b, m, n, dev):
    one = dr.make_case(21, min(b, 2), m, n, field0=FIELD, field1=FIELD, img0=IMG0, img1=IMG1)
    return {k: torch.cat([v] * (b // v.shape[0]), 0).to(dev).contiguous() for k, v in one.items() if isinstance(v, torch.Tensor)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "field": list(FIELD), "reps": args.reps}

    c = load(32, 2048, 2048, dev)
    mine, ref = dense_warp.cycle_dist(c["warp0"], c["warp1"]), torch_cycle_dist(c["warp0"], c["warp1"])
    diff = (mine - ref).abs().nan_to_num(nan=0.0)
    # the planted NaN / inf pixels only: torch on the GPU casts a non-finite position to an index, the CPU rule gives NaN
    nan_differs = int((torch.isnan(mine) != torch.isnan(ref)).sum())
    assert nan_differs <= 32 * 8 and float(diff.max()) < 1e-2, (nan_differs, float(diff.max()))
    med = timed({"hip": lambda: dense_warp.cycle_dist(c["warp0"], c["warp1"]),
                 "torch": lambda: torch_cycle_dist(c["warp0"], c["warp1"])}, args.reps)
    nbytes = 32 * FIELD[0] * FIELD[1] * 20
    row = {"B": 32, "hip_ms": round(med["hip"], 4), "torch_ms": round(med["torch"], 4),
           "ratio_torch_over_hip": round(med["torch"] / med["hip"], 2), "bytes": nbytes,
           "hip_bytes_per_s": round(nbytes / (med["hip"] * 1e-3) / 1e12, 3),
           "fraction_of_hbm_peak": round(nbytes / (med["hip"] * 1e-3) / HBM_PEAK, 3), "max_abs_difference_px": float(diff.max())}
    print(json.dumps(row))
    result["cycle_dist"] = row

    rows = []
    for b in (32, 1):
        c = load(b, 2048, 2048, dev) if b != 32 else c
        data = {"view0": {"image": torch.empty((b, 1) + IMG0, device=dev)}, "view1": {"image": torch.empty((b, 1) + IMG1, device=dev)}}
        kw = {"valid0": c["scores0"] > 0, "valid1": c["scores1"] > 0, "warp0": c["warp0"], "warp1": c["warp1"],
              "certainty0": c["certainty0"], "certainty1": c["certainty1"], "pos_th": POS, "neg_th": NEG, "pos_cert_th": PC,
              "pos_cycle_error_th": PCY, "neg_cert_th": NC, "neg_cycle_error_th": NCY, "dense": False}

        def taps():
            return dense_warp.gt_matches_from_roma(c["kp0"], c["kp1"], data, add_cycle_error=True, **kw)

        def field():
            e0, e1 = dense_warp.cycle_dist(c["warp0"], c["warp1"]), dense_warp.cycle_dist(c["warp1"], c["warp0"])
            return dense_warp.gt_matches_from_roma(c["kp0"], c["kp1"], data, cycle_error0=e0, cycle_error1=e1, **kw)

        a, f = taps(), field()
        assert torch.equal(a["matches0"], f["matches0"]) and torch.equal(a["matches1"], f["matches1"])
        t0, t1 = torch_labels(c)
        differ = int((t0 != a["matches0"]).sum()) + int((t1 != a["matches1"]).sum())
        assert differ <= 1e-3 * b * 4096, differ  # near-threshold points only
        med = timed({"taps": taps, "field": field, "torch": lambda: torch_labels(c)}, args.reps)
        row = {"B": b, "M": 2048, "N": 2048, "labels_differ_from_torch": differ,
               **{k + "_ms": round(v, 4) for k, v in med.items()},
               "ratio_field_over_taps": round(med["field"] / med["taps"], 2),
               "ratio_torch_over_taps": round(med["torch"] / med["taps"], 2),
               "ratio_torch_over_field": round(med["torch"] / med["field"], 2)}
        print(json.dumps(row))
        rows.append(row)
    result["labels"] = rows
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "dense_warp_bench.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
