"""Time the sparse-map labels (gfc_gt_matches_sparse_map: a pair split over workgroups) against the one-workgroup-per-
pair kernel and against the same arithmetic as torch operations.

    python tools/sparse_map_bench.py --out profiles      ->  profiles/sparse_map_bench.json

Per shape, alternating in one process on the same GPU (medians of device-event timings, ms per batch), the labels alone
(matches0/1 and positive0; no dense outputs, no ids, pos_th 3 <= neg_th 5, no th_epi) on the same inputs
(tests/sparse_map_reference.entry_case):
  split        gfc_gt_matches_sparse_map (sweep + finishing launch)
  split_ids    the same with id seeding and the masks written: what the Endomapper configuration runs
  one_wg       gfc_gt_matches_depth, one workgroup per pair: the yardstick
  torch        the reference's arithmetic as torch operations (float32, the M x N matrices materialised)
The three forms are compared on matches0/1 before anything is timed.  ratio_* = other / split: above 1 the split
kernel is faster.
`validation`: `ValidationPipeline.run` (reader, LightGlue with name-seeded weights, sparse-map labels, loss, metrics) on
the generated tree of tests/endomapper_reference.py (155 pairs of 64 + 64 key points, pair batch 32): wall-clock
pairs/s, the median of three passes after one warm-up pass.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sparse_map_reference as sr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

SHAPES = ((1, 2048, 2048), (4, 2048, 2048), (32, 2048, 2048), (32, 1024, 1024))
POS, NEG = 3.0, 5.0


def torch_labels(c):
    d0 = ((c["p01"].unsqueeze(-2) - c["kp1"].unsqueeze(-3)) ** 2).sum(-1)
    d1 = ((c["kp0"].unsqueeze(-2) - c["p10"].unsqueeze(-3)) ** 2).sum(-1)
    vis = c["vis0"].unsqueeze(-1) & c["vis1"].unsqueeze(-2)
    dist = torch.where(vis, torch.max(d0, d1), d0.new_tensor(float("inf")))
    min0, min1 = dist.min(-1).indices, dist.min(-2).indices
    ismin0 = torch.zeros(dist.shape, dtype=torch.bool, device=dist.device)
    ismin1 = ismin0.clone()
    ismin0.scatter_(-1, min0.unsqueeze(-1), value=1)
    ismin1.scatter_(-2, min1.unsqueeze(-2), value=1)
    positive = ismin0 & ismin1 & (dist < POS**2)
    m0 = torch.where(positive.any(-1), min0, torch.full_like(min0, -2))
    m1 = torch.where(positive.any(-2), min1, torch.full_like(min1, -2))
    m0 = torch.where((m0 == -2) & (d0.min(-1).values > NEG**2) & c["valid0"], torch.full_like(m0, -1), m0)
    m1 = torch.where((m1 == -2) & (d1.min(-2).values > NEG**2) & c["valid1"], torch.full_like(m1, -1), m1)
    return m0, m1


def validation_pass():
    import endomapper_reference as er
    from glue_factory_colon_amd import validate
    from glue_factory_colon_amd.endomapper import Endomapper

    with tempfile.TemporaryDirectory(prefix="gfc_sparse_map_bench_") as tmp:
        er.write_tree(tmp)
        ds = Endomapper(er.CONFS["all"], tmp, "val")
        vp = validate.ValidationPipeline(validate.endomapper_model_conf(), pair_batch=32)
        rates, res = [], None
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = vp.run(ds.feeder("cuda", num_workers=2, batch=32), view_key=ds.view_key)
            torch.cuda.synchronize()
            if i:
                rates.append(res["num_pairs"] / (time.perf_counter() - t0))
    return {"pairs": res["num_pairs"], "keypoints": er.LIMIT, "pair_batch": 32, "pairs_per_s": round(statistics.median(rates), 1),
            "loss_total": res["loss/total"], "gt_extra_positives": res["gt_extra_positives"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for b, m, n in SHAPES:
        one = sr.entry_case(11, min(b, 4), m, n)
        c = {k: torch.cat([v] * (b // v.shape[0]), 0).to(dev).contiguous() for k, v in one.items()}
        m0 = torch.empty((b, m), dtype=torch.long, device=dev)
        m1 = torch.empty((b, n), dtype=torch.long, device=dev)
        pos0 = torch.empty((b, m), dtype=torch.int32, device=dev)
        masks0 = torch.empty((b, 4, m), dtype=torch.uint8, device=dev)
        masks1 = torch.empty((b, 4, n), dtype=torch.uint8, device=dev)
        nbytes = nat.call("gfc_gt_matches_sparse_map_workspace_bytes", b, m, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def split(ids=False):
            i = (c["ids0"], c["ids1"], c["v3d0"], c["v3d1"]) if ids else (None,) * 4
            nat.call("gfc_gt_matches_sparse_map", c["kp0"], c["kp1"], c["p01"], c["p10"], c["vis0"], c["vis1"],
                     c["valid0"], c["valid1"], *i, None, b, m, n, POS, NEG, -1.0, m0, m1, masks0 if ids else None,
                     masks1 if ids else None, pos0, None, None, None, ws, nbytes, device=dev)

        def one_wg():
            nat.call("gfc_gt_matches_depth", c["kp0"], c["kp1"], c["p01"], c["p10"], c["vis0"], c["vis1"], c["valid0"],
                     c["valid1"], None, b, m, n, POS, NEG, -1.0, m0, m1, pos0, None, None, device=dev)

        forms = {"split": split, "split_ids": lambda: split(True), "one_wg": one_wg, "torch": lambda: torch_labels(c)}
        split()
        mine = (m0.clone(), m1.clone())
        one_wg()
        assert torch.equal(mine[0], m0) and torch.equal(mine[1], m1), "split and one-workgroup kernels disagree"
        t0, t1 = torch_labels(c)
        differ = int((t0 != m0).sum()) + int((t1 != m1).sum())
        assert differ <= 1e-3 * b * (m + n), differ  # near-threshold points only
        times = {k: [] for k in forms}
        for _ in range(3):
            for f in forms.values():
                f()
        for _ in range(args.reps):
            for k, f in forms.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                f()
                stop.record()
                stop.synchronize()
                times[k].append(start.elapsed_time(stop))
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"B": b, "M": m, "N": n, "reps": args.reps, "labels_differ_from_torch": differ,
               **{k + "_ms": round(v, 4) for k, v in med.items()},
               "ratio_one_wg_over_split": round(med["one_wg"] / med["split"], 2),
               "ratio_torch_over_split": round(med["torch"] / med["split"], 2),
               "ratio_one_wg_over_split_ids": round(med["one_wg"] / med["split_ids"], 2)}
        print(json.dumps(row))
        rows.append(row)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "sparse_map_bench.json")
    with open(path, "w") as f:
        validation = validation_pass()
        print(json.dumps(validation))
        json.dump({"device": torch.cuda.get_device_name(0), "shapes": rows, "validation": validation}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
