"""Matcher-only timing of the SuperGlue HIP path against its float32 restatement as torch operations on the same GPU.

    python tools/sg_bench.py --out DIR [--iters N] [--warmup W]

Cases: B = 32 and B = 1 pairs of 1024 + 1024 points (tests/superglue_reference.make_inputs: planted correspondences,
name-seeded weights), each at 50 and 100 Sinkhorn iterations.  Timed with device events after warm-up, the HIP path
(glue_factory_colon_amd.superglue) and the restatement (tests/superglue_reference.forward on device tensors)
alternating iteration by iteration in one process.  Per case it also reports
  * the share of the HIP matcher's time spent in Sinkhorn: gfc_sg_sinkhorn alone on the matcher's own cost, timed the
    same way, over the matcher's time;
  * the share spent in the 18 layers: the matcher's time minus that of the same model with `GNN_layers: []`, over the
    matcher's time;
  * the bytes the Sinkhorn kernels move per iteration, counted from the shapes (the cost matrix read once, v read per
    row block, u written, the per-block column partials written and read, v written), against 4 B (M+1) (N+1).
The restatement is checked against the HIP result before anything is timed.  Writes DIR/superglue_bench.json.  The
figures hold for the name-seeded weights; the published checkpoints cannot be fetched.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import superglue_reference as sgr  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import superglue, weights  # noqa: E402


def timed(fns, iters, warmup):
    """name -> callable; alternating, one event pair per call"""
    times = {name: [] for name in fns}
    with torch.no_grad():
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(iters):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "n": len(t)}
            for name, t in times.items()}


def sinkhorn_bytes(b, m, n):
    """Bytes per iteration of the two Sinkhorn kernels, from the shapes.  Row blocks as csrc/superglue.hip sizes them
    (about 64 per matrix, 8..32 rows each); checked against the library's workspace size."""
    rb = min(max((m + 64) // 64, 8), 32, m + 1)
    nblk = (m + rb) // rb
    c = n + 1
    slot = lambda x: (x + 255) // 256 * 256  # noqa: E731
    assert nat.lib().gfc_sg_sinkhorn_workspace_bytes(b, m, n) == slot(b * (m + 1) * 4) + slot(b * c * 4) + slot(b * nblk * c * 8)
    rows_kernel = 4 * b * m * n + 4 * b * nblk * c + 4 * b * (m + 1) + 8 * b * nblk * c
    merge_kernel = 8 * b * nblk * c + 4 * b * c
    return {"rows_per_block": rb, "row_blocks": nblk, "bytes_per_iteration": rows_kernel + merge_kernel,
            "augmented_matrix_bytes": 4 * b * (m + 1) * c,
            "ratio": (rows_kernel + merge_kernel) / (4 * b * (m + 1) * c)}


def case(b, m, n, iters_sk, iters, warmup, dev):
    lib = nat.lib()
    inp = sgr.make_inputs(0, b, m, n)
    data = sgr.as_data(inp, dev)
    conf = {"weights": "synthetic", "num_sinkhorn_iterations": iters_sk}
    model = superglue.SuperGlue(conf).eval().to(dev)
    bare = superglue.SuperGlue({**conf, "weights": None, "GNN_layers": []}).eval()
    bare.load_state_dict(weights.superglue_state_dict(0, n_layers=0))
    bare = bare.to(dev)
    sd = {k: v.to(dev) for k, v in weights.superglue_state_dict(0).items()}
    inp_dev = {k: v.to(dev) for k, v in inp.items()}
    with torch.no_grad():
        out = model(data)
        ref = sgr.forward(sd, inp_dev, iters_sk)
    torch.cuda.synchronize()
    err = float(((out["log_assignment"] - ref["log_assignment"]).abs() / (1 + ref["log_assignment"].abs())).max())
    same = float((out["matches0"] == ref["matches0"]).double().mean())
    assert err < 1e-4 and same == 1.0, (err, same)
    cost = out["sinkhorn_cost"].clone()
    la = torch.empty_like(out["log_assignment"])
    need = lib.gfc_sg_sinkhorn_workspace_bytes(b, m, n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    bin_score = float(model.bin_score.detach())

    def sinkhorn():
        nat.check(lib.gfc_sg_sinkhorn(nat.ptr(cost), bin_score, b, m, n, iters_sk, nat.ptr(la), nat.ptr(ws), need,
                                      nat.stream_ptr(dev)), "gfc_sg_sinkhorn")

    t = timed({"hip": lambda: model(data), "torch_restatement": lambda: sgr.forward(sd, inp_dev, iters_sk),
               "hip_without_layers": lambda: bare(data), "hip_sinkhorn_alone": sinkhorn,
               "torch_sinkhorn_alone": lambda: sgr.sinkhorn(cost, bin_score, iters_sk)}, iters, warmup)
    hip = t["hip"]["median_ms"]
    return {"B": b, "M": m, "N": n, "sinkhorn_iterations": iters_sk, "times": t,
            "speedup_over_torch_restatement": t["torch_restatement"]["median_ms"] / hip,
            "pairs_per_second": b / hip * 1e3,
            "share_sinkhorn": t["hip_sinkhorn_alone"]["median_ms"] / hip,
            "share_layers": (hip - t["hip_without_layers"]["median_ms"]) / hip,
            "sinkhorn_ms_per_iteration": t["hip_sinkhorn_alone"]["median_ms"] / iters_sk,
            "sinkhorn_traffic": sinkhorn_bytes(b, m, n),
            "log_assignment_vs_restatement": err, "matches0_equal_fraction": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sg_bench needs the GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    cases = [case(b, 1024, 1024, it, args.iters, args.warmup, dev) for b in (32, 1) for it in (50, 100)]
    for c in cases:
        print(json.dumps({k: c[k] for k in ("B", "sinkhorn_iterations", "speedup_over_torch_restatement",
                                            "pairs_per_second", "share_sinkhorn", "share_layers")}))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "superglue_bench.json"), "w") as f:
        json.dump({"what": "SuperGlue matcher alone, 1024 + 1024 points per pair, HIP path and float32 torch restatement "
                           "alternating in one process, device events; name-seeded weights",
                   "device": torch.cuda.get_device_name(0), "library": lib_version(), "cases": cases}, f, indent=1)


def lib_version():
    return nat.lib().gfc_version().decode()


if __name__ == "__main__":
    main()
