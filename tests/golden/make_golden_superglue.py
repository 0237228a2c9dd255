"""Generate tests/golden/superglue.npz and superglue_1024.npz by running the REFERENCE's own SuperGlue class.

Runs only where a checkout of the reference exists (its path in GFC_REFERENCE); the tests read the committed .npz
files, never the reference.  The class is constructed with `weights: None` (no download) and loads
glue_factory_colon_amd.weights.superglue_state_dict(0); `omegaconf` comes from tests/golden/_standins.

    GFC_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_superglue.py

Inputs come from tests/superglue_reference.make_inputs (the tests re-run it: only the seed is stored).  Stored:
  * the two small shapes (superglue.npz): every output in full; of the descriptors after the encoder, after layer 0
    (self), after layer 1 (cross) and after the last layer, TAP_ROWS evenly spaced packed rows each -- the full
    sets would be 3.9 MB, and no file here may pass 1 MiB;
  * 1024 x 1024, B = 2, 100 iterations (superglue_1024.npz): matches, matching scores, 16 sampled rows and 16 sampled
    columns of log_assignment in full, the sum and the absolute sum of every row;
  * per shape the reference's own fp32-against-float64 error, max |la32 - la64| / (1 + |la64|), from the same class
    under .double().
It also prints the conditions tests/test_superglue_reference_host.py asserts.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GFC_REFERENCE")
if not REF:
    raise SystemExit("set GFC_REFERENCE to a checkout of the reference (glue-factory with gluefactory_nonfree)")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gluefactory_nonfree.superglue as ref_sg  # noqa: E402

import superglue_reference as sgr  # noqa: E402
from glue_factory_colon_amd import weights  # noqa: E402

torch.set_grad_enabled(False)
SEED = 0
TAP_ROWS = 16
SAMPLES_1024 = 16


def make_model(iters, dtype):
    m = ref_sg.SuperGlue({"weights": None, "num_sinkhorn_iterations": iters}).eval()
    m.load_state_dict(weights.superglue_state_dict(0), strict=True)
    return m.to(dtype)


def run(model, inp, dtype):
    data = sgr.as_data(inp)
    data = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.items()}
    for side in ("0", "1"):
        data["view" + side] = {k: v.to(dtype) for k, v in data["view" + side].items()}
    return model(data)


def taps(model, inp):
    """The descriptors after the encoder, layer 0, layer 1 and the last layer from the reference's own sub-modules,
    called in the order of its `_forward` (superglue.py:281-292), as packed rows [B*M + B*N, 256]."""
    size = inp["image_size"]
    kp0 = ref_sg.normalize_keypoints(inp["keypoints0"], size=size)
    kp1 = ref_sg.normalize_keypoints(inp["keypoints1"], size=size)
    d0 = inp["descriptors0"].transpose(-1, -2) + model.kenc(kp0, inp["keypoint_scores0"])
    d1 = inp["descriptors1"].transpose(-1, -2) + model.kenc(kp1, inp["keypoint_scores1"])

    def packed():
        return torch.cat([d0.transpose(-1, -2).reshape(-1, 256), d1.transpose(-1, -2).reshape(-1, 256)], 0)

    out = [packed()]
    for i, (layer, name) in enumerate(zip(model.gnn.layers, model.gnn.names)):
        layer.attn.prob = []
        delta0, delta1 = model.gnn._forward(layer, d0, d1, name)
        d0, d1 = d0 + delta0, d1 + delta1
        if i < 2:
            out.append(packed())
    out.append(packed())
    return out


def tap_rows(rows):
    return torch.linspace(0, rows - 1, TAP_ROWS).round().long()


def main():
    small, big = {"seed": np.array(SEED)}, {"seed": np.array(SEED)}
    for b, m, n, iters in sgr.SHAPES:
        tag = f"{m}x{n}"
        inp = sgr.make_inputs(SEED, b, m, n)
        model = make_model(iters, torch.float32)
        out = run(model, inp, torch.float32)
        out64 = run(make_model(iters, torch.float64), inp, torch.float64)
        la, la64 = out["log_assignment"], out64["log_assignment"]
        err = float(((la.double() - la64).abs() / (1 + la64.abs())).max())
        cond = sgr.conditions(out, inp["gt0"], 0.2)
        print(f"{tag}: B {b}, {iters} iterations, reference fp32 vs float64 {err:.2e}, conditions {cond}")
        dst = big if m >= 1024 else small
        dst[f"{tag}/ref_fp32_error"] = np.array(err)
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
            dst[f"{tag}/{k}"] = out[k].numpy()
        if m >= 1024:
            g = torch.Generator().manual_seed(SEED)
            rows = torch.randperm(m + 1, generator=g)[:SAMPLES_1024].sort().values
            cols = torch.randperm(n + 1, generator=g)[:SAMPLES_1024].sort().values
            dst[f"{tag}/rows"], dst[f"{tag}/cols"] = rows.numpy(), cols.numpy()
            dst[f"{tag}/la_rows"] = la[:, rows].numpy()
            dst[f"{tag}/la_cols"] = la[:, :, cols].numpy()
            dst[f"{tag}/la_row_sum"] = la.sum(2).numpy()
            dst[f"{tag}/la_row_abs_sum"] = la.abs().sum(2).numpy()
        else:
            dst[f"{tag}/sinkhorn_cost"] = out["sinkhorn_cost"].numpy()
            dst[f"{tag}/log_assignment"] = la.numpy()
            t = taps(model, inp)
            # the sub-module sequence above is the class's own forward: its last tap must reproduce the class's cost
            md0 = model.final_proj(t[3][: b * m].reshape(b, m, 256).transpose(1, 2))
            md1 = model.final_proj(t[3][b * m:].reshape(b, n, 256).transpose(1, 2))
            assert torch.equal(torch.einsum("bdn,bdm->bnm", md0, md1) / 16, out["sinkhorn_cost"])
            idx = tap_rows(b * (m + n))
            dst[f"{tag}/tap_rows"] = idx.numpy()
            dst[f"{tag}/taps"] = torch.stack([x[idx] for x in t]).numpy()
    for name, arrays in (("superglue", small), ("superglue_1024", big)):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(f"{name}: {size / 1024:.0f} KB, keys={sorted(arrays)}")
        assert size <= 1 << 20, "a committed file may not pass 1 MiB"
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
