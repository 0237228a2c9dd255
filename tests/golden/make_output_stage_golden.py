"""Generate tests/golden/output_stage_{a,b}_gamma{05,1}.npz: the gradients the REFERENCE's autograd gives the output stage
of LightGlue's last layer (`transformers[L-1].cross_attn.{to_out, ffn}`) under its training loss, and the gradient at
that block's attention context.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_head_grad_golden.py, whose
omegaconf stand-in it shares); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_output_stage_golden.py

What is called: gluefactory.models.matchers.lightglue.LightGlue under `.train()` with gradients enabled (checkpointed
false, flash false, CPU) on the name-seeded weights, on the two cases of tests/layer_loss_cases.py at the seeds
tests/golden/layer_loss*.npz settled on; `loss` with loss.gamma 0.5 and 1.0, then
`torch.mean(losses["total"]).backward()` (gluefactory/train.py:1114), once in float32 and once in float64.  The whole
network has requires_grad.  A forward pre-hook on the last `to_out` keeps its two inputs (the attention context of side
0, then of side 1) with `retain_grad()`: the context feeds nothing but `to_out`, so its .grad is dctx.

Stored per case and gamma (float64 run in float64, float32 run in float32, suffix _f32):
  bout [256], b0 [512], gamma_ [512], beta [512], b3 [256]     the bias / LayerNorm gradients in full
  {wout,w0,w3}_rows [16,cols], _cols [rows,16]                 the weight gradients at seeded rows / columns
  {wout,w0,w3}_sumsq (float64 sum of squares), _bilinear = u^T dW v with the stored seeded u, v (a transposed result
  changes it)
  dctx0 [16,256], dctx1 [16,256]                               dctx at the rows of layer_loss_cases.sample_rows
Asserted here: every file stays below 1 MiB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GFC_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gluefactory.models.matchers import lightglue as ref_lg  # noqa: E402

import layer_loss_cases as lc  # noqa: E402
from glue_factory_colon_amd import weights  # noqa: E402

GAMMAS = {"05": 0.5, "1": 1.0}
FIXTURES = {"a": "layer_loss", "b": "layer_loss_b1"}
N_PICK = 16
WEIGHTS = {"wout": ("to_out", 256, 256), "w0": ("ffn.0", 512, 512), "w3": ("ffn.3", 256, 512)}


def picks():
    """{name: (rows, cols, u, v)} for the three weight gradients, seeded."""
    g = torch.Generator().manual_seed(13)
    out = {}
    for name, (_, r, c) in WEIGHTS.items():
        out[name] = (torch.randperm(r, generator=g)[:N_PICK].sort().values,
                     torch.randperm(c, generator=g)[:N_PICK].sort().values,
                     torch.randn(r, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64))
    return out


def model(gamma, dtype):
    lg = ref_lg.LightGlue({"input_dim": 256, "filter_threshold": 0.0, "checkpointed": False, "flash": False,
                           "n_layers": lc.N_LAYERS, "loss": {"gamma": gamma, "fn": "nll", "nll_balancing": 0.5}})
    lg.load_state_dict(weights.lightglue_state_dict(0), strict=False)
    return lg.to(dtype).train()


def labels_of(case):
    ga = case["gt_assignment"]
    if ga is None:  # the reference's nll_loss reads gt_assignment; the labels without one name the same positives
        g0 = case["gt_matches0"]
        ga = torch.zeros(g0.shape + (case["gt_matches1"].shape[1],), dtype=torch.bool)
        bi, ii = torch.nonzero(g0 > -1, as_tuple=True)
        ga[bi, ii, g0[bi, ii]] = True
    return {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"], "gt_assignment": ga}


def run(name, case, gamma, dtype):
    f = lambda t: t.to(dtype)  # noqa: E731
    data = {"keypoints0": f(case["keypoints0"]), "keypoints1": f(case["keypoints1"]),
            "descriptors0": f(case["descriptors0"]), "descriptors1": f(case["descriptors1"]),
            "view0": {"image_size": f(case["size"])}, "view1": {"image_size": f(case["size"])}}
    lg = model(gamma, dtype)
    ca = lg.transformers[lc.N_LAYERS - 1].cross_attn
    contexts = []

    def keep(_, args):
        args[0].retain_grad()
        contexts.append(args[0])

    handle = ca.to_out.register_forward_pre_hook(keep)
    pred = lg(data)
    handle.remove()
    losses, _ = lg.loss(pred, labels_of(case))
    torch.mean(losses["total"]).backward()
    assert len(contexts) == 2
    rows0, rows1 = lc.sample_rows(name)
    sub = ca.get_submodule
    out = {"bout": ca.to_out.bias.grad, "b0": sub("ffn.0").bias.grad, "gamma_": sub("ffn.1").weight.grad,
           "beta": sub("ffn.1").bias.grad, "b3": sub("ffn.3").bias.grad,
           "dctx0": contexts[0].grad.reshape(-1, 256)[rows0], "dctx1": contexts[1].grad.reshape(-1, 256)[rows1],
           "total": losses["total"].detach().double()}
    for key, (rows, cols, u, v) in picks().items():
        g = sub(WEIGHTS[key][0]).weight.grad
        out[key + "_rows"], out[key + "_cols"] = g[rows], g[:, cols]
        out[key + "_sumsq"] = (g.double() ** 2).sum()
        out[key + "_bilinear"] = u @ g.double() @ v
    return out


def npy(t):
    return t.detach().cpu().numpy()


def main():
    for name, fixture in FIXTURES.items():
        seed = int(np.load(os.path.join(HERE, fixture + ".npz"))["seed"])
        case = lc.make_case(name, seed)
        rows0, rows1 = lc.sample_rows(name)
        for tag, gamma in GAMMAS.items():
            r64, r32 = run(name, case, gamma, torch.float64), run(name, case, gamma, torch.float32)
            arrays = {"seed": np.int64(seed), "gamma": np.float64(gamma), "input_checksum": npy(lc.input_checksum(case)),
                      "rows0": npy(rows0), "rows1": npy(rows1),
                      **{k: npy(x) for k, x in r64.items()}, **{k + "_f32": npy(x) for k, x in r32.items()}}
            for key, (rows, cols, u, v) in picks().items():
                arrays.update({key + "_pick_rows": npy(rows), key + "_pick_cols": npy(cols), key + "_u": npy(u),
                               key + "_v": npy(v)})
            path = os.path.join(HERE, f"output_stage_{name}_gamma{tag}.npz")
            np.savez_compressed(path, **arrays)
            print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KB")
            assert os.path.getsize(path) < 1024 * 1024, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
