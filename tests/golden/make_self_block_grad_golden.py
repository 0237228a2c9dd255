"""Generate tests/golden/self_block_grad_{a,b}_gamma{05,1}.npz: the gradients the REFERENCE's autograd gives the ten
tensors of LightGlue's last self block (`transformers[L-1].self_attn`) under its training loss, and the gradient at the
rows that block reads.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_output_stage_golden.py, whose
cases, seeds, stand-in and gammas it shares); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_self_block_grad_golden.py

What is called: gluefactory.models.matchers.lightglue.LightGlue under `.train()` with gradients enabled (checkpointed
false, flash false, CPU) on the name-seeded weights, on the two cases of tests/layer_loss_cases.py; `loss` with
loss.gamma 0.5 and 1.0, then `torch.mean(losses["total"]).backward()` (gluefactory/train.py:1114), once in float32 and
once in float64.  The whole network has requires_grad.  A forward pre-hook on the last `self_attn` keeps its input for
both of its calls (side 0, then side 1) with `retain_grad()`: their .grad is the COMPLETE gradient at the rows the last
layer reads, head L - 2's direct share included.

Stored per case and gamma (float64 run in float64, float32 run in float32, suffix _f32):
  bqkv [768], bout [256], b0 [512], gamma_ [512], beta [512], b3 [256]   the bias and LayerNorm gradients in full
  {wqkv,wout,w0,w3}_rows [16,cols], _cols [rows,16]     the weight gradients at seeded rows / columns (state-dict order)
  {..}_sumsq (float64 sum of squares), _bilinear = u^T dW v with the stored seeded u, v (a transposed or row-permuted
  result changes it)
  dx0 [16,256], dx1 [16,256]                            the kept inputs' .grad at the rows of layer_loss_cases.sample_rows
Asserted here: every file stays below 1 MiB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_output_stage_golden as mos  # noqa: E402  (the paths, the model, the labels, the cases)

lc = mos.lc
N_PICK = mos.N_PICK
WEIGHTS = {"wqkv": ("Wqkv", 768, 256), "wout": ("out_proj", 256, 256), "w0": ("ffn.0", 512, 512), "w3": ("ffn.3", 256, 512)}


def picks():
    """{name: (rows, cols, u, v)} for the four weight gradients, seeded."""
    g = torch.Generator().manual_seed(31)
    out = {}
    for name, (_, r, c) in WEIGHTS.items():
        out[name] = (torch.randperm(r, generator=g)[:N_PICK].sort().values,
                     torch.randperm(c, generator=g)[:N_PICK].sort().values,
                     torch.randn(r, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64))
    return out


def run(name, case, gamma, dtype):
    f = lambda t: t.to(dtype)  # noqa: E731
    data = {"keypoints0": f(case["keypoints0"]), "keypoints1": f(case["keypoints1"]),
            "descriptors0": f(case["descriptors0"]), "descriptors1": f(case["descriptors1"]),
            "view0": {"image_size": f(case["size"])}, "view1": {"image_size": f(case["size"])}}
    lg = mos.model(gamma, dtype)
    sa = lg.transformers[lc.N_LAYERS - 1].self_attn
    kept = []

    def keep(_, args):
        args[0].retain_grad()
        kept.append(args[0])

    handle = sa.register_forward_pre_hook(keep)
    pred = lg(data)
    handle.remove()
    losses, _ = lg.loss(pred, mos.labels_of(case))
    torch.mean(losses["total"]).backward()
    assert len(kept) == 2 and kept[0].shape[1] == case["keypoints0"].shape[1]
    rows0, rows1 = lc.sample_rows(name)
    sub = sa.get_submodule
    out = {"bqkv": sa.Wqkv.bias.grad, "bout": sa.out_proj.bias.grad, "b0": sub("ffn.0").bias.grad,
           "gamma_": sub("ffn.1").weight.grad, "beta": sub("ffn.1").bias.grad, "b3": sub("ffn.3").bias.grad,
           "dx0": kept[0].grad.reshape(-1, 256)[rows0], "dx1": kept[1].grad.reshape(-1, 256)[rows1],
           "total": losses["total"].detach().double()}
    for key, (rows, cols, u, v) in picks().items():
        g = sub(WEIGHTS[key][0]).weight.grad
        out[key + "_rows"], out[key + "_cols"] = g[rows], g[:, cols]
        out[key + "_sumsq"] = (g.double() ** 2).sum()
        out[key + "_bilinear"] = u @ g.double() @ v
    return out


def main():
    npy = mos.npy
    for name, fixture in mos.FIXTURES.items():
        seed = int(np.load(os.path.join(HERE, fixture + ".npz"))["seed"])
        case = lc.make_case(name, seed)
        rows0, rows1 = lc.sample_rows(name)
        for tag, gamma in mos.GAMMAS.items():
            r64, r32 = run(name, case, gamma, torch.float64), run(name, case, gamma, torch.float32)
            arrays = {"seed": np.int64(seed), "gamma": np.float64(gamma), "input_checksum": npy(lc.input_checksum(case)),
                      "rows0": npy(rows0), "rows1": npy(rows1),
                      **{k: npy(x) for k, x in r64.items()}, **{k + "_f32": npy(x) for k, x in r32.items()}}
            for key, (rows, cols, u, v) in picks().items():
                arrays.update({key + "_pick_rows": npy(rows), key + "_pick_cols": npy(cols), key + "_u": npy(u),
                               key + "_v": npy(v)})
            path = os.path.join(HERE, f"self_block_grad_{name}_gamma{tag}.npz")
            np.savez_compressed(path, **arrays)
            print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KB")
            assert os.path.getsize(path) < 1024 * 1024, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
