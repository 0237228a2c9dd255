"""Generate tests/golden/cross_attn_grad_{a,b}_gamma{05,1}.npz: the gradients the REFERENCE's autograd gives `to_qk` and
`to_v` of LightGlue's last cross block (`transformers[L-1].cross_attn`) under its training loss, and the gradient at the
rows that block reads.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_output_stage_golden.py, whose
cases, seeds, stand-in and gammas it shares); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cross_attn_grad_golden.py

What is called: gluefactory.models.matchers.lightglue.LightGlue under `.train()` with gradients enabled (checkpointed
false, flash false, CPU) on the name-seeded weights, on the two cases of tests/layer_loss_cases.py; `loss` with
loss.gamma 0.5 and 1.0, then `torch.mean(losses["total"]).backward()` (gluefactory/train.py:1114), once in float32 and
once in float64.  The whole network has requires_grad.  A forward pre-hook on the last `cross_attn` keeps its two inputs
(the rows of side 0 and of side 1 after the self block) with `retain_grad()`: their .grad is the COMPLETE gradient at the
rows the last cross block reads.

Stored per case and gamma (float64 run in float64, float32 run in float32, suffix _f32):
  bqk [256], bv [256]                                   the bias gradients in full
  {wqk,wv}_rows [16,256], _cols [256,16]                the weight gradients at seeded rows / columns
  {wqk,wv}_sumsq (float64 sum of squares), _bilinear = u^T dW v with the stored seeded u, v (a transposed result changes
  it)
  dx0 [16,256], dx1 [16,256]                            the gradient at the block's input rows, at the rows of
                                                        layer_loss_cases.sample_rows
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
WEIGHTS = {"wqk": "to_qk", "wv": "to_v"}


def picks():
    """{name: (rows, cols, u, v)} for the two weight gradients, seeded."""
    g = torch.Generator().manual_seed(29)
    out = {}
    for name in WEIGHTS:
        out[name] = (torch.randperm(256, generator=g)[:N_PICK].sort().values,
                     torch.randperm(256, generator=g)[:N_PICK].sort().values,
                     torch.randn(256, generator=g, dtype=torch.float64), torch.randn(256, generator=g, dtype=torch.float64))
    return out


def run(name, case, gamma, dtype):
    f = lambda t: t.to(dtype)  # noqa: E731
    data = {"keypoints0": f(case["keypoints0"]), "keypoints1": f(case["keypoints1"]),
            "descriptors0": f(case["descriptors0"]), "descriptors1": f(case["descriptors1"]),
            "view0": {"image_size": f(case["size"])}, "view1": {"image_size": f(case["size"])}}
    lg = mos.model(gamma, dtype)
    ca = lg.transformers[lc.N_LAYERS - 1].cross_attn
    kept = []

    def keep(_, args):
        for t in args[:2]:
            t.retain_grad()
            kept.append(t)

    handle = ca.register_forward_pre_hook(keep)
    pred = lg(data)
    handle.remove()
    losses, _ = lg.loss(pred, mos.labels_of(case))
    torch.mean(losses["total"]).backward()
    assert len(kept) == 2
    rows0, rows1 = lc.sample_rows(name)
    out = {"bqk": ca.to_qk.bias.grad, "bv": ca.to_v.bias.grad,
           "dx0": kept[0].grad.reshape(-1, 256)[rows0], "dx1": kept[1].grad.reshape(-1, 256)[rows1],
           "total": losses["total"].detach().double()}
    for key, (rows, cols, u, v) in picks().items():
        g = ca.get_submodule(WEIGHTS[key]).weight.grad
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
            path = os.path.join(HERE, f"cross_attn_grad_{name}_gamma{tag}.npz")
            np.savez_compressed(path, **arrays)
            print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KB")
            assert os.path.getsize(path) < 1024 * 1024, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
