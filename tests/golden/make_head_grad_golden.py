"""Generate tests/golden/head_grad_{a,b}_gamma{05,0,1}.npz and head_grad_dx_{a,b}.npz: the gradients the REFERENCE's
autograd gives the assignment heads and exit tokens of LightGlue under its training loss.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_layer_loss_golden.py, whose
omegaconf stand-in it shares); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_head_grad_golden.py

What is called: gluefactory.models.matchers.lightglue.LightGlue under `.train()` with gradients enabled (checkpointed
false, flash false, CPU) on the name-seeded weights, on the two cases of tests/layer_loss_cases.py at the seeds
tests/golden/layer_loss*.npz settled on; `loss` with loss.gamma 1.0, 0.0 and 0.5, then
`torch.mean(losses["total"]).backward()` (gluefactory/train.py:1114), once in float32 and once in float64.  The whole
network has requires_grad: the parameters of log_assignment[l] enter the loss through head l only and the token reads
detached descriptors, so their .grad is the head-only gradient whatever flows into the trunk.

Stored per case and gamma (float64 run in float64, float32 run in float32, suffix _f32):
  bf [L,256], wm [L,256], bm [L], tw [L-1,256], tb [L-1]      final_proj.bias, matchability.*, token.0.* of every layer
  wf_rows [L,16,256], wf_cols [L,256,16]                      final_proj.weight.grad at `rows` / `cols` (seeded)
  wf_sumsq [L] (float64 sum of squares), wf_bilinear [L] = u^T dWf v with the stored seeded u, v (a transposed result
  changes it)
head_grad_dx_*.npz, loss.gamma 0.5: the DIRECT gradient at every layer's descriptors -- the reference's own
log_assignment[l] and loss_fn applied to detached leaf copies of ref_descriptors[:, l], the scalar mean_b(w_l nll_l /
sum_w) differentiated -- at the 16 rows per layer and side of layer_loss_cases.sample_rows, plus the sum of squares of
each layer and side.

Asserted here: the float32 and the float64 run agree on every correct0/1 target (the token gradient depends on them),
and every file stays below 1 MiB.
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

GAMMAS = {"05": 0.5, "0": 0.0, "1": 1.0}
FIXTURES = {"a": "layer_loss", "b": "layer_loss_b1"}
N_PICK = 16


def picks():
    g = torch.Generator().manual_seed(11)
    rows = torch.randperm(256, generator=g)[:N_PICK].sort().values
    cols = torch.randperm(256, generator=g)[:N_PICK].sort().values
    u = torch.randn(256, generator=g, dtype=torch.float64)
    v = torch.randn(256, generator=g, dtype=torch.float64)
    return rows, cols, u, v


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


def run(case, gamma, dtype, want_dx):
    f = lambda t: t.to(dtype)
    data = {"keypoints0": f(case["keypoints0"]), "keypoints1": f(case["keypoints1"]),
            "descriptors0": f(case["descriptors0"]), "descriptors1": f(case["descriptors1"]),
            "view0": {"image_size": f(case["size"])}, "view1": {"image_size": f(case["size"])}}
    labels = labels_of(case)
    lg = model(gamma, dtype)
    pred = lg(data)
    losses, _ = lg.loss(pred, labels)
    torch.mean(losses["total"]).backward()
    nl = lc.N_LAYERS
    rows, cols, u, v = picks()
    wf = torch.stack([lg.log_assignment[i].final_proj.weight.grad for i in range(nl)])
    out = {"bf": torch.stack([lg.log_assignment[i].final_proj.bias.grad for i in range(nl)]),
           "wm": torch.stack([lg.log_assignment[i].matchability.weight.grad.reshape(-1) for i in range(nl)]),
           "bm": torch.stack([lg.log_assignment[i].matchability.bias.grad.reshape(()) for i in range(nl)]),
           "tw": torch.stack([lg.token_confidence[i].token[0].weight.grad.reshape(-1) for i in range(nl - 1)]),
           "tb": torch.stack([lg.token_confidence[i].token[0].bias.grad.reshape(()) for i in range(nl - 1)]),
           "wf_rows": wf[:, rows], "wf_cols": wf[:, :, cols], "wf_sumsq": (wf.double() ** 2).sum((1, 2)),
           "wf_bilinear": torch.einsum("i,lij,j->l", u, wf.double(), v), "total": losses["total"].detach().double()}
    with torch.no_grad():
        las = [lg.log_assignment[i](pred["ref_descriptors0"][:, i], pred["ref_descriptors1"][:, i])[0] for i in range(nl)]
        final = las[-1]
        c0 = torch.stack([final[:, :-1, :].max(-1).indices == las[i][:, :-1, :].max(-1).indices for i in range(nl - 1)])
        c1 = torch.stack([final[:, :, :-1].max(-2).indices == las[i][:, :, :-1].max(-2).indices for i in range(nl - 1)])
    dx = None
    if want_dx:
        _, gt_weights, _ = lg.loss_fn({"log_assignment": final}, labels)
        w = [gamma ** (nl - i - 1) if gamma > 0.0 else i + 1 for i in range(nl - 1)] + [1.0]
        g0, g1 = [], []
        for i in range(nl):
            d0 = pred["ref_descriptors0"][:, i].detach().clone().requires_grad_(True)
            d1 = pred["ref_descriptors1"][:, i].detach().clone().requires_grad_(True)
            la, _ = lg.log_assignment[i](d0, d1)
            nll, _, _ = lg.loss_fn({"log_assignment": la}, labels, weights=gt_weights)
            torch.mean(nll * (w[i] / sum(w))).backward()
            g0.append(d0.grad.reshape(-1, 256))
            g1.append(d1.grad.reshape(-1, 256))
        dx = torch.stack(g0), torch.stack(g1)  # [L, B*M, 256], [L, B*N, 256]
    return out, (c0, c1), dx


def npy(t):
    return t.detach().cpu().numpy()


def main():
    rows, cols, u, v = picks()
    for name, fixture in FIXTURES.items():
        seed = int(np.load(os.path.join(HERE, fixture + ".npz"))["seed"])
        case = lc.make_case(name, seed)
        for tag, gamma in GAMMAS.items():
            want_dx = tag == "05"
            r64, t64, dx64 = run(case, gamma, torch.float64, want_dx)
            r32, t32, dx32 = run(case, gamma, torch.float32, want_dx)
            assert torch.equal(t64[0], t32[0]) and torch.equal(t64[1], t32[1]), "a correct0/1 target differs"
            arrays = {"seed": np.int64(seed), "gamma": np.float64(gamma), "input_checksum": npy(lc.input_checksum(case)),
                      "rows": npy(rows), "cols": npy(cols), "u": npy(u), "v": npy(v),
                      "correct0": npy(t64[0]), "correct1": npy(t64[1]),
                      **{k: npy(x) for k, x in r64.items()},
                      **{k + "_f32": npy(x) for k, x in r32.items()}}
            path = os.path.join(HERE, f"head_grad_{name}_gamma{tag}.npz")
            np.savez_compressed(path, **arrays)
            print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KB")
            assert os.path.getsize(path) < 1024 * 1024, "a committed file stays below 1 MiB"
            if want_dx:
                rows0, rows1 = lc.sample_rows(name)
                arrays = {"seed": np.int64(seed), "gamma": np.float64(gamma), "rows0": npy(rows0), "rows1": npy(rows1),
                          "dx0": npy(dx64[0][:, rows0]), "dx1": npy(dx64[1][:, rows1]),
                          "dx0_sumsq": npy((dx64[0] ** 2).sum((1, 2))), "dx1_sumsq": npy((dx64[1] ** 2).sum((1, 2))),
                          "dx0_f32": npy(dx32[0][:, rows0]), "dx1_f32": npy(dx32[1][:, rows1]),
                          "dx0_sumsq_f32": npy((dx32[0].double() ** 2).sum((1, 2))),
                          "dx1_sumsq_f32": npy((dx32[1].double() ** 2).sum((1, 2)))}
                path = os.path.join(HERE, f"head_grad_dx_{name}.npz")
                np.savez_compressed(path, **arrays)
                print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KB")
                assert os.path.getsize(path) < 1024 * 1024, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
