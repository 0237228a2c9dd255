"""Record how much of its per-element bound (tests/self_block_grad_reference.py) every output of the self-attention
backward uses, per shape: the core alone and the block entry, on the shapes and cases of
tests/test_gpu_self_attn_backward.py, against the float64 closed form on the same bits -- and ONE hash over the outputs
of the earlier backward entries, to compare with a build of the parent commit.

    python tools/self_block_backward_parity.py --out profiles [--parent TREE]  ->  profiles/self_block_backward_parity.json

The hash (sha256 over the bytes of every output, in a fixed order) covers gfc_lg_ffn_backward at its test's 13 row counts
x 2 weight sets, gfc_lg_cross_attn_backward at its test's 4 shapes (with dx_in), gfc_lg_head_backward at its test's 17
shapes, and layer_loss_backward(output_stage=True, cross_attention=True, descriptor_grads=True, accumulate=False) on both
cases of tests/layer_loss_cases.py at loss.gamma 0.5 and 1.  With --parent TREE (a checkout of the parent commit with its
library built inside it; tools/ab_build.sh builds the library) the same code runs once more in a fresh process on that
tree's package, tests and library, and the JSON says whether the two hashes are equal.
    python tools/self_block_backward_parity.py --hash-only TREE     prints the hash of TREE (what the child runs)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def use_tree(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))


def earlier_hash():
    """The hash described above, on the tree that is on sys.path."""
    import numpy as np
    import torch

    import layer_loss_cases as lc
    import output_stage_reference as osr
    import test_gpu_cross_attn_backward as tc
    import test_gpu_cross_attn_module as tm
    import test_gpu_ffn_backward as tf
    import test_gpu_head_backward as th

    h = hashlib.sha256()
    count = 0

    def add(tag, outs):
        nonlocal count
        for k in sorted(outs):
            if outs[k] is not None:
                h.update(f"{tag}/{k}".encode() + outs[k].detach().contiguous().cpu().numpy().tobytes())
                count += 1

    for with_out in (True, False):
        p = tf.on_device(osr.random_params(torch.Generator().manual_seed(7 + with_out), with_out))
        for r in tf.ROWS:
            x, ctx, dy = (t.to(tf.DEV) for t in tf.random_rows(r, 100 + r))
            add(f"ffn {r} {with_out}", tf.run(x, ctx, dy, p))
    for shape in ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 700, 1400)):
        x, ctx, dctx, dx_in, p = tc.random_block(shape, 40 + sum(shape))
        add(f"cross {shape}", tc.run_block(x, ctx, dctx, dx_in, p, shape))
    _, params = th.shared_model()
    for b, m, n in th.SHAPES:
        x0, x1 = th.rows(b, m, 1, 3.0), th.rows(b, n, 2, 3.0)
        gt0, gt1, gta = th.make_labels(b, m, n, 3, "assignment" if m % 2 else "mixed")
        g = torch.tensor([0.7, 0.0, -0.4][:b]) if b == 3 else torch.full((b,), 1.0 / b)
        add(f"head {b} {m} {n}", th.run_head(params, 3, x0, x1, gt0, gt1, gta, g, 0.5))
    seed = int(np.load(os.path.join(tm.GOLDEN, "layer_loss.npz"))["seed"])
    for name in ("a", "b"):
        case = lc.make_case(name, seed)
        for gamma in (0.5, 1.0):
            lg = tm.model(loss={"gamma": gamma})
            with torch.no_grad():
                pred = lg.forward_layers(tm.inputs(case), keep_output_stage=True)
            add(f"module {name} {gamma}", lg.layer_loss_backward(pred, tm.labels(case), accumulate=False, output_stage=True,
                                                                  cross_attention=True, descriptor_grads=True))
    torch.cuda.synchronize()
    return {"sha256": h.hexdigest(), "tensors": count}


def fractions():
    import torch

    import self_block_grad_reference as sbr
    import test_gpu_self_attn_backward as t

    def core(qkv, ctx, dctx, cos, sin, shape):
        dev = [None if x is None else x.to(t.DEV).contiguous() for x in (qkv, ctx, dctx, cos, sin)]
        got = t.run_core(*dev, shape)
        want, errs = sbr.attention_backward(*(None if x is None else x.double() for x in dev), *shape)
        tol = sbr.U * errs
        return {k: sbr.worst_ratio(got[:, c:c + 256], want[:, c:c + 256], tol[:, c:c + 256])
                for k, c in (("dq", 0), ("dk", 256), ("dv", 512))}

    def block(shape):
        x, cos, sin, ctx, dctx, dx_in, w, bias = (v.to(t.DEV) for v in sbr.random_block(*shape, seed=40 + sum(shape)))
        full = t.run_block(x, cos, sin, ctx, dctx, dx_in, w, bias, shape)
        att = t.run_block(x, cos, sin, ctx, dctx, None, w, bias, shape)
        d = lambda v: v.double()  # noqa: E731
        want, errs = sbr.backward(d(x), d(cos), d(sin), d(ctx), d(dctx), d(dx_in), d(w), d(bias), *shape)
        tol = sbr.bounds(errs)
        got = dict(full, dx_att=att["dx"])
        return {k: sbr.worst_ratio(got[k], want[k], tol[k]) for k in sbr.OUTPUTS}

    name = lambda s: "x".join(map(str, s))  # noqa: E731
    ik, dk = sbr.identical_keys_case(), sbr.dominant_key_case()
    return {"device": torch.cuda.get_device_name(0), "unit": "largest |got - float64| / bound over the elements",
            "core": {name(s): core(*sbr.random_core(*s, seed=sum(s)), s) for s in t.SHAPES},
            "core_cases": {"general_tables": core(*sbr.random_core(2, 70, 45, seed=21, equal_pairs=False), (2, 70, 45)),
                           "identical_keys": core(*ik[:3], None, None, ik[3]),
                           "dominant_key": core(*dk[:3], None, None, dk[3])},
            "block": {name(s): block(s) for s in ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 700, 1400))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built inside it")
    ap.add_argument("--hash-only", default=None, metavar="TREE")
    args = ap.parse_args()
    if args.hash_only:
        use_tree(os.path.abspath(args.hash_only))
        print("HASH " + json.dumps(earlier_hash()))
        return
    use_tree(os.path.dirname(HERE))
    res = fractions()
    res["earlier_entries_hash"] = {"this": earlier_hash()}
    if args.parent:
        env = {k: v for k, v in os.environ.items() if k != "GFC_AMD_LIB"}
        parent = os.path.abspath(args.parent)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--hash-only", parent], capture_output=True,
                           text=True, env=env, cwd=parent)
        line = [x for x in r.stdout.splitlines() if x.startswith("HASH ")]
        if r.returncode or not line:
            raise RuntimeError(f"the parent's run failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        res["earlier_entries_hash"]["parent"] = json.loads(line[0][5:])
        res["earlier_entries_hash"]["equal"] = res["earlier_entries_hash"]["parent"] == res["earlier_entries_hash"]["this"]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "self_block_backward_parity.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
