"""Record how much of its per-element bound (tests/cross_attn_grad_reference.py) every output of the cross-attention
backward uses, per shape: the core alone and the block entry, on the shapes and cases of
tests/test_gpu_cross_attn_backward.py, against the float64 closed form on the same bits.

    python tools/cross_attn_backward_parity.py --out profiles  ->  profiles/cross_attn_backward_parity.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cross_attn_grad_reference as car  # noqa: E402
import test_gpu_cross_attn_backward as t  # noqa: E402


def core_fractions(qk, v, ctx, dctx, shape):
    dev = [x.to(t.DEV) for x in (qk, v, ctx, dctx)]
    got = t.run_core(*dev, shape)
    want, errs = car.attention_backward(*(x.double() for x in dev), *shape)
    tol = car.bounds(errs)
    return {k: car.worst_ratio(g, want[k], tol[k]) for k, g in zip(("dqk", "dv"), got)}


def block_fractions(shape):
    x, ctx, dctx, dx_in, p = t.random_block(shape, 40 + sum(shape))
    full, att = t.run_block(x, ctx, dctx, dx_in, p, shape), t.run_block(x, ctx, dctx, None, p, shape)
    want, errs = car.backward(x.double(), ctx.double(), dctx.double(), dx_in.double(), car.to64(p), *shape)
    tol = car.bounds(errs)
    got = dict(full, dx_att=att["dx"])
    return {k: car.worst_ratio(got[k], want[k], tol[k]) for k in car.OUTPUTS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    args = ap.parse_args()
    name = lambda s: "x".join(map(str, s))  # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "unit": "largest |got - float64| / bound over the elements",
           "core": {name(s): core_fractions(*car.random_core(*s, seed=sum(s)), s) for s in t.SHAPES},
           "core_cases": {"identical_keys": core_fractions(*car.identical_keys_case()),
                          "dominant_key": core_fractions(*car.dominant_key_case()[:5])},
           "block": {name(s): block_fractions(s) for s in ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 700, 1400))}}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "cross_attn_backward_parity.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
