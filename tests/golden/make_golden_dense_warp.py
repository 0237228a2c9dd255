"""Generate tests/golden/dense_warp.npz by running the REFERENCE's own cycle_dist and gt_matches_from_roma on CPU.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_golden_hpatches.py, whose
empty `kornia` / `cv2` modules and `_standins` it shares by importing it); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dense_warp.py [--seed S]

What is called: cycle_dist (gluefactory/utils/image.py:260-270), as the reference's RoMa module calls it with
add_cycle_error (cycle_error0 = cycle_dist(warp0, warp1), cycle_error1 = cycle_dist(warp1, warp0)), and
gt_matches_from_roma (gluefactory/geometry/gt_generation.py:61-269), each on float32 inputs and on `.double()` inputs.

Cases `c<k>` = dense_warp_reference.CASES (key points m x n, the field of warp1): inputs of make_case -- images of
120 x 160 and 96 x 128, warp0 of 48 x 64, planted blocks, NaN / inf pixels, key points on the borders, padded key
points.  The fields of case 0 serve every case (stored once); a case has its own key points.
Settings `s<k>` = dense_warp_reference.SETTINGS.  The script walks seeds until float32 and float64 agree on every integer,
mask, `assignment` and `reward`, the restatement equals the float64 run and flags NOTHING undecided.
Stored: the inputs (float32), the reference's float32 integers and masks, `assignment` with numpy.packbits, `reward` as
int8, and its float32 and float64 floats (proj, certainty_kp, cycle_error_kp, scores; the cycle fields of case 0).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden_hpatches as mh  # noqa: E402,F401  (sets up sys.modules / sys.path for the reference)

sys.path.insert(0, os.path.join(ROOT, "tests"))
from gluefactory.geometry.gt_generation import gt_matches_from_roma  # noqa: E402
from gluefactory.utils.image import cycle_dist  # noqa: E402

import dense_warp_reference as dr  # noqa: E402

torch.set_grad_enabled(False)
INT_KEYS = ("matches0", "matches1") + tuple(k + s for k in dr.MASK_KEYS for s in "01")
FLOAT_KEYS = ("proj_0to1", "proj_1to0", "certainty_kp0", "certainty_kp1", "cycle_error_kp0", "cycle_error_kp1",
              "matching_scores0", "matching_scores1")
FIELD_KEYS = ("warp0", "warp1", "certainty0", "certainty1")
INPUT_KEYS = ("kp0", "kp1", "scores0", "scores1", "warp0", "warp1", "certainty0", "certainty1")


def run(case, setting, dtype):
    pos, neg, pc, pcy, nc, ncy, with_cycle = setting
    f = lambda k: case[k].to(dtype)  # noqa: E731
    data = {"view0": {"image": torch.empty((1, 1) + case["img0_hw"])}, "view1": {"image": torch.empty((1, 1) + case["img1_hw"])}}
    cyc = {}
    if with_cycle:
        cyc = {"cycle_error0": cycle_dist(f("warp0"), f("warp1")), "cycle_error1": cycle_dist(f("warp1"), f("warp0"))}
    r = gt_matches_from_roma(f("kp0"), f("kp1"), data, valid0=case["scores0"] > 0, valid1=case["scores1"] > 0,
                             warp0=f("warp0"), warp1=f("warp1"), certainty0=f("certainty0"), certainty1=f("certainty1"),
                             pos_th=pos, neg_th=neg, pos_cert_th=pc, pos_cycle_error_th=pcy, neg_cert_th=nc,
                             neg_cycle_error_th=ncy, **cyc)
    assert len(r) == 20
    return {k: v[0] for k, v in r.items()}, {k: v[0] for k, v in cyc.items()}


def same_floats(a, b, tol):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and bool(((a - b).abs().nan_to_num(nan=0.0, posinf=0.0) <= tol).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    out = {"settings": np.array([[-1.0 if v is None else float(v) for v in s] for s in dr.SETTINGS])}
    for c, (m, n, field1) in enumerate(dr.CASES):
        seed = args.seed
        while True:
            case = dr.make_case(seed * 100 + c, 1, m, n, field1=field1)
            if c > 0:  # one set of fields for every case: only case 0 stores them
                case.update({k: first[k] for k in FIELD_KEYS})
            ok, results = True, {}
            for s, setting in enumerate(dr.SETTINGS):
                r64, cyc64 = run(case, setting, torch.float64)
                chk = dr.run(case, setting)
                und = int(chk["undecided0"].sum()) + int(chk["undecided1"].sum()) + int(chk["undecided_dense"].sum())
                agree = all(torch.equal(chk[k], r64[k]) for k in INT_KEYS + ("assignment",)) and \
                    torch.equal(chk["reward"], r64["reward"]) and \
                    all(same_floats(chk[k], r64[k], 1e-9) for k in FLOAT_KEYS)
                if cyc64:
                    agree = agree and same_floats(dr.cycle_dist(case["warp0"][0].double(), case["warp1"][0].double())[0],
                                                  cyc64["cycle_error0"], 1e-9)
                assert agree, "the restatement differs from the reference"
                if und:
                    print(f"c{c} seed {seed} s{s}: undecided {und}", flush=True)
                    ok = False
                    break
                r32, cyc32 = run(case, setting, torch.float32)
                same = all(torch.equal(r32[k], r64[k]) for k in INT_KEYS + ("assignment",)) and \
                    torch.equal(r32["reward"].double(), r64["reward"])
                g0 = r32["matches0"]
                print(f"c{c} seed {seed} s{s}: same {same}, matches0 match/unmatched/ignore {int((g0 > -1).sum())}/"
                      f"{int((g0 == -1).sum())}/{int((g0 == -2).sum())}, masks "
                      f"{[int(r32[k].sum()) for k in INT_KEYS[2:]]}", flush=True)
                ok = ok and same
                results[s] = (r32, r64, cyc32, cyc64)
                if not ok:
                    break
            if ok:
                break
            seed += 1
        pre = f"c{c}_"
        out[pre + "seed"] = np.int64(seed)
        out[pre + "hw"] = np.array([case["img0_hw"], case["img1_hw"]])
        if c == 0:
            first = case
        for k in INPUT_KEYS:
            if c == 0 or k not in FIELD_KEYS:
                out[pre + k] = case[k][0].numpy()
        for s, (r32, r64, cyc32, cyc64) in results.items():
            tag = f"{pre}s{s}_"
            for k in INT_KEYS:
                out[tag + k] = r32[k].numpy()
            out[tag + "assignment"] = np.packbits(r32["assignment"].numpy())
            out[tag + "reward"] = r32["reward"].numpy().astype(np.int8)
            if s < 2:  # the floats do not depend on the thresholds, only on whether the cycle fields exist; scores do
                for k in FLOAT_KEYS[:6]:
                    out[tag + k + "_f32"], out[tag + k + "_f64"] = r32[k].numpy(), r64[k].numpy()
            for k in FLOAT_KEYS[6:]:
                out[tag + k + "_f32"], out[tag + k + "_f64"] = r32[k].numpy(), r64[k].numpy()
            if s == 0 and c == 0:
                for k in cyc32:
                    out[pre + k + "_f32"], out[pre + k + "_f64"] = cyc32[k].numpy(), cyc64[k].numpy()
    path = os.path.join(HERE, "dense_warp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; sparse_map.npz has", os.path.getsize(os.path.join(HERE, "sparse_map.npz")))


if __name__ == "__main__":
    main()
