"""Generate tests/golden/validation.npz by running the REFERENCE's own validation code on CPU.

Runs only on the build machine, where the reference checkout exists (GFC_REFERENCE, as make_golden_hpatches.py, whose
empty `kornia` / `cv2` modules and `_standins` it shares by importing it); the tests read the committed .npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_validation.py [--seed S]

What is called: gt_matches_from_homography, NLLLoss.forward, matcher_metrics, and LightGlue.loss in eval mode on the
name-seeded weights -- each on float32 inputs and on `.double()` inputs (suffix _f64).

Ground-truth cases `gt_<name>_*` (key points as in make_golden_hpatches.py):
  exact    5 x 4      pos_th = neg_th = 3, dist == pos_th^2 exactly (case 4 there): the one case on a threshold
  130x67              pos_th = neg_th = 3
  twins    300 x 257  pos_th 3 < neg_th 6, bit-identical twins on both sides (case 2 there)
  masks    130 x 67   pos_th 3 < neg_th 5, valid0 / valid1 masks; rows 10..19 of image 0 all invalid
  65x1, 1x65          pos_th = neg_th = 3
The script walks seeds until, in every case but `exact`, float32 and float64 agree on every integer output, on
assignment and on reward, and tests/validation_reference.py flags NOTHING undecided (key points and dense elements).
Loss cases `loss_<name>_*`: tests/validation_cases.py LOSS_CASES (unique top score or none above zero); stored are the
random inputs and the reference's ten values in validation_reference.OUT_KEYS order (ref32 / ref64).
Depth cases `depth_<c>_<branch>_<epi>_*`: the three pairs of tests/golden/pose_depth.npz (PINHOLE, OPENCV,
OPENCV_FISHEYE; 257 x 130 key points) through gt_matches_from_pose_depth with epi_th None (`n`) and 5 (`e`), depth
`sampled` from the maps for all three, and for pair 0 also `cached` (depth_keypoints + a thinned valid mask) and `anded`
(a valid mask ANDed with the sampled validity); stored: matches0/1, assignment, reward, visible0/1 and the masks
given.  float32 and float64 must agree on all of them.
`ap_<name>_*`: validation_cases.ap_cases (small random and degenerate inputs of ranking_ap) and the reference's value.
`lg_*`: one 300 + 257 pair (case 3 of make_golden_hpatches.py, descriptors from validation_cases.descriptors_for)
through the reference LightGlue (9 layers, filter_threshold 0) and its eval-mode `loss` against the
homography_matcher labels (3 / 3): matches0, the eight losses and four metrics.
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
import make_golden_hpatches as mh  # noqa: E402  (sets up sys.modules / sys.path for the reference)

sys.path.insert(0, ROOT)
from gluefactory.geometry.gt_generation import gt_matches_from_homography  # noqa: E402
from gluefactory.models.matchers import lightglue as ref_lg  # noqa: E402
from gluefactory.models.utils.losses import NLLLoss  # noqa: E402
from gluefactory.models.utils.metrics import matcher_metrics  # noqa: E402

import hpatches_reference as hr  # noqa: E402
import validation_cases as vc  # noqa: E402
import validation_reference as vr  # noqa: E402
from glue_factory_colon_amd import weights  # noqa: E402

torch.set_grad_enabled(False)
GT_CASES = (("exact", None, 3.0, 3.0), ("130x67", 0, 3.0, 3.0), ("twins", 2, 3.0, 6.0), ("masks", 1, 3.0, 5.0),
            ("65x1", None, 3.0, 3.0), ("1x65", None, 3.0, 3.0))
GT_KEYS = ("matches0", "matches1", "assignment", "reward", "proj_0to1", "proj_1to0")


def gt_case(name, c, seed):
    if name == "exact":
        case = mh.exact_case()
    elif c is not None:
        case = mh.make_case(seed, c)
    else:  # one key point against 65: the single one is the partner of number 7
        g = torch.Generator().manual_seed(seed * 10 + 7)
        H = mh.homography(g, 1)
        kp0 = torch.rand((65, 2), generator=g) * mh.SIZE
        kp1 = hr.warp(kp0[7:8].double(), H.double(), 1e-5).float() + 0.5
        case = {"H": H, "kp0": kp0, "kp1": kp1}
        if name == "1x65":
            case = {"H": torch.linalg.inv(H.double()).float(), "kp0": kp1, "kp1": kp0}
    out = {"H": case["H"], "kp0": case["kp0"], "kp1": case["kp1"]}
    if name == "masks":
        g = torch.Generator().manual_seed(seed * 10 + 9)
        out["valid0"] = torch.rand(out["kp0"].shape[0], generator=g) > 0.2
        out["valid0"][10:20] = False
        out["valid1"] = torch.rand(out["kp1"].shape[0], generator=g) > 0.2
    if name == "twins":
        out.update(dup0=case["dup0"], dup1=case["dup1"], dup_row=case["dup_row"])
    return out


def run_gt(case, pos, neg, dtype):
    v0, v1 = case.get("valid0"), case.get("valid1")
    r = gt_matches_from_homography(case["kp0"][None].to(dtype), case["kp1"][None].to(dtype), case["H"][None].to(dtype),
                                   pos_th=pos, neg_th=neg, valid_mask0=None if v0 is None else v0[None],
                                   valid_mask1=None if v1 is None else v1[None])
    return {k: r[k][0] for k in GT_KEYS}


def run_loss(case, dtype):
    la = vc.la_of(case["la_q"])[None].to(dtype)
    data = {"gt_matches0": case["gt0"][None], "gt_matches1": case["gt1"][None], "gt_assignment": case["assignment"][None]}
    pred = {"log_assignment": la, "matches0": case["m0"][None], "matching_scores0": case["scores0"][None].to(dtype)}
    nll, _, lm = NLLLoss({}).forward(pred, data)
    mm = matcher_metrics(pred, data)
    row_norm = la.exp()[:, :-1].sum(2).mean(1)
    vals = [lm["nll_pos"], lm["nll_neg"], lm["num_matchable"], lm["num_unmatchable"], lm["assignment_nll"], row_norm,
            mm["match_recall"], mm["match_precision"], mm["accuracy"], mm["average_precision"]]
    assert torch.equal(nll, lm["assignment_nll"])
    return torch.stack([v[0].double() for v in vals])


def depth_cases():
    import make_golden_pose as mp
    from gluefactory.geometry.gt_generation import gt_matches_from_pose_depth
    from gluefactory.geometry.wrappers import Pose

    fx = np.load(os.path.join(HERE, "pose_depth.npz"))
    out = {}
    for c, model in enumerate(fx["models"]):
        t = lambda k: torch.from_numpy(fx[k][c])  # noqa: E731

        def run(dtype, epi_th, kw):
            data = {"view0": {"camera": mp.ref_camera(t("cam0")[None], str(model), dtype), "depth": t("depth0")[None].to(dtype)},
                    "view1": {"camera": mp.ref_camera(t("cam1")[None], str(model), dtype), "depth": t("depth1")[None].to(dtype)},
                    "T_0to1": Pose(t("T_0to1")[None].to(dtype))}
            kw = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in kw.items()}
            return gt_matches_from_pose_depth(t("kp0")[None].to(dtype), t("kp1")[None].to(dtype), data, pos_th=3.0,
                                              neg_th=5.0, epi_th=epi_th, **kw)

        thin0 = t("valid0") & (torch.arange(mp.M) % 7 != 3)
        thin1 = t("valid1") & (torch.arange(mp.N) % 7 != 3)
        branches = {"sampled": {}}
        if c == 0:
            branches["cached"] = {"depth_keypoints0": t("depth_kp0")[None], "valid_depth_keypoints0": thin0[None],
                                  "depth_keypoints1": t("depth_kp1")[None], "valid_depth_keypoints1": thin1[None]}
            branches["anded"] = {"valid_depth_keypoints0": (torch.arange(mp.M) % 5 != 2)[None],
                                 "valid_depth_keypoints1": (torch.arange(mp.N) % 5 != 2)[None]}
        for bname, kw in branches.items():
            for tag, epi_th in (("n", None), ("e", 5.0)):
                r32, r64 = run(torch.float32, epi_th, kw), run(torch.float64, epi_th, kw)
                keys = ("matches0", "matches1", "assignment", "reward", "visible0", "visible1")
                same = all(torch.equal(r32[k].double(), r64[k].double()) for k in keys)
                g0 = r32["matches0"][0]
                print(f"depth {c} {model} {bname} {tag}: same {same}, matches0 match/unmatched/ignore "
                      f"{int((g0 > -1).sum())}/{int((g0 == -1).sum())}/{int((g0 == -2).sum())}, "
                      f"reward -1/0/1 {[int((r32['reward'] == v).sum()) for v in (-1, 0, 1)]}")
                assert same, (c, bname, tag)
                for k in keys:
                    out[f"depth_{c}_{bname}_{tag}_{k}"] = r32[k][0].numpy()
            for k, v in kw.items():
                if k.startswith("valid"):
                    out[f"depth_{c}_{bname}_{k}"] = v[0].numpy()
    return out


def lightglue_case(seed):
    while True:  # labels no float32 evaluation can move: nothing undecided
        case = mh.make_case(seed, 3)
        kp0, kp1, H = case["kp0"], case["kp1"], case["H"]
        chk = vr.gt_matches_homography(kp0.double(), kp1.double(), H.double(), 3.0, 3.0)
        if int(chk["undecided0"].sum()) + int(chk["undecided1"].sum()) == 0:
            break
        seed += 1
    back = hr.warp(kp1.double(), torch.linalg.inv(H.double()))
    d0, d1 = vc.descriptors_for(kp0), vc.descriptors_for(kp1, partner=back)
    lg = ref_lg.LightGlue({"input_dim": 256, "filter_threshold": 0.0}).eval()
    lg.load_state_dict(weights.lightglue_state_dict(0), strict=False)
    size = mh.SIZE[None]
    data = {"keypoints0": kp0[None], "keypoints1": kp1[None], "descriptors0": d0[None], "descriptors1": d1[None],
            "view0": {"image_size": size}, "view1": {"image_size": size}}
    pred = lg(data)
    gt = gt_matches_from_homography(kp0[None], kp1[None], H[None], pos_th=3.0, neg_th=3.0)
    losses, metrics = lg.loss(pred, {**data, **pred, **{f"gt_{k}": v for k, v in gt.items()}})
    out = {"lg_H": H, "lg_kp0": kp0, "lg_kp1": kp1, "lg_matches0": pred["matches0"][0],
           "lg_gt_matches0": gt["matches0"][0], "lg_gt_matches1": gt["matches1"][0]}
    for k, v in {**losses, **metrics}.items():
        out[f"lg_{k}"] = v[0]
    print("lightglue:", {k: float(v[0]) for k, v in {**losses, **metrics}.items()},
          "matches", int((pred["matches0"] > -1).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    out = {}
    for name, c, pos, neg in GT_CASES:
        seed = args.seed
        while True:
            case = gt_case(name, c, seed)
            r32, r64 = run_gt(case, pos, neg, torch.float32), run_gt(case, pos, neg, torch.float64)
            same = all(torch.equal(r32[k].double(), r64[k].double()) for k in GT_KEYS[:4])
            chk = vr.gt_matches_homography(case["kp0"].double(), case["kp1"].double(), case["H"].double(), pos, neg,
                                           case.get("valid0"), case.get("valid1"))
            und = int(chk["undecided0"].sum()) + int(chk["undecided1"].sum()) + int(chk["undecided_dense"].sum())
            if name == "exact" or (same and und == 0):
                break
            seed += 1
        assert same, name
        g0 = r32["matches0"]
        print(f"gt {name}: seed {seed}, matches0 match/unmatched/ignore "
              f"{int((g0 > -1).sum())}/{int((g0 == -1).sum())}/{int((g0 == -2).sum())}, undecided {und}")
        out[f"gt_{name}_seed"] = np.int64(seed)
        out[f"gt_{name}_th"] = np.array([pos, neg])
        for k, v in {**case, **r32}.items():
            out[f"gt_{name}_{k}"] = v.numpy()
        for k in ("proj_0to1", "proj_1to0"):
            out[f"gt_{name}_{k}_f64"] = r64[k].numpy()
    for name, m, n, kind in vc.LOSS_CASES:
        case = vc.loss_case(args.seed * 100 + len(name) + m, m, n, kind)
        top = case["scores0"].max()
        assert float(top) == 0.0 or int((case["scores0"] == top).sum()) == 1, name
        r32, r64 = run_loss(case, torch.float32), run_loss(case, torch.float64)
        print(f"loss {name}:", [round(float(v), 5) for v in r32])
        for k, v in case.items():
            out[f"loss_{name}_{k}"] = v.numpy()
        out[f"loss_{name}_ref32"], out[f"loss_{name}_ref64"] = r32.numpy(), r64.numpy()
    for name, m, gt, s in vc.ap_cases():
        ap = matcher_metrics({"matches0": m[None], "matching_scores0": s[None]}, {"gt_matches0": gt[None]})
        print(f"ap {name}: {float(ap['average_precision'][0]):.6f}")
        out[f"ap_{name}_m"], out[f"ap_{name}_gt"], out[f"ap_{name}_scores"] = m.numpy(), gt.numpy(), s.numpy()
        out[f"ap_{name}_ref"] = ap["average_precision"][0].numpy()
    out.update(depth_cases())
    out.update({k: v.numpy() for k, v in lightglue_case(args.seed).items()})
    path = os.path.join(HERE, "validation.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
