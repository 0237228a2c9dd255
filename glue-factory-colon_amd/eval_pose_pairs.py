"""Pose / depth evaluation of cached predictions on the GPU path -- counterpart of the `run_eval` of the reference's
posed-pair benchmarks (gluefactory/eval/endomapper_dense1500.py:102-183; megadepth1500, scannet1500 and eth3d share its
shape): per pair the match counts, `eval_matches_epipolar`, `eval_matches_depth` when the item carries depth, and the robust
relative pose per RANSAC threshold with the pose AUCs at the best one: through `eval_relative_pose_robust` given an
estimator object, or -- `eval_conf = {"estimator": "gfc_amd", ...}` and no object -- through ONE call of the GPU
five-point RANSAC (`eval_utils.relative_pose_ransac`) per group of pairs for all thresholds.

`items` is any iterable of the reference's data dicts, one pair each (`name`, `T_0to1`, `view0/1` = {`camera`
[, `depth`]}, cameras and poses as geometry.Camera / Pose or the reference's wrappers).  The reference walks them pair
by pair; here consecutive items of equal shapes (key-point counts, depth-map sizes, camera models) go through ONE call
of each kernel (one workgroup per pair either way: the numbers do not depend on the grouping).

From a dataset on disk: `posed_images.PosedImages` reads the directory, `PosedPairFeeder` prepares images, depth and
masks on the GPU, `get_predictions` exports `predictions.h5` and `run` evaluates it:

    python -m glue_factory_colon_amd.eval_pose_pairs --data_dir /data --benchmark megadepth1500 \\
        --extractor_weights superpoint_v6_from_tf.pth --matcher_weights superpoint_lightglue.pth --estimator gfc_amd

What is NOT here: figures, and the `image_pairs` list reader the reference's scannet1500 is configured with (its
settings are kept below; the command line refuses it).  Parity of the GPU estimator with OpenCV / PoseLib / pycolmap
(what the reference delegates to) is unpinned; so is the reader against the reference's own class (posed_images.py).
"""
import argparse
import json
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from . import eval_utils, geometry
from .cache_loader import CacheLoader
from .eval_hpatches import CONTEXT_KEYS, MEMORY_KEYS, TIMING_KEYS, med_mean_summaries

MIN_MATCHES_FOR_POSE = 5
EXPORT_KEYS = ["keypoints0", "keypoints1", "keypoint_scores0", "keypoint_scores1", "matches0", "matches1",
               "matching_scores0", "matching_scores1"]
OPTIONAL_EXPORT_KEYS = [*TIMING_KEYS, *MEMORY_KEYS, *CONTEXT_KEYS]
# default_conf["data"] of the reference's pipelines (eval/megadepth1500.py:47-59, eval/scannet1500.py:28-37,
# eval/endomapper_dense1500.py:43-56); "name" is the reference's dataset class
BENCHMARK_DATA = {
    "megadepth1500": {"name": "posed_images", "root": "", "image_dir": "{scene}/images", "depth_dir": "{scene}/depths",
                      "views": "{scene}/views.txt", "view_groups": "{scene}/pairs.txt", "depth_format": "h5",
                      "scene_list": ["megadepth1500"], "preprocessing": {"side": "long"}},
    "scannet1500": {"name": "image_pairs", "pairs": "scannet1500/pairs_calibrated.txt", "root": "scannet1500/",
                    "extra_data": "relative_pose", "preprocessing": {"side": "long"}, "num_workers": 14},
    "endomapper_dense1500": {"name": "posed_images", "root": "", "image_dir": "{scene}/images",
                             "depth_dir": "{scene}/depths", "views": "{scene}/views.txt",
                             "view_groups": "{scene}/pairs.txt", "depth_format": "npz", "crop_endomapper_dense": True,
                             "depth_scale_scene_info_dir": "endomapper_dense/scene_info", "read_specular_mask": True,
                             "specular_scene_info_dir": "endomapper_dense/scene_info",
                             "scene_list": ["endomapper_dense1500"]},
}


def _name(item):
    return item["name"][0] if isinstance(item["name"], (list, tuple)) else item["name"]


def _stack_holder(holders):
    first = holders[0]
    data = torch.cat([h._data.reshape(-1, h._data.shape[-1]) for h in holders], 0)
    if hasattr(first, "model"):
        out = geometry.Camera(data, model=first.model)
    else:
        out = geometry.Pose(data)
    return out


class PosePairsPipeline:
    export_keys = EXPORT_KEYS
    optional_export_keys = OPTIONAL_EXPORT_KEYS

    def __init__(self, eval_conf=None, max_group=64, pair_batch=1):
        self.eval_conf = {"estimator": None, "ransac_th": 1.0, **dict(eval_conf or {})}
        self.max_group = int(max_group)
        self.pair_batch = max(1, int(pair_batch))

    def get_predictions(self, experiment_dir, model, feeder, overwrite=False):
        """endomapper_dense1500.py:87-100: `predictions.h5` of every pair of `feeder` (a `PosedPairFeeder`, or any
        iterable of loader items), `pair_batch` consecutive pairs per forward."""
        from .export_predictions import export_predictions

        pred_file = Path(experiment_dir) / "predictions.h5"
        if not pred_file.exists() or overwrite:
            export_predictions(feeder, model, pred_file, keys=self.export_keys, optional_keys=self.optional_export_keys,
                               pair_batch=self.pair_batch)
        return pred_file

    def run(self, experiment_dir, model, feeder, overwrite=False):
        """Predictions (all ranks), then the evaluation and `summaries.json` on rank 0.  Returns (summaries, results) on
        rank 0, (None, None) elsewhere."""
        import torch.distributed as dist

        pred_file = self.get_predictions(experiment_dir, model, feeder, overwrite=overwrite)
        if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
            return None, None
        summaries, results = self.run_eval(feeder, pred_file)
        with open(Path(experiment_dir) / "summaries.json", "w") as f:
            json.dump(summaries, f, indent=1)
        return summaries, results

    def thresholds(self):
        """endomapper_dense1500.py:107-111: a positive number -> that one, a non-positive one -> the sweep."""
        th = self.eval_conf["ransac_th"]
        if isinstance(th, (list, tuple, np.ndarray)):
            return [float(t) for t in th]
        return [float(th)] if float(th) > 0 else [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]

    def _flush(self, group, device, out, pose_out=None):
        datas, preds = zip(*[g[:2] for g in group])

        def stack(key, dtype):
            return torch.stack([p[key] for p in preds]).to(device=device, dtype=dtype)

        kp0, kp1, m0 = stack("keypoints0", torch.float32), stack("keypoints1", torch.float32), stack("matches0", torch.long)
        cam0 = _stack_holder([d["view0"]["camera"] for d in datas])
        cam1 = _stack_holder([d["view1"]["camera"] for d in datas])
        T = _stack_holder([d["T_0to1"] for d in datas])
        epi = eval_utils.pose_epipolar_metrics(kp0, kp1, m0, cam0, cam1, T).cpu()
        dep = None
        if "depth" in datas[0]["view0"]:
            depth0 = torch.cat([d["view0"]["depth"].reshape((-1,) + tuple(d["view0"]["depth"].shape[-2:])) for d in datas])
            depth1 = torch.cat([d["view1"]["depth"].reshape((-1,) + tuple(d["view1"]["depth"].shape[-2:])) for d in datas])
            dep = eval_utils.pose_depth_metrics(kp0, kp1, m0, depth0, depth1, cam0, cam1, T).cpu()
        for j in range(len(group)):
            row = {key: (int(epi[j, c]) if key == "num_matches" else float(epi[j, c]))
                   for c, key in enumerate(eval_utils.EPIPOLAR_RESULT_KEYS)}
            if dep is not None:
                row.update({key: float(dep[j, c]) for c, key in enumerate(eval_utils.DEPTH_RESULT_KEYS)})
            out.append(row)
        if pose_out is not None:
            self._pose_rows(group, kp0, kp1, m0, cam0, cam1, pose_out)

    def _pose_rows(self, group, kp0, kp1, m0, cam0, cam1, pose_out):
        """One estimator call for the whole group and all thresholds; stream_id = the pair's position in `items`.
        Matches are counted as `matches0 > -1`, as `eval_relative_pose_robust` and the reference select them; the
        kernel additionally wants `matches0 < N`, which every valid prediction satisfies."""
        ths = self.thresholds()
        conf = self.eval_conf
        res = eval_utils.relative_pose_ransac(
            kp0, kp1, m0, cam0, cam1, ths, num_hypotheses=conf.get("num_hypotheses", 2048),
            lo_iters=conf.get("lo_iters", 3), seed=conf.get("seed", 0), stream_id=[g[2] for g in group])
        R, t, succ, ninl = res["R"].cpu(), res["t"].cpu(), res["success"].cpu(), res["num_inliers"].cpu()
        n_matches = (m0 > -1).sum(1).cpu().tolist()
        for j, (data, _, _) in enumerate(group):
            for q, th in enumerate(ths):
                if n_matches[j] < MIN_MATCHES_FOR_POSE:
                    row = {k: float("nan") for k in eval_utils.POSE_RESULT_KEYS}
                elif not bool(succ[j, q]):
                    row = {"rel_pose_error": float("inf"), "ransac_inl": 0, "ransac_inl%": 0}
                else:
                    t_err, r_err = eval_utils.relative_pose_error(data["T_0to1"], R[j, q], t[j, q])
                    row = {"rel_pose_error": float(max(r_err, t_err)), "ransac_inl": float(ninl[j, q]),
                           "ransac_inl%": float(ninl[j, q]) / n_matches[j]}
                for k, v in row.items():
                    pose_out[th][k].append(v)

    @staticmethod
    def _shape_key(data, pred):
        views = tuple((geometry.model_id(data[v]["camera"]),
                       tuple(data[v]["depth"].shape[-2:]) if "depth" in data[v] else None) for v in ("view0", "view1"))
        return (pred["keypoints0"].shape[0], pred["keypoints1"].shape[0], views)

    def run_eval(self, items, pred_file, estimator=None, device="cuda"):
        """-> (summaries, results): per-pair lists under the reference's keys, `med_*` / `mean_*` of every numeric
        one; with an estimator (an object, or eval_conf["estimator"] = "gfc_amd") also `rel_pose_error@{5,10,20}°`,
        `rel_pose_error_mAA` and the per-pair pose lists at the best threshold (every tested threshold under
        results["pose_results"]).  An eval_conf["estimator"] name this package does not have, with no estimator
        object, raises NotImplementedError (no pose would be computed)."""
        named = estimator is None and self.eval_conf["estimator"] is not None
        if named and self.eval_conf["estimator"] not in eval_utils.RELATIVE_POSE_ESTIMATORS:
            eval_utils.relative_pose_estimator_from_conf(self.eval_conf)  # raises: no such estimator here
        cache = CacheLoader({"path": str(pred_file), "collate": None, "add_data_path": False}).eval()
        rows, extras, names = [], [], []
        pose_results = defaultdict(lambda: defaultdict(list))
        group, key = [], None
        for data in items:
            name = _name(data)
            pred = cache({"name": [name], "view0": {"scales": data["view0"].get("scales", torch.ones(1, 2))},
                          "view1": {"scales": data["view1"].get("scales", torch.ones(1, 2))}})
            k = self._shape_key(data, pred)
            if group and (k != key or len(group) >= self.max_group):
                self._flush(group, device, rows, pose_results if named else None)
                group = []
            key = k
            group.append((data, pred, len(names)))
            names.append(name)
            extras.append({q: pred[q].item() for q in (*TIMING_KEYS, *MEMORY_KEYS, *CONTEXT_KEYS) if q in pred})
            if estimator is not None:
                n_matches = int((pred["matches0"] > -1).sum())
                for th in self.thresholds():
                    if n_matches < MIN_MATCHES_FOR_POSE:
                        res = {q: float("nan") for q in eval_utils.POSE_RESULT_KEYS}
                    else:
                        res = eval_utils.eval_relative_pose_robust(
                            data, pred, {"estimator": self.eval_conf["estimator"], "ransac_th": th}, estimator=estimator)
                    for q, v in res.items():
                        pose_results[th][q].append(v)
        if group:
            self._flush(group, device, rows, pose_results if named else None)
        results = defaultdict(list)
        for row, extra, name in zip(rows, extras, names):
            for q, v in {**row, **extra, "names": name}.items():
                results[q].append(v)
        summaries = med_mean_summaries(results)
        results = dict(results)
        if (estimator is not None or named) and pose_results:
            pose_results = {th: dict(r) for th, r in pose_results.items()}
            pose_summaries, best_th = eval_utils.eval_poses(pose_results, auc_ths=[5, 10, 20], key="rel_pose_error")
            results = {**results, **pose_results[best_th], "pose_results": pose_results}
            summaries = {**summaries, **pose_summaries}
        return summaries, results


def main(argv=None):
    from . import posed_images
    from .eval_hpatches import build_model

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_dir", required=True, help="the directory the benchmark's `root` is relative to")
    ap.add_argument("--benchmark", required=True, choices=sorted(BENCHMARK_DATA))
    ap.add_argument("--experiment_dir", default=None, help="default: outputs/<benchmark>")
    ap.add_argument("--extractor_weights", default="synthetic", help="local .pth (reference key names) or 'synthetic'")
    ap.add_argument("--matcher_weights", default="synthetic")
    ap.add_argument("--open", action="store_true", help="superpoint-open + in-tree lightglue instead of the official pair")
    ap.add_argument("--max_num_keypoints", type=int, default=2048)
    ap.add_argument("--resize", type=int, default=None, help="preprocessing.resize (the benchmarks leave it unset)")
    ap.add_argument("--estimator", default=None, choices=[None, *eval_utils.RELATIVE_POSE_ESTIMATORS],
                    help="robust relative-pose estimator for rel_pose_error* (default: none)")
    ap.add_argument("--ransac_th", type=float, default=1.0, help="inlier threshold in pixels; <= 0: the sweep 0.5 .. 3.0")
    ap.add_argument("--pair_batch", type=int, default=8)
    ap.add_argument("--overwrite", action="store_true")
    args = ap.parse_args(argv)
    data_conf = {k: v for k, v in BENCHMARK_DATA[args.benchmark].items()}
    if data_conf.pop("name") != "posed_images":
        raise NotImplementedError(f"{args.benchmark}: the reference reads it through its `image_pairs` dataset, which is "
                                  "not built here; a `posed_images` directory (views.txt, pairs.txt) is")
    if args.resize is not None:
        data_conf["preprocessing"] = {**data_conf.get("preprocessing", {}), "resize": args.resize}
    experiment_dir = Path(args.experiment_dir or f"outputs/{args.benchmark}")
    experiment_dir.mkdir(parents=True, exist_ok=True)
    dataset = posed_images.PosedImages(data_conf, args.data_dir)
    pipe = PosePairsPipeline({"estimator": args.estimator, "ransac_th": args.ransac_th}, pair_batch=args.pair_batch)
    model = build_model(args.extractor_weights, args.matcher_weights, official=not args.open,
                        max_num_keypoints=args.max_num_keypoints).to("cuda")
    summaries, _ = pipe.run(experiment_dir, model, dataset.feeder("cuda"), overwrite=args.overwrite)
    print(json.dumps(summaries, indent=1))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
