"""EndoPatches1800 evaluation on the GPU path -- counterpart of `gluefactory.eval.endopatches1800.Endopatches1800Pipeline`
(reference gluefactory/eval/endopatches1800.py:12-67): the HPatches pipeline over the `homographies` dataset.

A folder of frames (`<data_dir>/{train,val,test}`, test frames named `<sequence>_<number>.<ext>`) -> the benchmark
schedule (sources x homography levels x photometric levels, one seed per item: `homographies.HomographyPairs`) -> every
source decoded once and its nine variants warped in ONE `gfc_warp_perspective` call (`HomographyPairFeeder`; the
reference calls cv2.warpPerspective on the host twice per pair) -> `export_predictions` with view 0 of a source extracted
once -> `predictions.h5` -> the match metrics, DLT error and (with an estimator) robust homography of `eval_hpatches`,
under the same summary names.  `get_predictions`, `run_eval`, `run` and the robust option are inherited.

    python -m glue_factory_colon_amd.eval_endopatches --data_dir /data/all_SLAM_ENE26 --photometric identity \\
        [--source_dir /data/endopatches1800_source_images] [--estimator gfc_amd]
    python -m glue_factory_colon_amd.eval_endopatches --data_dir /data/all_SLAM_ENE26 --saved /data/endopatches1800

The warp is UNPINNED against OpenCV (homographies.py, tests/warp_reference.py).  The reference's default photometric
augmentation `lg` is an albumentations pipeline that this package does not have: generating needs
`--photometric identity` (NOT the benchmark the reference publishes -- a geometric-only variant of it); the published
benchmark is evaluated from its saved form (`--saved`), whose files carry the augmentation.  No per-level tables: the
reference has none.
"""
import argparse
import json
import os
from pathlib import Path

import torch

from . import eval_utils
from .base_model import merge
from .eval_hpatches import HPatchesPipeline, build_model
from .homographies import HomographyPairs

# eval/endopatches1800.py:14-45 (the loader keys `batch_size` / `num_workers` of the reference's DataLoader are the
# pipeline's `pair_batch` / `num_workers` arguments here)
DEFAULT_DATA_CONF = {
    "name": "homographies", "data_dir": "all_SLAM_ENE26", "train_size": 150000, "val_size": 2000, "test_size": 1800,
    "test_seed": 0, "test_sequences": ["Seq_003", "Seq_016"], "test_homography_levels": [0.3, 0.5, 0.7],
    "test_photometric_levels": [0.25, 0.6, 0.95], "test_source_dir": "endopatches1800_source_images",
    "test_image_list": None, "save_dataset": False, "read_dataset_from_disk": False,
    "saved_dataset_dir": "endopatches1800", "reseed": True, "right_only": False, "left_view_difficulty": 0.0,
    "right_view_difficulty": None, "crop_vignette": True, "vignette_crop_coords": [81, 663, 55, 484],
    "photometric": {"name": "lg"},
    "homography": {"difficulty": 0.7, "max_angle": 45, "patch_shape": [580, 426]},
}


class Endopatches1800Pipeline(HPatchesPipeline):
    default_data_conf = DEFAULT_DATA_CONF

    def __init__(self, data_conf=None, data_root=None, pair_batch=36, num_workers=2, eval_conf=None):
        """data_root: what the reference calls DATA_PATH (default $GFC_DATA_PATH or the current directory): `data_dir`,
        `test_source_dir` and `saved_dataset_dir` are relative to it unless absolute.  pair_batch: a multiple of the
        variants per source keeps every source inside one batch (36 = four sources of 3 x 3 variants)."""
        self.data_root = data_root
        super().__init__(merge(self.default_data_conf, dict(data_conf or {})), pair_batch=pair_batch,
                         num_workers=num_workers, eval_conf=eval_conf)
        conf = self.dataset.conf
        if conf["test_homography_levels"] is not None and conf["test_photometric_levels"] is not None:
            # the items of a source stay on one rank: what sharing their view 0 needs
            self.shard_group = len(conf["test_homography_levels"]) * len(conf["test_photometric_levels"])

    def _get_dataset(self, data_conf):
        from .registry import get_dataset

        conf = {k: v for k, v in data_conf.items() if k != "name"}
        return get_dataset(data_conf.get("name", "homographies"))(conf, self.data_root)

    def _feeder(self):
        return self.dataset.feeder(batch=self.pair_batch, num_workers=self.num_workers, depth=max(64, 2 * self.pair_batch))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_dir", required=True, help="the image tree (train/ val/ test/ inside)")
    ap.add_argument("--saved", default=None, help="a saved benchmark (source_names.txt, <dir>/attribs.txt, ...): read it "
                                                  "instead of generating")
    ap.add_argument("--source_dir", default=None, help="test_source_dir: <dir>/<sequence>/ lists the benchmark's sources")
    ap.add_argument("--photometric", default=None, help="photometric.name (only 'identity' can be generated here)")
    ap.add_argument("--test_size", type=int, default=None)
    ap.add_argument("--sequences", nargs="*", default=None, help="test_sequences")
    ap.add_argument("--save_to", default=None, help="also write the generated benchmark in the reference's saved layout")
    ap.add_argument("--experiment_dir", default="outputs/endopatches1800")
    ap.add_argument("--extractor_weights", default="synthetic", help="local .pth (reference key names) or 'synthetic'")
    ap.add_argument("--matcher_weights", default="synthetic")
    ap.add_argument("--open", action="store_true", help="superpoint-open + in-tree lightglue instead of the official pair")
    ap.add_argument("--pair_batch", type=int, default=36)
    ap.add_argument("--num_workers", type=int, default=2, help="reader threads that decode the sources ahead of the GPU")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--estimator", default=None, choices=[None, *eval_utils.RANSAC_ESTIMATORS],
                    help="robust homography estimator for H_error_ransac* (default: none, DLT only)")
    ap.add_argument("--ransac_th", type=float, default=-1.0, help="inlier threshold in pixels; <= 0: the sweep 0.5 .. 3.0")
    args = ap.parse_args(argv)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16)))
    data_dir = Path(args.data_dir).resolve()
    conf = {"data_dir": data_dir.name}
    if args.saved is not None:
        conf.update(read_dataset_from_disk=True, saved_dataset_dir=str(Path(args.saved).resolve()), test_source_dir=None)
    else:
        conf["test_source_dir"] = None if args.source_dir is None else str(Path(args.source_dir).resolve())
    if args.photometric is not None:
        conf["photometric"] = {"name": args.photometric}
    if args.test_size is not None:
        conf["test_size"] = args.test_size
    if args.sequences is not None:
        conf["test_sequences"] = list(args.sequences)
    pipe = Endopatches1800Pipeline(conf, data_root=data_dir.parent, pair_batch=args.pair_batch,
                                   num_workers=args.num_workers,
                                   eval_conf={"estimator": args.estimator, "ransac_th": args.ransac_th} if args.estimator else None)
    if args.save_to is not None:
        pipe.dataset.save_dataset(args.save_to)
    model = build_model(args.extractor_weights, args.matcher_weights, official=not args.open).to("cuda")
    summaries, _ = pipe.run(args.experiment_dir, model, overwrite=args.overwrite)
    print(json.dumps(summaries, indent=1))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
