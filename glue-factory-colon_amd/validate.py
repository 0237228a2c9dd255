"""Validation pass on the GPU: the reference's `do_evaluation` (gluefactory/train.py:100-304) without plots and PR
curves -- `model.eval()`, the prediction of every pair, `losses, metrics = model.loss(pred, data)`, the mean of
every `metrics` key and of `loss/<key>` over the pairs (AverageMetric: NaNs left out), and on request the per-pair TSV
of the fork (`step index name overlap precision recall accuracy ap`, train.py:163-249).

    python -m glue_factory_colon_amd.validate --data_dir D --dataset {homographies,posed_images,endomapper}
                                              [--split val] [--pair_batch N] [--log_metrics FILE]

The pairs run through `TwoViewPipeline.forward_pairs` in batches of `pair_batch`; inside a batch the pairs of equal
(M, N) form one group: ONE ground-truth call and ONE loss call (`TwoViewPipeline.loss` on the stacked group, the
ground truth with `dense_outputs: False`, so no [M,N] label matrix exists) and ONE device-to-host read.
`homographies` pairs (a `HomographyPairFeeder`) carry `H_0to1` and take matchers.homography_matcher; `posed_images`
pairs (a `PosedPairFeeder`) carry cameras, depth maps and `T_0to1` and take matchers.depth_matcher (`--th_epi`); a group
of posed pairs also shares its depth-map sizes and camera model.
`endomapper` pairs (an `EndomapperFeeder`: cached CudaSift features, no extractor, no depth map) take
matchers.sparse_depth_matcher (`use_gt_pos true, th_positive null, th_negative 10`, as the fork's configuration) or
matchers.sparse_dense_depth_matcher; the label inputs that come out of the cache are stacked next to the prediction.
The labels run without the dense matrices, so the sum of `extra_positives` -- positives of the reference's dense
`assignment` that `matches0` cannot name -- rides in the group's one read and is reported as `gt_extra_positives`.
`--eval_overlap_bins "0:0.2,0.2:0.4"`: the reference's overlap bins (train.py:123-143, 280-299), returned under "bins".
`--layer_report`: every group goes through the matcher's `forward_layers` and `layer_loss` instead of its forward and
`loss` (still one read per group): the summary gains `loss/confidence`, `loss/total_deep` (the reference's training-mode
total) and a per-layer table -- nll, recall and precision of the layer's own matches, agreement with the final layer,
token BCE and the share of points confident at the layer (what `depth_confidence` is compared with) -- and the TSV gains
those columns after the existing ones.  Without the flag nothing changes.
"""
import argparse
import math
import os
import sys
from pathlib import Path

import torch

from .base_model import merge
from .two_view_pipeline import TwoViewPipeline

DEFAULT_MODEL_CONF = {
    "extractor": {"name": "extractors.superpoint_open", "weights": "synthetic", "max_num_keypoints": 512,
                  "detection_threshold": 0.0, "nms_radius": 3},
    "matcher": {"name": "matchers.lightglue", "weights": "synthetic", "filter_threshold": 0.1, "flash": False},
    "ground_truth": {"name": "matchers.homography_matcher", "th_positive": 3, "th_negative": 3, "dense_outputs": False},
    "profile_calls": False,
}
TSV_HEADER = "step\tindex\tname\toverlap\tprecision\trecall\taccuracy\tap\n"
# --layer_report: per layer (all L) and per layer but the last (the token heads), in the TSV and in the summary table
LAYER_KEYS = ("nll", "recall", "precision")
TOKEN_KEYS = ("agree", "token_bce", "ratio_confident")
MATCHER_INPUT_KEYS = ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "scales0", "scales1", "oris0", "oris1")
GROUP_PRED_KEYS = ("keypoints0", "keypoints1", "log_assignment", "matches0", "matching_scores0")
# what a view's cache hands to the ground truth (suffixed 0 / 1 in the prediction): stacked with the group when present
GROUP_LABEL_KEYS = ("sparse_depth", "valid_depth_mask", "valid_3D_mask", "point3D_ids", "depth_keypoints",
                    "valid_depth_keypoints")
ENDOMAPPER_MODEL_CONF = {"extractor": {"name": None}, "allow_no_extract": True,
                         "matcher": {"add_scale_ori": True, "input_dim": 128}}
SPARSE_GROUND_TRUTH = {"name": "matchers.sparse_depth_matcher", "use_gt_pos": True, "th_positive": None,
                       "th_negative": 10, "th_epi": None, "dense_outputs": False}
DEPTH_GROUND_TRUTH = {"name": "matchers.depth_matcher", "th_positive": 3, "th_negative": 5, "th_epi": None,
                      "dense_outputs": False}


class AverageMetric:
    """gluefactory/utils/tools.py:17-32: the mean of everything it was given, NaNs left out; NaN for nothing."""

    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, values):
        for v in values:
            if not math.isnan(v):
                self.sum += v
                self.count += 1

    def compute(self):
        return self.sum / self.count if self.count else float("nan")


def overlap_bins(spec):
    """train.py:123-143: [(low, high, name)] from "low:high,low:high" or [[low, high], ...]; the overall bin
    (min low, max high) is appended unless it is there already.  None / empty -> None."""
    if not spec:
        return None
    if isinstance(spec, str):
        spec = [part.split(":") for part in spec.split(",") if part.strip()]
    bins = []
    for bounds in spec:
        if bounds is None or len(bounds) != 2:
            raise ValueError("eval_overlap_bins must contain [min, max] pairs.")
        bins.append((float(bounds[0]), float(bounds[1])))
    lows, highs = zip(*bins)
    overall = (min(lows), max(highs))
    if overall not in bins:
        bins.append(overall)
    return [(low, high, f"overlap_{low:.2f}_{high:.2f}") for low, high in bins]


def bin_results(bins, overlaps, rows):
    """train.py:280-299: per bin the mean of every key over the pairs with low <= overlap < high (NaNs left out); a bin
    without pairs is left out.  overlaps: one float per pair (NaN: in no bin); rows: one {key: value} per pair."""
    out = {}
    for low, high, name in bins or []:
        members = [r for o, r in zip(overlaps, rows) if low <= o < high]
        if not members:
            continue
        bucket = {}
        for r in members:
            for k, v in r.items():
                bucket.setdefault(k, AverageMetric()).update([v])
        out[name] = {k: m.compute() for k, m in bucket.items()}
    return out


def _overlap(item):
    overlap = item.get("overlap_0to1")
    return float("nan") if overlap is None else float(torch.as_tensor(overlap).reshape(-1)[0])


class ValidationPipeline:
    def __init__(self, model_conf=None, pair_batch=32, device="cuda", eval_overlap_bins=None, layer_report=False):
        self.bins = overlap_bins(eval_overlap_bins)
        self.layer_report = bool(layer_report)
        self.model = TwoViewPipeline(merge(DEFAULT_MODEL_CONF, dict(model_conf or {}))).eval().to(device)
        if not hasattr(self.model, "ground_truth"):
            raise ValueError("the validation pass needs a ground_truth component")
        self.pair_batch = max(1, int(pair_batch))
        self.device = torch.device(device)
        self.reads = 0  # device-to-host reads so far: one per group
        # --layer_report: (key of a pair's row, column name) behind the existing TSV columns; none without the flag
        self._extra = []
        if self.layer_report:
            nl = int(self.model.matcher.conf.n_layers)
            self._extra = [("loss/confidence", "confidence"), ("loss/total_deep", "total_deep")] + [
                (f"layer/{i}/{k}", f"{k}_{i}") for i in range(nl) for k in LAYER_KEYS] + [
                (f"layer/{i}/{k}", f"{k}_{i}") for i in range(nl - 1) for k in TOKEN_KEYS]

    def _group_loss(self, datas, preds):
        """`model.loss` of pairs with equal (M, N), stacked: ({key: [G] values}, keys) after ONE device-to-host read."""
        label_keys = tuple(k + s for k in GROUP_LABEL_KEYS for s in "01" if k + s in preds[0])
        # (with --layer_report the pairs come without the matcher's keys: `_layer_numbers` runs it on the group)
        pred = {k: torch.cat([p[k] for p in preds], 0) for k in GROUP_PRED_KEYS + label_keys
                if not self.layer_report or k in preds[0]}
        data = self._group_data(datas)
        if self.layer_report:
            numbers = self._layer_numbers(datas, preds, pred, data)
        else:
            losses, metrics = self.model.loss(pred, data)
            numbers = {**metrics, **{"loss/" + k: v for k, v in losses.items()}}
        keys = list(numbers)
        rows = [numbers[k].float() for k in keys]
        extra = pred.get("gt_extra_positives")  # the sparse-map matchers without dense outputs
        if extra is not None:
            rows.append(extra.float())
        host = torch.stack(rows, 0).cpu()
        self.reads += 1
        if extra is not None:
            self.extra_positives = (self.extra_positives or 0) + int(host[-1].sum())
        return {k: host[i].tolist() for i, k in enumerate(keys)}

    def _forward_layers(self, stacked):
        """The matcher's `forward_layers` on a group's stacked key points and descriptors (finetune_heads overrides it)."""
        return self.model.matcher.forward_layers(stacked)

    def _layer_numbers(self, datas, preds, pred, data):
        """The numbers of a group with --layer_report: the matcher's `forward_layers` on the stacked key points and
        descriptors, then `layer_loss`.  `loss/total` keeps its meaning (the final layer's NLL, as without the flag); the
        training-mode total is `loss/total_deep`; the report's [G,L] entries become `layer/<l>/<key>` vectors."""
        from .metrics import KEYS

        stacked = {k: torch.cat([p[k] for p in preds], 0) for k in MATCHER_INPUT_KEYS if k in preds[0]}
        for v in ("view0", "view1"):
            sizes = [d.get(v, {}).get("image_size") for d in datas]
            if all(s is not None for s in sizes):
                stacked[v] = {"image_size": torch.cat([torch.as_tensor(s, dtype=torch.float32).reshape(1, 2)
                                                       for s in sizes], 0).to(self.device)}
        pred.update(self._forward_layers(stacked))
        losses, report = self.model.layer_loss(pred, data)
        numbers = {k: report[k] for k in KEYS}
        numbers.update({"loss/" + k: v for k, v in losses.items() if k not in ("total", "confidence")})
        numbers.update({"loss/total": losses["last"], "loss/confidence": losses["confidence"],
                        "loss/total_deep": losses["total"]})
        for k in LAYER_KEYS + TOKEN_KEYS:
            table = report["layer_" + k]
            numbers.update({f"layer/{i}/{k}": table[:, i] for i in range(table.shape[1])})
        return numbers

    def _group_data(self, datas):
        """The labels' inputs of a group, stacked: `H_0to1` [G,3,3], or cameras, depth maps and `T_0to1` of G pairs."""
        if "H_0to1" in datas[0]:
            return {"H_0to1": torch.cat([d["H_0to1"].to(self.device).reshape(1, 3, 3) for d in datas], 0)}
        from . import geometry

        def holder(cls, items, **kw):
            return cls(torch.cat([it._data.reshape(1, -1) for it in items], 0).to(self.device), **kw)

        data = {"T_0to1": holder(geometry.Pose, [d["T_0to1"] for d in datas])}
        for v in ("view0", "view1"):
            cams = [d[v]["camera"] for d in datas]
            data[v] = {"camera": holder(geometry.Camera, cams, model=cams[0].model)}
            if datas[0][v].get("depth") is not None:
                data[v]["depth"] = torch.cat([d[v]["depth"].to(self.device).reshape((1,) + tuple(d[v]["depth"].shape[-2:]))
                                              for d in datas], 0)
        return data

    @staticmethod
    def _group_key(item, pred):
        key = (pred["keypoints0"].shape[1], pred["keypoints1"].shape[1])
        if "H_0to1" in item:
            return key
        return key + tuple((None if item[v].get("depth") is None else tuple(item[v]["depth"].shape[-2:]),
                            item[v]["camera"].model) for v in ("view0", "view1"))

    def run(self, loader, log_metrics=None, step=0, view_key=None):
        """loader: an iterable of batch-1 pair dicts (`view0/1.image`, `H_0to1`, optionally `name`), e.g. a
        `HomographyPairFeeder`.  view_key(item, i): optional names of shared images for `forward_pairs`.
        -> {metric: mean, "loss/<key>": mean, "num_pairs": n}."""
        results, n_pairs = {}, 0
        self.extra_positives, self._overlaps, self._rows = None, [], []
        log_file = None
        if log_metrics is not None:
            path = Path(log_metrics)
            header = not path.exists() or path.stat().st_size == 0
            mine = TSV_HEADER.rstrip("\n") + "".join("\t" + name for _, name in self._extra) + "\n"
            if not header and self.layer_report:
                with path.open(encoding="ascii") as f:
                    found = f.readline()
                if found != mine:  # (without the flag a file is appended to as it always was)
                    raise ValueError(f"{path} was written with other columns ({len(found.split(chr(9)))}, this run "
                                     f"writes {len(mine.split(chr(9)))}): --layer_report needs a log file of its own")
            log_file = path.open("a", encoding="ascii")
            if header:
                log_file.write(mine)
        try:
            with torch.no_grad():
                chunk = []
                for item in loader:
                    chunk.append(item)
                    if len(chunk) == self.pair_batch:
                        n_pairs += self._run_chunk(chunk, n_pairs, results, log_file, step, view_key)
                        chunk = []
                if chunk:
                    n_pairs += self._run_chunk(chunk, n_pairs, results, log_file, step, view_key)
        finally:
            if log_file is not None:
                log_file.close()
        out = {k: m.compute() for k, m in results.items()}
        out["num_pairs"] = n_pairs
        if self.extra_positives is not None:
            out["gt_extra_positives"] = self.extra_positives
        if self.bins is not None:
            out["bins"] = bin_results(self.bins, self._overlaps, self._rows)
        return out

    def _run_chunk(self, chunk, first, results, log_file, step, view_key):
        keys = None if view_key is None else [(view_key(d, 0), view_key(d, 1)) for d in chunk]
        if self.layer_report:  # the matcher runs per group, with every layer kept
            preds = self.model.extract_pairs(chunk, view_keys=keys)
        else:
            preds = self.model.forward_pairs(chunk, view_keys=keys)
        groups = {}
        for j, p in enumerate(preds):
            groups.setdefault(self._group_key(chunk[j], p), []).append(j)
        rows = [None] * len(chunk)
        for members in groups.values():
            numbers = self._group_loss([chunk[j] for j in members], [preds[j] for j in members])
            for k, values in numbers.items():
                results.setdefault(k, AverageMetric()).update(values)
            for g, j in enumerate(members):
                rows[j] = {k: v[g] for k, v in numbers.items()}
        if self.bins is not None:
            self._overlaps += [_overlap(item) for item in chunk]
            self._rows += rows
        if log_file is not None:
            for j, (item, row) in enumerate(zip(chunk, rows)):
                name = item.get("name", item.get("names", f"{first + j}_0"))
                name = name[0] if isinstance(name, (list, tuple)) else name
                overlap = _overlap(item)
                extra = "".join(f"\t{row[k]:.6f}" for k, _ in self._extra)
                log_file.write(f"{step}\t{first + j}_0\t{name}\t{overlap:.2f}\t{row['match_precision']:.6f}\t"
                               f"{row['match_recall']:.6f}\t{row['accuracy']:.6f}\t{row['average_precision']:.6f}"
                               f"{extra}\n")
        return len(chunk)


def endomapper_model_conf(ground_truth="sparse_depth_matcher", th_positive=None, th_negative=10.0, th_epi=None,
                          matcher_weights="synthetic"):
    """The model of the Endomapper validation: no extractor, LightGlue on 128-d CudaSift descriptors with scales and
    orientations, one of the two sparse-map label components."""
    gt = {**SPARSE_GROUND_TRUTH, "name": "matchers." + ground_truth, "th_positive": th_positive,
          "th_negative": th_negative, "th_epi": th_epi}
    return merge(ENDOMAPPER_MODEL_CONF, {"matcher": {"weights": matcher_weights}, "ground_truth": gt})


def _endomapper_split(data_dir, split):
    """The split file `<split>_seqs_maps.txt` of the tree when it is there, else every sequence that has a map."""
    name = f"{split}_seqs_maps.txt"
    if (data_dir / name).exists():
        return name
    return sorted({f.stem.rsplit("_map", 1)[0] for f in (data_dir / "processed_npz").glob("*_map*.npz")})


def _layer_table(res):
    """The per-layer table of --layer_report from the `layer/<l>/<key>` means (nothing without them)."""
    layers = sorted({int(k.split("/")[1]) for k in res if k.startswith("layer/")})
    if not layers:
        return
    print("layer " + " ".join(["index"] + list(LAYER_KEYS + TOKEN_KEYS)))
    for i in layers:
        cells = [f"{res[f'layer/{i}/{k}']:.6f}" if f"layer/{i}/{k}" in res else "-" for k in LAYER_KEYS + TOKEN_KEYS]
        print(f"layer {i} " + " ".join(cells))


def _print(res):
    for k in sorted(res):
        if not k.startswith("layer/"):
            print(f"{k}: {res[k]:.6f}" if isinstance(res[k], float) else f"{k}: {res[k]}")
    _layer_table(res)
    return res


def _report(res):
    extra = res.get("gt_extra_positives")
    for k in sorted(res):
        if k.startswith("layer/"):
            continue
        if k == "bins":
            for name, bucket in res[k].items():
                print(f"{name}: " + ", ".join(f"{q} {v:.6f}" for q, v in sorted(bucket.items())))
        else:
            print(f"{k}: {res[k]:.6f}" if isinstance(res[k], float) else f"{k}: {res[k]}")
    if extra:
        print(f"loss/* saw {extra} fewer positives than the reference's dense assignment (duplicate ids or a distance "
              "positive beside a seed)")
    _layer_table(res)
    return res


def data_arguments(ap):
    """The options that choose the pairs, the model and the labels (shared with finetune_heads)."""
    ap.add_argument("--data_dir", required=True, help="the image tree (train/ val/ test/ inside)")
    ap.add_argument("--dataset", default="homographies", choices=["homographies", "posed_images", "endomapper"])
    ap.add_argument("--split", default="val")
    ap.add_argument("--pair_batch", type=int, default=32)
    ap.add_argument("--extractor_weights", default="synthetic", help="local .pth (reference key names) or 'synthetic'")
    ap.add_argument("--matcher_weights", default="synthetic")
    ap.add_argument("--max_num_keypoints", type=int, default=512)
    ap.add_argument("--num_workers", type=int, default=2)
    ap.add_argument("--th_epi", type=float, default=None, help="posed_images: th_epi of the depth matcher (MegaDepth: 5)")
    ap.add_argument("--benchmark", default="megadepth1500", help="posed_images: the directory layout, a posed_images "
                                                                 "preset of eval_pose_pairs.BENCHMARK_DATA")
    ap.add_argument("--ground_truth", default="sparse_depth_matcher",
                    choices=["sparse_depth_matcher", "sparse_dense_depth_matcher"], help="endomapper: the label component")
    ap.add_argument("--th_positive", type=float, default=None, help="endomapper: th_positive (default null)")
    ap.add_argument("--th_negative", type=float, default=10.0, help="endomapper: th_negative")
    ap.add_argument("--max_num_features", type=int, default=2048, help="endomapper: key points per view")


def setup(args):
    """-> (model_conf of the ValidationPipeline, loader() = a fresh feeder over the split, view_key or None, the
    function that prints a result) for the parsed `data_arguments`."""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16)))
    from .registry import get_dataset

    model_conf = {"extractor": {"weights": args.extractor_weights, "max_num_keypoints": args.max_num_keypoints},
                  "matcher": {"weights": args.matcher_weights}}
    if args.dataset == "endomapper":
        data_dir = Path(args.data_dir).resolve()
        dataset = get_dataset("endomapper")({"data_dir": data_dir.name, "max_num_features": args.max_num_features,
                                             "reseed": True, args.split + "_split": _endomapper_split(data_dir, args.split)},
                                            data_dir.parent, split=args.split)
        conf = endomapper_model_conf(args.ground_truth, args.th_positive, args.th_negative, args.th_epi,
                                     args.matcher_weights)
        return (conf, lambda: dataset.feeder("cuda", num_workers=args.num_workers, batch=args.pair_batch),
                dataset.view_key, _report)
    if args.dataset == "posed_images":
        from .eval_pose_pairs import BENCHMARK_DATA

        conf = dict(BENCHMARK_DATA[args.benchmark])
        if conf.pop("name") != "posed_images":
            raise NotImplementedError(f"{args.benchmark}: not a posed_images directory")
        dataset = get_dataset("posed_images")(conf, args.data_dir)
        return ({**model_conf, "ground_truth": {**DEPTH_GROUND_TRUTH, "th_epi": args.th_epi}},
                lambda: dataset.feeder("cuda", num_workers=args.num_workers), None, _print)
    data_dir = Path(args.data_dir).resolve()
    dataset = get_dataset("homographies")({"data_dir": data_dir.name, "photometric": {"name": "identity"},
                                           "reseed": True}, data_dir.parent, split=args.split)
    return (model_conf, lambda: dataset.feeder(batch=args.pair_batch, num_workers=args.num_workers), dataset.view_key,
            _print)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    data_arguments(ap)
    ap.add_argument("--log_metrics", default=None, help="append the per-pair TSV to this file")
    ap.add_argument("--eval_overlap_bins", default=None, help='overlap bins "low:high,low:high" (reported under bins)')
    ap.add_argument("--layer_report", action="store_true",
                    help="score every LightGlue layer (forward_layers + layer_loss): loss/confidence, loss/total_deep, "
                         "a per-layer table and the same columns in the TSV")
    args = ap.parse_args(argv)
    model_conf, loader, view_key, report = setup(args)
    # (the overlap bins belong to the Endomapper pairs, the only ones that carry an overlap)
    pipe = ValidationPipeline(model_conf, pair_batch=args.pair_batch, layer_report=args.layer_report,
                              eval_overlap_bins=args.eval_overlap_bins if args.dataset == "endomapper" else None)
    return report(pipe.run(loader(), log_metrics=args.log_metrics, view_key=view_key))


if __name__ == "__main__":
    main(sys.argv[1:])
