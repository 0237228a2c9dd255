"""Re-fit LightGlue's assignment heads and exit tokens on one's own pairs, the trunk frozen: the part of the reference's
training step (gluefactory/train.py:1106-1160) that needs no transformer backward.  The gradients are those of the
reference's training loss (`LightGlue.layer_loss_backward`); the trunk, `input_proj` and the positional encoding are
never touched.

    python -m glue_factory_colon_amd.finetune_heads --data_dir D --dataset {homographies,posed_images,endomapper}
        [--params {tokens,heads,all,output_stage,all+output_stage,cross_block,all+cross_block,last_layer,all+last_layer}] [--lr 1e-3] [--optimizer {adam,sgd}] [--clip_grad G] [--epochs E]
        [--max_steps S] [--pair_batch N] --out FILE

The pairs come from `validate`'s feeders, with its ground-truth options and its grouping: inside a `--pair_batch` chunk
the pairs of equal (M, N) form one group, which goes through `forward_layers`, `layer_loss` and `layer_loss_backward`
with grad_total = 1 / (pairs in the chunk); ONE optimizer step is taken per chunk, then `heads_updated()`.  `--params
tokens` / `heads` hand only those parameters to the optimizer; the others are not passed to it.  `--params output_stage`
re-fits `to_out` and `ffn` of the last layer's cross block (eight tensors, about 460 k parameters, whose exact gradients
`layer_loss_backward(output_stage=True)` gives), `all+output_stage` those with the heads and tokens; the rest of the trunk
stays frozen, and every step also ends with `output_stage_updated()`.  `--params cross_block` re-fits the twelve tensors
of the last cross block (the output stage and `to_qk`, `to_v`, through `layer_loss_backward(output_stage=True,
cross_attention=True)`), `all+cross_block` those with the heads and tokens; every such step also ends with
`cross_attention_updated()`.  `--params last_layer` re-fits all 22 tensors of the last layer (the cross block and the
self block in front of it, through `layer_loss_backward(..., self_block=True)`), `all+last_layer` those with the heads and
tokens; every such step also ends with `self_block_updated()`.  `loss/total_deep`,
`loss/confidence` and the per-layer table of `validate --layer_report` are printed before and after, and the matcher's
`state_dict()` is written to `--out`, which `conf.weights = FILE` loads.  No schedules, no checkpoint resume, no mixed
precision.
"""
import argparse
import itertools
import sys

import torch

from . import validate

PREFIXES = {"tokens": ("token_confidence.",), "heads": ("log_assignment.",),
            "all": ("token_confidence.", "log_assignment.")}
# choices that also train the last layer's output stage -> the prefixes of the heads and tokens trained with it
OUTPUT_STAGE = {"output_stage": (), "all+output_stage": PREFIXES["all"], "cross_block": (),
                "all+cross_block": PREFIXES["all"], "last_layer": (), "all+last_layer": PREFIXES["all"]}
CROSS_BLOCK = ("cross_block", "all+cross_block", "last_layer", "all+last_layer")  # ... and to_qk, to_v in front of its attention
LAST_LAYER = ("last_layer", "all+last_layer")  # ... and the self block in front of the cross block


class HeadTuner(validate.ValidationPipeline):
    """The validation pass with every layer scored; while `tuning` is set, every group also accumulates the head and
    token gradients and every chunk ends with one optimizer step."""

    def __init__(self, model_conf=None, pair_batch=32, device="cuda", params="all", lr=1e-3, optimizer="adam",
                 clip_grad=None):
        super().__init__(model_conf, pair_batch=pair_batch, device=device, layer_report=True)
        matcher = self.model.matcher
        self.output_stage = params in OUTPUT_STAGE
        self.cross_attention = params in CROSS_BLOCK
        self.self_block = params in LAST_LAYER
        prefixes = OUTPUT_STAGE[params] if self.output_stage else PREFIXES[params]
        touched = PREFIXES["all"]
        if self.output_stage:
            stage = f"transformers.{int(matcher.conf.n_layers) - 1}.cross_attn."
            prefixes += (stage + "to_out.", stage + "ffn.")
            touched += (stage + "to_out.", stage + "ffn.")
            if self.cross_attention:
                prefixes += (stage + "to_qk.", stage + "to_v.")
                touched += (stage + "to_qk.", stage + "to_v.")
            if self.self_block:
                block = f"transformers.{int(matcher.conf.n_layers) - 1}.self_attn."
                prefixes += (block,)
                touched += (block,)
        self.trained = {n: p for n, p in matcher.named_parameters() if n.startswith(prefixes)}
        self.touched = [p for n, p in matcher.named_parameters() if n.startswith(touched)]
        cls = {"adam": torch.optim.Adam, "sgd": torch.optim.SGD}[optimizer]
        self.optimizer = cls(list(self.trained.values()), lr=lr)
        self.clip_grad = clip_grad
        self.tuning = False  # set by `tune`: `run` then takes steps
        self.steps = 0
        self._chunk_pairs = 1

    def _forward_layers(self, stacked):
        # the rows and context the output stage's backward starts from are kept only while a step needs them
        return self.model.matcher.forward_layers(stacked, keep_output_stage=self.tuning and self.output_stage,
                                                 keep_self_block=self.tuning and self.self_block)

    def _layer_numbers(self, datas, preds, pred, data):
        numbers = super()._layer_numbers(datas, preds, pred, data)
        if self.tuning:
            g = torch.full((len(datas),), 1.0 / self._chunk_pairs, device=self.device)
            self.model.layer_loss_backward(pred, data, grad_total=g, output_stage=self.output_stage,
                                           cross_attention=self.cross_attention, self_block=self.self_block)
        return numbers

    def _run_chunk(self, chunk, first, results, log_file, step, view_key):
        if not self.tuning:
            return super()._run_chunk(chunk, first, results, log_file, step, view_key)
        self._chunk_pairs = len(chunk)
        for p in self.touched:
            p.grad = None
        n = super()._run_chunk(chunk, first, results, log_file, step, view_key)
        if self.clip_grad is not None:
            torch.nn.utils.clip_grad_norm_(list(self.trained.values()), self.clip_grad)
        self.optimizer.step()
        self.model.matcher.heads_updated()
        if self.output_stage:
            self.model.matcher.output_stage_updated()
        if self.cross_attention:
            self.model.matcher.cross_attention_updated()
        if self.self_block:
            self.model.matcher.self_block_updated()
        self.steps += 1
        return n

    def tune(self, loader, max_steps=None, view_key=None):
        """One pass over `loader` with an optimizer step per chunk (at most `max_steps` more steps)."""
        if max_steps is not None:
            loader = itertools.islice(loader, max(0, max_steps - self.steps) * self.pair_batch)
        self.tuning = True
        try:
            return self.run(loader, view_key=view_key)
        finally:
            self.tuning = False


def _summary(tag, res):
    print(f"{tag}: loss/total_deep {res.get('loss/total_deep', float('nan')):.6f} loss/confidence "
          f"{res.get('loss/confidence', float('nan')):.6f} pairs {res['num_pairs']}")
    validate._layer_table(res)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    validate.data_arguments(ap)
    ap.add_argument("--params", default="all", choices=sorted(PREFIXES) + sorted(OUTPUT_STAGE))
    ap.add_argument("--lr", type=float, default=1e-3, help="the reference's default learning rate")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "sgd"])
    ap.add_argument("--clip_grad", type=float, default=None, help="clip the gradient norm of the trained parameters")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--max_steps", type=int, default=None, help="stop after this many optimizer steps")
    ap.add_argument("--out", required=True, help="the matcher's state_dict() is written here")
    args = ap.parse_args(argv)
    model_conf, loader, view_key, _ = validate.setup(args)
    tuner = HeadTuner(model_conf, pair_batch=args.pair_batch, params=args.params, lr=args.lr, optimizer=args.optimizer,
                      clip_grad=args.clip_grad)
    before = tuner.run(loader(), view_key=view_key)
    _summary("before", before)
    for _ in range(args.epochs):
        if args.max_steps is not None and tuner.steps >= args.max_steps:
            break
        tuner.tune(loader(), max_steps=args.max_steps, view_key=view_key)
    after = tuner.run(loader(), view_key=view_key)
    _summary(f"after {tuner.steps} steps", after)
    torch.save({k: v.detach().cpu() for k, v in tuner.model.matcher.state_dict().items()}, args.out)
    print(f"wrote {args.out}")
    return before, after


if __name__ == "__main__":
    main(sys.argv[1:])
