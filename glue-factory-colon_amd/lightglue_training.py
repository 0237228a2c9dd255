"""The training side of the LightGlue matcher: the validation loss, the kept-layers forward, the deep-supervision loss
and the gradients of the heads, the exit tokens and the last layer -- its cross block (output stage and attention) and
its self block (FFN part, rotary attention and Wqkv)
(reference file gluefactory/models/matchers/lightglue.py:151-164,193-222,495-498,546-547,588-637).  `LightGlueTraining` is a mix-in of
`lightglue.LightGlue`: it reads the module's configuration, parameters, packed weights and workspace and adds no state
of its own, so every method is called on the matcher as before.
"""
import ctypes

import torch

from . import _native as nat
from ._rows import match_outputs, pack_sides, put_sides, split_sides, stacked_sides
from .base_model import conf_get
from .losses import OUT_KEYS, as_dict, validation_metrics
from .metrics import KEYS

_FINAL_LOSSES = ("assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable")


def _refuse_adaptive(conf, name):
    """Entry point `name` works on the full-depth pass only."""
    if conf.depth_confidence > 0 or conf.width_confidence > 0:
        raise NotImplementedError(
            f"{name}: depth_confidence / width_confidence > 0 (early stopping, pruning) are disabled in the reference's "
            "training mode (lightglue.py:471-472) and refused here; on an early-stopped / pruned prediction the "
            "reference applies the LAST head to the stop layer's descriptors, which such a prediction does not hold")


def _refuse_other_loss(conf, name):
    if conf_get(conf.loss, "fn", "nll") != "nll":
        raise NotImplementedError(f"{name}: loss.fn {conf.loss.fn!r}: only 'nll' is built")


def _layer_weights(conf):
    """The weights w_l of the layers l < L - 1 in the training loss (lightglue.py:611-614): gamma^(L-l-1) for
    loss.gamma > 0, else l + 1.  The last layer has weight 1 (lightglue.py:597-598)."""
    gamma, nl = float(conf_get(conf.loss, "gamma", 1.0)), conf.n_layers
    return [gamma ** (nl - i - 1) if gamma > 0.0 else float(i + 1) for i in range(nl - 1)]


class _LayerPass:
    """What `layer_loss` and `layer_loss_backward` share: the checks of a `forward_layers` prediction (the constructor:
    host only, before any GPU work), then (`open`) the labels as the kernels read them, ONE set of per-layer buffers,
    one workspace, and the launches both loops make on a layer's rows.  One layer is alive at a time."""

    def __init__(self, lg, name, pred):
        conf = lg.conf
        nl = conf.n_layers
        ref0, ref1 = pred["ref_descriptors0"], pred["ref_descriptors1"]
        if ref0.dim() != 4 or ref0.shape[1] != nl or ref1.shape[1] != nl:
            raise ValueError(f"{name} needs the descriptors of all {nl} layers, ref_descriptors0 is "
                             f"{tuple(ref0.shape)}: the prediction must come from forward_layers, not forward")
        b, _, m, d = ref0.shape
        n = ref1.shape[2]
        if m == 0 or n == 0:
            raise ValueError(f"{name} of a pair without key points in one view ({m} x {n})")
        _refuse_adaptive(conf, name)
        _refuse_other_loss(conf, name)
        self.lg, self.pred, self.ref0, self.ref1 = lg, pred, ref0, ref1
        self.nl, self.b, self.m, self.n, self.d = nl, b, m, n, d
        self.bm, self.rows = b * m, b * (m + n)
        self.device = ref0.device
        self.balancing = float(conf_get(conf.loss, "nll_balancing", 0.5))
        self.weights = _layer_weights(conf)

    def open(self, data, *entry_points, by_rows=()):
        """The device side.  The workspace is sized for gfc_lg_assign, gfc_lg_layer_scores and the caller's other
        `entry_points`, each by the `_workspace_bytes(B, M, N)` of its name (`by_rows`: by `_workspace_bytes(rows)`)."""
        b, m, n, device = self.b, self.m, self.n, self.device
        nat.require_cuda(self.ref0, "pred['ref_descriptors0']")
        self.params = self.lg.ensure_packed(device)[0]
        self.la_final = la_final = self.pred["log_assignment"].float().contiguous()
        self.gt0 = gt0 = data["gt_matches0"].to(device=device, dtype=torch.long).contiguous()
        self.gt1 = gt1 = data["gt_matches1"].to(device=device, dtype=torch.long).contiguous()
        gta = data.get("gt_assignment")
        if tuple(la_final.shape) != (b, m + 1, n + 1) or tuple(gt0.shape) != (b, m) or tuple(gt1.shape) != (b, n) or (
                gta is not None and tuple(gta.shape) != (b, m, n)):
            raise ValueError(f"ref_descriptors {tuple(self.ref0.shape)} / {tuple(self.ref1.shape)} do not fit "
                             f"log_assignment {tuple(la_final.shape)}, gt_matches0 {tuple(gt0.shape)}, gt_matches1 "
                             f"{tuple(gt1.shape)}")
        self.gta = None if gta is None else gta.to(device=device).ne(0).contiguous()
        names = ("gfc_lg_assign", "gfc_lg_layer_scores") + entry_points
        need = [nat.call(f"{name}_workspace_bytes", b, m, n) for name in names]
        need += [nat.call(f"{name}_workspace_bytes", self.rows) for name in by_rows]
        self.ws = self.lg._ws.get(max(need), device)
        # ONE buffer for every layer's own assignment, matches and token logits
        self.pm0, self.pm1, self.ps0, self.ps1, self.la = match_outputs(b, m, n, device)
        self.logits = torch.empty((self.rows,), device=device)

    def layer_rows(self, i):
        """[B*M + B*N, 256], side 0 first: slot i of the stack of forward_layers as it is, else one concatenation."""
        return pack_sides(self.ref0[:, i].float().contiguous(), self.ref1[:, i].float().contiguous())

    def assign(self, i, x):
        """Layer i's own assignment (its head on its rows x) into `la`, its mutual matches into `pm0/1`, `ps0/1`."""
        nat.call("gfc_lg_assign", ctypes.byref(self.params), i, x, x[self.bm:], self.b, self.m, self.n,
                 float(self.lg.conf.filter_threshold), self.pm0, self.pm1, self.ps0, self.ps1, self.la, self.ws,
                 self.ws.numel())

    def token_logits(self, i, x):
        """Layer i's exit-token logits (gfc_lg_rowdot without the sigmoid) into `logits`."""
        nat.call("gfc_lg_rowdot", x, self.d, self.rows, self.params.token_w[i], self.params.token_b[i], 0, self.logits)

    def layer_scores(self, threshold, out, correct=None):
        """gfc_lg_layer_scores of `la` against the final assignment and of `logits` against `threshold` into out [B,6];
        with `correct` [B*M + B*N] uint8 also the tokens' targets."""
        c0, c1 = (None, None) if correct is None else (correct, correct[self.bm:])
        nat.call("gfc_lg_layer_scores", self.la, self.la_final, self.logits, self.logits[self.bm:], float(threshold),
                 self.b, self.m, self.n, out, c0, c1, self.ws, self.ws.numel())


class LightGlueTraining:
    def loss(self, pred, data):
        """The reference's `loss` (lightglue.py:588-637) in eval mode: (losses, metrics) of a full-depth prediction and
        the labels `gt_matches0/1` (and `gt_assignment`, when the ground truth made one) in `data`.  In eval mode the
        reference keeps the last layer only, so its layer loop runs zero times and total = last = the NLL of the final
        assignment; it recomputes that assignment from ref_descriptors[:, -1] with the last head, which is
        pred["log_assignment"] here.  One launch (gfc_lg_validation_metrics) gives the loss terms, row_norm and the
        four matcher metrics; every value is a [B] tensor."""
        if self.training:
            raise NotImplementedError("the training loss (per-layer terms, token confidence, backward) is out of scope")
        conf = self.conf
        _refuse_adaptive(conf, "loss")
        _refuse_other_loss(conf, "loss")
        out = validation_metrics(pred["log_assignment"], data["gt_matches0"], data["gt_matches1"],
                                 data.get("gt_assignment"), pred["matches0"], pred["matching_scores0"],
                                 conf_get(conf.loss, "nll_balancing", 0.5))
        d = as_dict(out, OUT_KEYS)
        losses = {"total": d["assignment_nll"], "last": d["assignment_nll"].clone(),
                  **{k: d[k] for k in _FINAL_LOSSES}, "row_norm": d["row_norm"]}
        return losses, {k: d[k] for k in KEYS}

    # -- every layer kept: the training-mode forward and loss of the reference, forward only ---------------
    def forward_layers(self, data: dict, keep_output_stage: bool = False, keep_self_block: bool = False) -> dict:
        """The reference's forward under `model.train()` (lightglue.py:495-498,546-547): full depth, every layer's
        descriptors kept -- `ref_descriptors0` [B,L,M,256], `ref_descriptors1` [B,L,N,256], index l the output of
        transformer l; every other key as `forward` returns it.  LightGlue has no dropout and no batch norm, so this is
        the eval forward with the layers kept; it does not look at `self.training`.  Early stopping and pruning are
        refused, as the reference disables both in training mode (lightglue.py:471-472).
        The host drives the layers one by one (`gfc_lg_layer_pairs`: `gfc_lg_layer` with the cross attention
        gfc_lg_forward_packed takes for the batch) and ends with `gfc_lg_assign` on the last head: the launch
        sequence of gfc_lg_forward_packed.  Layer l works in place on slot l of one stack buffer [L, B*M + B*N, 256],
        which it enters by one device-to-device copy of slot l - 1; the returned descriptors are permuted views of it.
        With `keep_output_stage` the last layer runs through gfc_lg_layer_pairs_keep (the same launches and two copies)
        and the prediction also holds what the backward of that layer's output stage starts from
        (`layer_loss_backward(output_stage=True)`): `output_stage_rows0` [B,M,256] / `output_stage_rows1` [B,N,256], the
        rows the last cross block reads, and `output_stage_context0/1`, its attention context before `to_out`: views of
        two [B*M + B*N, 256] buffers.  Every other key is the default call's, bit for bit.
        With `keep_self_block` (needs `keep_output_stage`) the last layer runs through gfc_lg_layer_pairs_keep_self (one
        more copy) and the prediction also holds what `layer_loss_backward(self_block=True)` starts from:
        `self_block_context0/1`, the last SELF attention's context before `out_proj`, views of a third buffer, and the
        rotary tables of the packed rows, `self_block_cos` / `self_block_sin` [B*M + B*N, 64] -- they are kept, not
        recomputed, because the backward sees the labels and not the key points.  The rows the last self block reads
        are `ref_descriptors0/1[:, L-2]`."""
        if keep_self_block and not keep_output_stage:
            raise ValueError("keep_self_block needs keep_output_stage=True: the self block's backward starts from the "
                             "cross block's")
        self._check_ready(data)
        conf = self.conf
        _refuse_adaptive(conf, "forward_layers")
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        nat.require_cuda(kpts0, "data['keypoints0']")
        b, m, _ = kpts0.shape
        n = kpts1.shape[1]
        device = kpts0.device
        kp, de, so, s0, s1 = self._uniform_rows(data)
        d, nl = conf.descriptor_dim, conf.n_layers
        if keep_output_stage and conf.matmul_precision != "fp32":
            raise NotImplementedError("matmul_precision 'fp16': the output stage is kept for the fp32 matcher")
        if m == 0 or n == 0:  # the early return of `forward`
            pred = self._empty_result(torch.zeros((b, nl, m, d), device=device), torch.zeros((b, nl, n, d), device=device))
            if keep_output_stage:
                for key in ("output_stage_rows", "output_stage_context"):
                    put_sides(pred, key, (torch.zeros((b, m, d), device=device), torch.zeros((b, n, d), device=device)))
            if keep_self_block:
                put_sides(pred, "self_block_context", (torch.zeros((b, m, d), device=device),
                                                       torch.zeros((b, n, d), device=device)))
                pred["self_block_cos"] = torch.zeros((b * (m + n), 64), device=device)
                pred["self_block_sin"] = torch.zeros((b * (m + n), 64), device=device)
            return pred
        params = self._packed[0]
        rows = b * (m + n)
        stack = torch.empty((nl, rows, d), device=device)
        if conf.input_dim != d:
            self._input_proj(params, de, stack[0], rows)
        else:
            stack[0].copy_(de)
        # problem b = side 0 of pair b, b + B = side 1 (the tables of gfc_lg_forward_packed), one upload
        r0 = torch.arange(b, dtype=torch.int32) * m
        r1 = b * m + torch.arange(b, dtype=torch.int32) * n
        cm, cn = torch.full_like(r0, m), torch.full_like(r1, n)
        self_p = torch.cat([torch.stack([r0, cm, r0, cm], 1), torch.stack([r1, cn, r1, cn], 1)], 0)
        cross_p = torch.cat([torch.stack([r0, cm, r1, cn], 1), torch.stack([r1, cn, r0, cm], 1)], 0)
        tabs = torch.cat([self_p.reshape(-1), cross_p.reshape(-1), r0, r1, cm, cn]).to(device)
        self_p, cross_p = tabs[:8 * b].view(2 * b, 4), tabs[8 * b:16 * b].view(2 * b, 4)
        row0, cnt = tabs[16 * b:18 * b], tabs[18 * b:20 * b]
        sizes = torch.cat([s0, s1], 0).contiguous()
        cos, sin = torch.empty((rows, 64), device=device), torch.empty((rows, 64), device=device)
        nat.call("gfc_lg_posenc", kp, so, sizes, row0, cnt, 2 * b, max(m, n), params.posenc_wr,
                 4 if so is not None else 2, cos, sin)
        # gfc_lg_layer_pairs: gfc_lg_layer with the cross attention `forward` takes for this batch (from 8 large pairs
        # on it evaluates sim once), so that the last layer is `forward`'s at every batch size
        ws = self._ws.get(max(nat.call("gfc_lg_layer_pairs_workspace_bytes", b, m, n),
                              nat.call("gfc_lg_assign_workspace_bytes", b, m, n)), device)
        kept = torch.empty((3 if keep_self_block else 2, rows, d), device=device) if keep_output_stage else None
        for i in range(nl):
            if i > 0:
                stack[i].copy_(stack[i - 1])
            if kept is not None and i == nl - 1:
                if keep_self_block:
                    nat.call("gfc_lg_layer_pairs_keep_self", ctypes.byref(params), i, stack[i], cos, sin, b, m, n, self_p,
                             cross_p, kept[0], kept[1], kept[2], ws, ws.numel())
                else:
                    nat.call("gfc_lg_layer_pairs_keep", ctypes.byref(params), i, stack[i], cos, sin, b, m, n, self_p,
                             cross_p, kept[0], kept[1], ws, ws.numel())
                continue
            nat.call("gfc_lg_layer_pairs", ctypes.byref(params), i, stack[i], cos, sin, b, m, n, self_p, cross_p, ws,
                     ws.numel())
        m0, m1, ms0, ms1, scores = match_outputs(b, m, n, device)
        last = stack[nl - 1]
        nat.call("gfc_lg_assign", ctypes.byref(params), nl - 1, last, last[b * m:], b, m, n,
                 float(conf.filter_threshold), m0, m1, ms0, ms1, scores, ws, ws.numel())
        pred = self._result(m0, m1, ms0, ms1, *stacked_sides(stack, b, m, n), scores)
        if kept is not None:
            put_sides(pred, "output_stage_rows", split_sides(kept[0], b, m, n))
            put_sides(pred, "output_stage_context", split_sides(kept[1], b, m, n))
        if keep_self_block:
            put_sides(pred, "self_block_context", split_sides(kept[2], b, m, n))
            pred["self_block_cos"], pred["self_block_sin"] = cos, sin
        return pred

    def layer_loss(self, pred, data):
        """The reference's `loss` under `model.train()` (lightglue.py:597-630), forward only, plus a per-layer exit
        report: (losses, report) of a `forward_layers` prediction and the labels `gt_matches0/1` (and `gt_assignment`,
        when the ground truth made one) in `data`.  It does not look at `self.training`.

        Every layer l < L - 1 goes through its own head (gfc_lg_assign into ONE re-used log-assignment buffer, so only
        the final assignment and one layer's are alive), gfc_lg_validation_metrics on that assignment with that
        layer's own mutual matches, the token logits (gfc_lg_rowdot without the sigmoid) and gfc_lg_layer_scores.  The
        reference re-uses the weight matrix of the last layer for every layer (`weights=gt_weights`,
        lightglue.py:598,609); that matrix depends on the labels only, so gfc_lg_validation_metrics on each layer with
        the same labels is the same arithmetic.

        losses, each [B]: `last`, `assignment_nll`, `nll_pos`, `nll_neg`, `num_matchable`, `num_unmatchable`,
        `row_norm` of the final layer (what `loss` returns), `confidence` = sum_l (bce0_l + bce1_l) / 2 / (L - 1) and
        `total` = (nll_{L-1} + sum_l w_l nll_l) / (1 + sum_l w_l) + confidence with w_l = gamma^(L-l-1) for
        loss.gamma > 0, else l + 1, added in the reference's order.
        report (MI355X addition), [B,L]: `layer_nll`, `layer_nll_pos`, `layer_nll_neg`, `layer_recall`,
        `layer_precision` (the matcher metrics of layer l's own mutual matches); [B,L-1]: `layer_agree` = the share of
        points whose arg-max (dustbin included) is that of the final layer -- the token-confidence target --,
        `layer_token_bce`, `layer_ratio_confident` = the share of points with !(token < confidence_threshold(l)), the
        number check_if_stop (lightglue.py:569-580) compares with depth_confidence; [B]: the four matcher metrics of the
        final layer under the names `loss` gives them."""
        lp = _LayerPass(self, "layer_loss", pred)
        lp.open(data)
        nl, b, m, n, device = lp.nl, lp.b, lp.m, lp.n, lp.device
        thresholds = self._host_thresholds()  # no device-to-host read after the first call
        vm = torch.empty((nl, b, len(OUT_KEYS)), device=device)       # gfc_lg_validation_metrics of every layer
        sc = torch.empty((max(nl - 1, 0), b, 6), device=device)        # gfc_lg_layer_scores of every layer but the last
        nat.call("gfc_lg_validation_metrics", lp.la_final, lp.gt0, lp.gt1, lp.gta,
                 pred["matches0"].to(device=device, dtype=torch.long).contiguous(),
                 pred["matching_scores0"].to(device=device, dtype=torch.float32).contiguous(), b, m, n, lp.balancing,
                 vm[nl - 1])
        for i in range(nl - 1):
            x = lp.layer_rows(i)
            lp.assign(i, x)
            nat.call("gfc_lg_validation_metrics", lp.la, lp.gt0, lp.gt1, lp.gta, lp.pm0, lp.ps0, b, m, n, lp.balancing,
                     vm[i])
            lp.token_logits(i, x)
            lp.layer_scores(thresholds[i], sc[i])
        col = OUT_KEYS.index
        nll = vm[:, :, col("assignment_nll")]  # [L,B]
        # lightglue.py:597-630 in its order of additions
        total, sum_weights = nll[nl - 1], 1.0
        confidence = torch.zeros((b,), device=device)
        for i, weight in enumerate(lp.weights):
            sum_weights += weight
            total = total + nll[i] * weight
            confidence = confidence + (sc[i, :, 2] + sc[i, :, 3]) / 2.0 / (nl - 1)
        total = total / sum_weights + confidence
        final = vm[nl - 1]
        losses = {"total": total, "last": final[:, col("assignment_nll")].clone(),
                  **{k: final[:, col(k)] for k in _FINAL_LOSSES},
                  "row_norm": final[:, col("row_norm")], "confidence": confidence}
        report = {"layer_nll": nll.t(), "layer_nll_pos": vm[:, :, col("nll_pos")].t(),
                  "layer_nll_neg": vm[:, :, col("nll_neg")].t(), "layer_recall": vm[:, :, col("match_recall")].t(),
                  "layer_precision": vm[:, :, col("match_precision")].t(),
                  "layer_agree": ((sc[:, :, 0] + sc[:, :, 1]) / (m + n)).t(),
                  "layer_token_bce": ((sc[:, :, 2] + sc[:, :, 3]) / 2.0).t(),
                  "layer_ratio_confident": ((sc[:, :, 4] + sc[:, :, 5]) / (m + n)).t(),
                  **{k: final[:, col(k)] for k in KEYS}}
        return losses, report

    # -- gradients of the training loss with respect to the heads and exit tokens (the trunk frozen) --------
    def layer_loss_backward(self, pred, data, grad_total=None, descriptor_grads=False, accumulate=True,
                            output_stage=False, cross_attention=False, self_block=False):
        """The gradients of `layer_loss`'s `total` with respect to the assignment heads and the exit tokens, what
        `torch.mean(losses["total"]).backward()` (gluefactory/train.py:1114) leaves in their `.grad` in the reference:
        the parameters of log_assignment[l] enter the loss through head l only (lightglue.py:589-616) and the token
        reads detached descriptors (lightglue.py:83-85).  The trunk is not followed; `row_norm` and `last` carry no
        gradient.

        pred: a `forward_layers` prediction; data: the labels, as `layer_loss` takes them; grad_total [B]: the weight of
        each pair's `total` in the differentiated scalar (default 1 / B each: the mean).  Returns a dict keyed by the
        reference's state-dict names: `log_assignment.{l}.final_proj.weight` [256,256] / `.bias` [256],
        `log_assignment.{l}.matchability.weight` [1,256] / `.bias` [1], `token_confidence.{l}.token.0.weight` [1,256] /
        `.bias` [1].  With `accumulate` the same tensors are added into `.grad` of the module's parameters (created when
        absent, as Tensor.backward does), so a torch optimizer works unchanged.  With `descriptor_grads` the dict also
        holds `grad_ref_descriptors0` [B,L,M,256] and `grad_ref_descriptors1` [B,L,N,256], permuted views of one
        [L, B*M + B*N, 256] buffer (the layout of forward_layers' stack): the DIRECT gradient at every layer's
        descriptors, where a trunk backward would start.  Without the flag that buffer is never allocated.

        One layer is alive at a time, with one re-used workspace: gfc_lg_head_backward on the layer's rows; for l < L - 1
        the layer's own assignment (gfc_lg_assign), its token logits, the targets correct0/1 from gfc_lg_layer_scores
        and gfc_lg_token_backward.  Nothing is read back to the host.  Gradients are built for the fp32 matcher.

        With `output_stage` (a prediction of `forward_layers(keep_output_stage=True)`, n_layers >= 2) the dict, and
        `.grad` under `accumulate`, also hold the gradients of the last layer's output stage,
        `transformers.{L-1}.cross_attn.to_out.weight/.bias` and `.ffn.0/.1/.3.weight/.bias`: these eight tensors reach
        the loss through head L - 1 only (lightglue.py:219-221,589-616; there is no exit token after the last layer), so
        head L - 1's direct descriptor gradient, taken for that layer alone, sent through that one FFN block
        (gfc_lg_ffn_backward on the state-dict weights, not the folded ones) is exactly what the reference's backward
        leaves in them.  `grad_output_stage_rows0/1` and `grad_output_stage_context0/1` are the kernel's two row outputs:
        the gradient at the rows the last cross block reads, through the residual and the first half of the
        concatenation only, and at its attention context -- the operands an attention backward starts from.

        With `cross_attention` (needs `output_stage`) those two go through the backward of that block's bidirectional
        attention (gfc_lg_cross_attn_backward on the state-dict `to_qk` / `to_v`): the dict, and `.grad` under
        `accumulate`, also hold `transformers.{L-1}.cross_attn.to_qk.weight/.bias` and `.to_v.weight/.bias` -- exact for
        the same reason: the last cross block reaches the loss through head L - 1 alone (lightglue.py:193-222) -- and
        the dict `grad_cross_block_rows0` [B,M,256] / `grad_cross_block_rows1` [B,N,256], the COMPLETE gradient at the
        rows the last cross block reads (`grad_output_stage_rows` plus the attention's share), where the backward of
        the last self block starts.  Without the keyword every result is what it was, bit for bit.

        With `self_block` (needs `cross_attention` and a prediction of `forward_layers(keep_self_block=True)`) that
        gradient goes through the last SELF block (lightglue.py:151-164): gfc_lg_ffn_backward on the state-dict
        `out_proj`, `ffn.0/.1/.3` of `transformers.{L-1}.self_attn` with the rows of layer L - 2 and the kept self
        context, then gfc_lg_self_attn_backward (rotary attention and `Wqkv`, on the packed row order; the gradients are
        mapped back to the state dict's by the inverse of `_pack`'s index, which is exact).  The dict, and `.grad` under
        `accumulate`, also hold the ten tensors of `transformers.{L-1}.self_attn.` -- exact for the same reason: the
        last self block reaches the loss through the last cross block and head L - 1 alone -- so all 22 tensors of
        layer L - 1 have their gradients.  The dict also holds `grad_self_block_rows0/1`, the gradient at layer L - 1's
        input rows through layer L - 1 alone, and `grad_layer_input_rows0/1`, the same plus head L - 2's direct
        descriptor gradient: the COMPLETE gradient at `ref_descriptors0/1[:, L-2]`, where the backward of layer L - 2
        would start.  No gradient for `posenc.Wr` is produced: the rotary tables get gradient from every layer.
        Without the keyword every result is what it was, bit for bit."""
        lp = _LayerPass(self, "layer_loss_backward", pred)
        nl, b, m, n, d, rows, device = lp.nl, lp.b, lp.m, lp.n, lp.d, lp.rows, lp.device
        if self.conf.matmul_precision != "fp32":
            raise NotImplementedError("matmul_precision 'fp16': gradients are built for the fp32 matcher")
        if output_stage:
            if nl < 2:
                raise ValueError("output_stage needs n_layers >= 2")
            missing = [k for k in ("output_stage_rows0", "output_stage_rows1", "output_stage_context0",
                                   "output_stage_context1") if k not in pred]
            if missing:
                raise ValueError(f"output_stage needs {missing} in the prediction: call "
                                 "forward_layers(data, keep_output_stage=True)")
        elif cross_attention:
            raise ValueError("cross_attention needs output_stage=True: the attention backward starts from the output "
                             "stage's two row gradients")
        if self_block:
            if not cross_attention:
                raise ValueError("self_block needs cross_attention=True: the self block's backward starts from the "
                                 "complete gradient at the rows the cross block reads")
            missing = [k for k in ("self_block_context0", "self_block_context1", "self_block_cos", "self_block_sin")
                       if k not in pred]
            if missing:
                raise ValueError(f"self_block needs {missing} in the prediction: call "
                                 "forward_layers(data, keep_output_stage=True, keep_self_block=True)")
        lp.open(data, "gfc_lg_head_backward", "gfc_lg_token_backward",
                *(("gfc_lg_cross_attn_backward",) if cross_attention else ()),
                *(("gfc_lg_self_attn_backward",) if self_block else ()),
                by_rows=("gfc_lg_ffn_backward",) if output_stage else ())
        if grad_total is None:
            gtot = torch.full((b,), 1.0 / b, device=device)
        else:
            gtot = grad_total.to(device=device, dtype=torch.float32).contiguous()
            if tuple(gtot.shape) != (b,):
                raise ValueError(f"grad_total must be [{b}], got {tuple(gtot.shape)}")
        # every nll is divided by the sum of the weights (lightglue.py:626), in float64
        weights = lp.weights + [1.0]
        g = (torch.tensor(weights, dtype=torch.float64) / sum(weights)).float().to(device)[:, None] * gtot[None]  # [L,B]
        dwf, dbf = torch.empty((nl, d, d), device=device), torch.empty((nl, d), device=device)
        dwm, dbm = torch.empty((nl, 1, d), device=device), torch.empty((nl, 1), device=device)
        dtw, dtb = torch.empty((max(nl - 1, 0), 1, d), device=device), torch.empty((max(nl - 1, 0), 1), device=device)
        dx = torch.empty((nl, rows, d), device=device) if descriptor_grads else None
        # head L - 1's direct gradient, for that layer only when the whole buffer is not asked for
        dy = None if not output_stage else dx[nl - 1] if dx is not None else torch.empty((rows, d), device=device)
        # ... and head L - 2's, which completes the gradient at the last layer's input rows
        dy_in = None if not self_block else dx[nl - 2] if dx is not None else torch.empty((rows, d), device=device)
        correct = torch.empty((rows,), device=device, dtype=torch.uint8)
        sc = torch.empty((b, 6), device=device)
        for i in range(nl):
            x = lp.layer_rows(i)
            own = dy if i == nl - 1 else dy_in if i == nl - 2 else None
            nat.call("gfc_lg_head_backward", ctypes.byref(lp.params), i, x, x[lp.bm:], lp.gt0, lp.gt1, lp.gta, g[i],
                     lp.balancing, b, m, n, dwf[i], dbf[i], dwm[i], dbm[i],
                     own if own is not None else None if dx is None else dx[i], lp.ws, lp.ws.numel())
            if i == nl - 1:
                break
            lp.assign(i, x)
            lp.token_logits(i, x)
            lp.layer_scores(0.5, sc, correct)
            nat.call("gfc_lg_token_backward", x, x[lp.bm:], lp.logits, lp.logits[lp.bm:], correct, correct[lp.bm:], gtot,
                     nl, b, m, n, dtw[i], dtb[i], lp.ws, lp.ws.numel())
        grads = {}
        for i in range(nl):
            grads[f"log_assignment.{i}.final_proj.weight"], grads[f"log_assignment.{i}.final_proj.bias"] = dwf[i], dbf[i]
            grads[f"log_assignment.{i}.matchability.weight"] = dwm[i]
            grads[f"log_assignment.{i}.matchability.bias"] = dbm[i]
        for i in range(nl - 1):
            grads[f"token_confidence.{i}.token.0.weight"], grads[f"token_confidence.{i}.token.0.bias"] = dtw[i], dtb[i]
        rows_out, x_mid, ctx = self._output_stage_backward(lp, dy, grads) if output_stage else (None, None, None)
        dx_mid = self._cross_attention_backward(lp, x_mid, ctx, rows_out, grads) if cross_attention else None
        dx_self = self._self_block_backward(lp, dx_mid, grads) if self_block else None
        if accumulate:
            for name, grad in grads.items():
                param = self.get_parameter(name)
                grad = grad.to(device=param.device, dtype=param.dtype)
                if param.grad is None:
                    param.grad = grad.clone()
                else:
                    param.grad += grad
        if dx is not None:
            put_sides(grads, "grad_ref_descriptors", stacked_sides(dx, b, m, n))
        if rows_out is not None:
            put_sides(grads, "grad_output_stage_rows", split_sides(rows_out[0], b, m, n))
            put_sides(grads, "grad_output_stage_context", split_sides(rows_out[1], b, m, n))
        if dx_mid is not None:
            put_sides(grads, "grad_cross_block_rows", split_sides(dx_mid, b, m, n))
        if dx_self is not None:
            put_sides(grads, "grad_self_block_rows", split_sides(dx_self, b, m, n))
            put_sides(grads, "grad_layer_input_rows", split_sides(dx_self + dy_in, b, m, n))
        return grads

    # the last cross block's parameters behind its output stage, by their names under transformers.{L-1}.cross_attn.
    _OUTPUT_STAGE = ("to_out.weight", "to_out.bias", "ffn.0.weight", "ffn.0.bias", "ffn.1.weight", "ffn.1.bias",
                     "ffn.3.weight", "ffn.3.bias")

    def _output_stage_backward(self, lp, dy, grads):
        """Head L - 1's direct gradient dy [B*M + B*N, 256] through the last layer's output stage (gfc_lg_ffn_backward on
        the rows and the context the prediction kept): the eight parameter gradients into `grads`; returns the kernel's
        two row outputs [2, B*M + B*N, 256], and the packed rows and context it read."""
        pred, rows, d = lp.pred, lp.rows, lp.d
        w = self._output_stage_weights(lp.device)
        x = pack_sides(pred["output_stage_rows0"].float().contiguous(), pred["output_stage_rows1"].float().contiguous())
        ctx = pack_sides(pred["output_stage_context0"].float().contiguous(),
                         pred["output_stage_context1"].float().contiguous())
        if tuple(x.shape) != (rows, d) or tuple(ctx.shape) != (rows, d):
            raise ValueError(f"the kept output stage {tuple(x.shape)} / {tuple(ctx.shape)} does not fit the "
                             f"descriptors ({rows} rows)")
        og = {name: torch.empty_like(w[name]) for name in self._OUTPUT_STAGE}
        rows_out = torch.empty((2, rows, d), device=lp.device)
        nat.call("gfc_lg_ffn_backward", x, ctx, dy, w["to_out.weight"], w["to_out.bias"], w["ffn.0.weight"],
                 w["ffn.0.bias"], w["ffn.1.weight"], w["ffn.1.bias"], w["ffn.3.weight"], rows, og["to_out.weight"],
                 og["to_out.bias"], og["ffn.0.weight"], og["ffn.0.bias"], og["ffn.1.weight"], og["ffn.1.bias"],
                 og["ffn.3.weight"], og["ffn.3.bias"], rows_out[0], rows_out[1], lp.ws, lp.ws.numel())
        for name in self._OUTPUT_STAGE:
            grads[f"transformers.{lp.nl - 1}.cross_attn.{name}"] = og[name]
        return rows_out, x, ctx

    # ... and in front of its attention
    _CROSS_ATTENTION = ("to_qk.weight", "to_qk.bias", "to_v.weight", "to_v.bias")

    def _cross_attention_backward(self, lp, x, ctx, rows_out, grads):
        """The output stage's two row gradients (rows_out[0] at the rows through the residual and the concatenation,
        rows_out[1] at the context) through the last cross block's attention (gfc_lg_cross_attn_backward on the packed
        rows x and context ctx the prediction kept): the four parameter gradients into `grads`; returns the complete
        gradient at x [B*M + B*N, 256]."""
        w = self._cross_attention_weights(lp.device)
        ag = {name: torch.empty_like(w[name]) for name in self._CROSS_ATTENTION}
        dx = torch.empty((lp.rows, lp.d), device=lp.device)
        nat.call("gfc_lg_cross_attn_backward", x, ctx, rows_out[1], rows_out[0], w["to_qk.weight"], w["to_qk.bias"],
                 w["to_v.weight"], w["to_v.bias"], lp.b, lp.m, lp.n, ag["to_qk.weight"], ag["to_qk.bias"],
                 ag["to_v.weight"], ag["to_v.bias"], dx, lp.ws, lp.ws.numel())
        for name in self._CROSS_ATTENTION:
            grads[f"transformers.{lp.nl - 1}.cross_attn.{name}"] = ag[name]
        return dx

    # the last SELF block: its FFN part by the names the output stage has (out_proj in the place of to_out) ...
    _SELF_STAGE = ("out_proj.weight", "out_proj.bias", "ffn.0.weight", "ffn.0.bias", "ffn.1.weight", "ffn.1.bias",
                   "ffn.3.weight", "ffn.3.bias")

    def _self_block_backward(self, lp, dy, grads):
        """The complete gradient dy [B*M + B*N, 256] at the last self block's output through that block: its FFN part
        (gfc_lg_ffn_backward on the rows of layer L - 2 and the self context the prediction kept), then its rotary
        attention and Wqkv (gfc_lg_self_attn_backward on the packed Wqkv the forward reads): the ten parameter
        gradients into `grads`, Wqkv's mapped back to state-dict row order; returns the gradient at the block's input
        rows [B*M + B*N, 256]."""
        pred, rows, d, device, l = lp.pred, lp.rows, lp.d, lp.device, lp.nl - 1
        w = self._self_block_weights(device)
        x = lp.layer_rows(l - 1)
        ctx = pack_sides(pred["self_block_context0"].float().contiguous(), pred["self_block_context1"].float().contiguous())
        cos, sin = pred["self_block_cos"].float().contiguous(), pred["self_block_sin"].float().contiguous()
        if tuple(ctx.shape) != (rows, d) or tuple(cos.shape) != (rows, 64) or tuple(sin.shape) != (rows, 64):
            raise ValueError(f"the kept self block {tuple(ctx.shape)} / {tuple(cos.shape)} / {tuple(sin.shape)} does not "
                             f"fit the descriptors ({rows} rows)")
        sg = {name: torch.empty_like(w[name]) for name in self._SELF_STAGE}
        rows_out = torch.empty((2, rows, d), device=device)
        nat.call("gfc_lg_ffn_backward", x, ctx, dy, w["out_proj.weight"], w["out_proj.bias"], w["ffn.0.weight"],
                 w["ffn.0.bias"], w["ffn.1.weight"], w["ffn.1.bias"], w["ffn.3.weight"], rows, sg["out_proj.weight"],
                 sg["out_proj.bias"], sg["ffn.0.weight"], sg["ffn.0.bias"], sg["ffn.1.weight"], sg["ffn.1.bias"],
                 sg["ffn.3.weight"], sg["ffn.3.bias"], rows_out[0], rows_out[1], lp.ws, lp.ws.numel())
        # Wqkv in the packed row order, where the forward reads it; its gradient comes out in that order
        by_ptr = {t.data_ptr(): t for t in self._packed[1]}
        wqkv, bqkv = by_ptr[lp.params.wqkv[l]], by_ptr[lp.params.bqkv[l]]
        dw, db = torch.empty_like(wqkv), torch.empty_like(bqkv)
        dx = torch.empty((rows, d), device=device)
        nat.call("gfc_lg_self_attn_backward", x, cos, sin, ctx, rows_out[1], rows_out[0], wqkv, bqkv, lp.b, lp.m, lp.n, dw,
                 db, dx, lp.ws, lp.ws.numel())
        pre = f"transformers.{l}.self_attn."
        for name in self._SELF_STAGE:
            grads[pre + name] = sg[name]
        src = w["packed_rows"]  # packed row r holds state-dict row src[r]
        grads[pre + "Wqkv.weight"] = torch.empty_like(dw).index_copy_(0, src, dw)
        grads[pre + "Wqkv.bias"] = torch.empty_like(db).index_copy_(0, src, db)
        return dx

    def _wqkv_rows(self):
        """src[packed row] = state-dict row of Wqkv: packed s*d + head*dh + dd <- head*(3*dh) + dd*3 + s (`_pack`)."""
        d, dh = self.conf.descriptor_dim, self.conf.descriptor_dim // self.conf.num_heads
        idx = torch.arange(3 * d)
        s_, rem = idx // d, idx % d
        return (rem // dh) * (3 * dh) + (rem % dh) * 3 + s_

    def _self_stage_params(self):
        sa = self.transformers[self.conf.n_layers - 1].self_attn
        return {name: sa.get_parameter(name) for name in self._SELF_STAGE}

    def _self_block_weights(self, device):
        """fp32 device copies of the UNFOLDED `out_proj` / `ffn` parameters of the last self block, as
        `_output_stage_weights` holds the cross block's, and `packed_rows`, the index of `_wqkv_rows` on the device."""
        return self._derive("selfb", lambda: {
            **{name: p.detach().to(device=device, dtype=torch.float32).contiguous()
               for name, p in self._self_stage_params().items()}, "packed_rows": self._wqkv_rows().to(device)})

    def _cross_attention_params(self):
        ca = self.transformers[self.conf.n_layers - 1].cross_attn
        return {name: ca.get_parameter(name) for name in self._CROSS_ATTENTION}

    def _cross_attention_weights(self, device):
        """fp32 device copies of `to_qk` and `to_v` of the last cross block, as `_output_stage_weights` holds its own."""
        return self._derive("cross", lambda: {name: p.detach().to(device=device, dtype=torch.float32).contiguous()
                                              for name, p in self._cross_attention_params().items()})

    def _output_stage_params(self):
        ca = self.transformers[self.conf.n_layers - 1].cross_attn
        return {name: ca.get_parameter(name) for name in self._OUTPUT_STAGE}

    def _output_stage_weights(self, device):
        """fp32 device copies of the UNFOLDED parameters of the output stage (a parameter that already lives on the
        device in fp32 is read where it is), created on first use for the packed weights in force."""
        return self._derive("stage", lambda: {name: p.detach().to(device=device, dtype=torch.float32).contiguous()
                                              for name, p in self._output_stage_params().items()})

    def heads_updated(self):
        """Call after parameters of the assignment heads or exit tokens were changed in place (optimizer.step()): the
        device copies the kernels read are refreshed IN PLACE, at the addresses captured graphs replay, so `forward`,
        `forward_pairs` and `forward_layers` give what a fresh module loaded from `state_dict()` gives.  The trunk's
        packed weights are not rebuilt.  (A parameter that already lives on the device in fp32 is read by the kernels
        where it is: only its fp16 copy needs the refresh.)"""
        if self._packed is None:
            return
        with torch.no_grad():
            for param, t32, t16 in self._packed[3]:
                if t32.data_ptr() != param.data_ptr():
                    t32.copy_(param.detach().reshape(t32.shape))
                if t16 is not None:
                    t16.copy_(t32)

    def output_stage_updated(self):
        """Call after the parameters of the last layer's output stage (`to_out` and `ffn` of its cross block) were
        changed in place (optimizer.step()): `to_out` is folded into `ffn[0]` again by the function `_pack` uses, on the
        same device, and W0', b0', gamma, beta, W3, b3 (and `to_out` itself without fold_out_proj) are written into the
        packed device copies IN PLACE, at the addresses captured graphs replay; fp16 copies are rounded again from the
        fp32 ones and the unfolded copies the backward reads are refreshed.  The result is what a fresh module loaded
        from `state_dict()` packs, bit for bit; nothing else of the packed weights is touched."""
        if self._packed is None:
            return
        p, l = self._packed[0], self.conf.n_layers - 1
        by_ptr = {t.data_ptr(): t for t in self._packed[1]}
        ca = self.transformers[l].cross_attn
        w0, b0 = self._fold_ffn0(ca.ffn[0], ca.to_out)
        items = [(w0, p.c_ffn0_w[l], p.c_ffn0_w16[l]), (b0, p.c_ffn0_b[l], None), (ca.ffn[1].weight, p.c_ln_g[l], None),
                 (ca.ffn[1].bias, p.c_ln_b[l], None), (ca.ffn[3].weight, p.c_ffn3_w[l], p.c_ffn3_w16[l]),
                 (ca.ffn[3].bias, p.c_ffn3_b[l], None)]
        if not bool(self.conf.fold_out_proj):
            items += [(ca.to_out.weight, p.c_out_w[l], p.c_out_w16[l]), (ca.to_out.bias, p.c_out_b[l], None)]
        with torch.no_grad():
            for src, ptr, ptr16 in items:
                t32 = by_ptr[ptr]
                if t32.data_ptr() != src.data_ptr():
                    t32.copy_(src.detach().reshape(t32.shape))
                if ptr16:
                    by_ptr[ptr16].copy_(t32)
            stage = self._derived.stage
            if stage is not None and stage[0] is self._packed:
                for name, param in self._output_stage_params().items():
                    t = stage[1][name]
                    if t.data_ptr() != param.data_ptr():
                        t.copy_(param.detach())

    def self_block_updated(self):
        """Call after the ten parameters of the last layer's SELF block were changed in place (optimizer.step()): the
        packed `wqkv` / `bqkv` (rows permuted by `_pack`'s index), `out_proj` folded into `ffn[0]` again by the function
        `_pack` uses (or `out_proj` itself without fold_out_proj), gamma, beta, W3, b3 are written into the packed device
        copies IN PLACE, at the addresses captured graphs replay; fp16 copies are rounded again from the fp32 ones and the
        unfolded copies the backward reads are refreshed.  The result is what a fresh module loaded from `state_dict()`
        packs, bit for bit; nothing else of the packed weights is touched."""
        if self._packed is None:
            return
        p, l = self._packed[0], self.conf.n_layers - 1
        by_ptr = {t.data_ptr(): t for t in self._packed[1]}
        sa = self.transformers[l].self_attn
        src = self._wqkv_rows()
        w0, b0 = self._fold_ffn0(sa.ffn[0], sa.out_proj)
        items = [(sa.Wqkv.weight[src], p.wqkv[l], p.wqkv16[l]), (sa.Wqkv.bias[src], p.bqkv[l], None),
                 (w0, p.s_ffn0_w[l], p.s_ffn0_w16[l]), (b0, p.s_ffn0_b[l], None), (sa.ffn[1].weight, p.s_ln_g[l], None),
                 (sa.ffn[1].bias, p.s_ln_b[l], None), (sa.ffn[3].weight, p.s_ffn3_w[l], p.s_ffn3_w16[l]),
                 (sa.ffn[3].bias, p.s_ffn3_b[l], None)]
        if not bool(self.conf.fold_out_proj):
            items += [(sa.out_proj.weight, p.s_out_w[l], p.s_out_w16[l]), (sa.out_proj.bias, p.s_out_b[l], None)]
        with torch.no_grad():
            for t, ptr, ptr16 in items:
                t32 = by_ptr[ptr]
                if t32.data_ptr() != t.data_ptr():
                    t32.copy_(t.detach().reshape(t32.shape))
                if ptr16:
                    by_ptr[ptr16].copy_(t32)
            selfb = self._derived.selfb
            if selfb is not None and selfb[0] is self._packed:
                for name, param in self._self_stage_params().items():
                    t = selfb[1][name]
                    if t.data_ptr() != param.data_ptr():
                        t.copy_(param.detach())

    def cross_attention_updated(self):
        """Call after `to_qk` / `to_v` of the last layer's cross block were changed in place (optimizer.step()): the
        packed [to_qk; to_v] weight and bias of that layer are written again IN PLACE, at the addresses captured graphs
        replay, the fp16 copy is rounded again from the fp32 one and the copies the backward reads are refreshed.  The
        result is what a fresh module loaded from `state_dict()` packs, bit for bit; nothing else is touched."""
        if self._packed is None:
            return
        p, l, d = self._packed[0], self.conf.n_layers - 1, self.conf.descriptor_dim
        by_ptr = {t.data_ptr(): t for t in self._packed[1]}
        ca = self.transformers[l].cross_attn
        with torch.no_grad():
            w32, b32 = by_ptr[p.c_qkv_w[l]], by_ptr[p.c_qkv_b[l]]
            for t32, qk, v in ((w32, ca.to_qk.weight, ca.to_v.weight), (b32, ca.to_qk.bias, ca.to_v.bias)):
                t32[:d].copy_(qk.detach())
                t32[d:].copy_(v.detach())
            if p.c_qkv_w16[l]:
                by_ptr[p.c_qkv_w16[l]].copy_(w32)
            cross = self._derived.cross
            if cross is not None and cross[0] is self._packed:
                for name, param in self._cross_attention_params().items():
                    t = cross[1][name]
                    if t.data_ptr() != param.data_ptr():
                        t.copy_(param.detach())
