"""LightGlue matcher on MI355X -- drop-in for `gluefactory.models.matchers.lightglue`
(reference file gluefactory/models/matchers/lightglue.py:322-640, inference path).

Same configuration keys, same `forward(data) -> dict` contract (lightglue.py:422-553) and
the same state-dict key names (lightglue.py:349-408), including the legacy
`self_attn.{i}` -> `transformers.{i}.self_attn` rename (lightglue.py:394-401), so the official
`superpoint_lightglue.pth` / `disk_lightglue.pth` load unchanged.  Like the reference class it
is a plain nn.Module (not a BaseModel) resolved through `__main_model__`.  The torch
sub-modules are parameter containers only; the forward pass is one call into libgfc_amd.so.  The losses, the
kept-layers forward and the gradients (`loss`, `forward_layers`, `layer_loss`, `layer_loss_backward`, `heads_updated`,
`output_stage_updated`) are the mix-in of `lightglue_training.py`.

    model.matcher.name = glue_factory_colon_amd.lightglue
"""
import copy
import ctypes
import itertools
import sys
import threading
from pathlib import Path

import torch
from torch import nn

from . import _native as nat
from . import weights as _weights
from ._rows import match_outputs, pack_sides, split_sides
from .base_model import Conf, merge
from .lightglue_training import LightGlueTraining


def _ffn(d):
    return nn.Sequential(nn.Linear(2 * d, 2 * d), nn.LayerNorm(2 * d, elementwise_affine=True), nn.GELU(),
                         nn.Linear(2 * d, d))


class _SelfBlock(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.Wqkv = nn.Linear(d, 3 * d)
        self.out_proj = nn.Linear(d, d)
        self.ffn = _ffn(d)


class _CrossBlock(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.to_qk = nn.Linear(d, d)
        self.to_v = nn.Linear(d, d)
        self.to_out = nn.Linear(d, d)
        self.ffn = _ffn(d)


class _Layer(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.self_attn = _SelfBlock(d)
        self.cross_attn = _CrossBlock(d)


class _PosEnc(nn.Module):
    def __init__(self, m, f_dim):
        super().__init__()
        self.Wr = nn.Linear(m, f_dim // 2, bias=False)


class _Assignment(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.matchability = nn.Linear(d, 1)
        self.final_proj = nn.Linear(d, d)


class _TokenConfidence(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.token = nn.Sequential(nn.Linear(d, 1), nn.Sigmoid())


_CAPTURE_LOCK = threading.Lock()  # one stream capture at a time per process


def _image_size(data, side):
    """`view{side}.image_size` like the reference (lightglue.py:430-434); a view without one normalises by the extent
    of its own key points (normalize_keypoints, lightglue.py:31-32).  (The reference leaves the size unbound when a
    view is absent; here that is treated like a missing size.)"""
    size = data.get("view" + side, {}).get("image_size")
    kp = data["keypoints" + side]
    if size is None and kp.shape[-2] > 0:
        size = 1 + kp.float().amax(-2) - kp.float().amin(-2)
    return size


class _Derived:
    """What is worked out once from one set of packed weights and replaced with them.  Every entry is (the packed
    weights it was made for, value), so an entry is never used with other weights than its own (`LightGlue._derive`)."""

    def __init__(self):
        self.thresholds = None  # confidence_thresholds as a host list
        self.stage = None  # the output stage's unfolded fp32 device copies, by name (lightglue_training.py)
        self.cross = None  # to_qk / to_v of the last cross block, fp32 device copies, by name (lightglue_training.py)
        self.selfb = None  # out_proj / ffn of the last self block, fp32 device copies, by name (lightglue_training.py)


class LightGlue(LightGlueTraining, nn.Module):
    default_conf = {
        "name": "lightglue",
        "input_dim": 256,
        "add_scale_ori": False,
        "descriptor_dim": 256,
        "n_layers": 9,
        "num_heads": 4,
        "flash": False,
        "mp": False,
        "depth_confidence": -1,
        "width_confidence": -1,
        "filter_threshold": 0.0,
        "checkpointed": False,
        "weights": None,  # path of a checkpoint, or "synthetic[:seed]" for the name-seeded weights
        "weights_from_version": "v0.1_arxiv",
        "loss": {"gamma": 1.0, "fn": "nll", "nll_balancing": 0.5},
        # MI355X-specific: fold out_proj / to_out into the first FFN matrix at load time (one GEMM and one
        # [rows,256] HBM round trip less per block; same function, rounding differs by ~1e-7 relative)
        "fold_out_proj": True,
        # MI355X-specific, opt-in: problems of at most this many rows (b * (m + n); batch-1 evaluation: 2048) replay the
        # matcher's ~100 launches as ONE captured HIP graph per (b, m, n) (static buffers, inputs copied in, outputs
        # copied out).  Same kernels, same results.  0 (default) = eager launches: measured at batch 1 the graph saves
        # 0.05 of 1.65 ms per pair (the matcher is bound by its small grids, not by launch gaps),
        # and HIP refuses concurrent captures from several host threads (export_predictions(workers > 1)).
        "graph_max_rows": 0,
        # MI355X-specific, opt-in: "fp16" runs every matrix product of the matcher on the fp16 MFMA (fp16 operands
        # rounded to nearest even, fp32 sums); positional encoding, soft-max statistics, LayerNorm, GELU, residuals,
        # the row buffer and the assignment's log double soft-max stay fp32 ("fp16 matcher").  "fp32"
        # (default): every contraction in exact fp32.  `mp` keeps the reference class's meaning here (none).
        "matmul_precision": "fp32",
        # MI355X-specific, opt-in: `forward_pairs` runs its adaptive (depth_confidence / width_confidence) batch-1 items
        # as ONE pass -- the layers over the live rows of all pairs, the stop / prune decisions and the re-pack between
        # two layers on the device (gfc_lg_adaptive_step), one small device->host read per layer for the whole batch
        # instead of several per pair.  Same decisions on the same bits as the pair-by-pair path.  False (default):
        # adaptive pairs take the single-pair path, as before.  `forward()` is not affected.
        "adaptive_pair_batch": False,
    }
    required_data_keys = ["keypoints0", "keypoints1", "descriptors0", "descriptors1"]

    def __init__(self, conf) -> None:
        super().__init__()
        self.conf = conf = Conf(merge(self.default_conf, conf))
        if conf.descriptor_dim != 256 or conf.num_heads != 4:
            raise NotImplementedError("the MI355X kernels are built for descriptor_dim 256, 4 heads (head_dim 64)")
        if conf.matmul_precision not in ("fp32", "fp16"):
            raise ValueError(f"matmul_precision must be 'fp32' or 'fp16', not {conf.matmul_precision!r}")
        if conf.n_layers > nat.GFC_LG_MAX_LAYERS:
            raise NotImplementedError(f"at most {nat.GFC_LG_MAX_LAYERS} layers")
        if conf.input_dim != conf.descriptor_dim:
            if conf.input_dim % 32:
                raise NotImplementedError("input_dim must be a multiple of 32")
            self.input_proj = nn.Linear(conf.input_dim, conf.descriptor_dim, bias=True)
        else:
            self.input_proj = nn.Identity()
        d, n = conf.descriptor_dim, conf.n_layers
        head_dim = d // conf.num_heads
        self.posenc = _PosEnc(2 + 2 * bool(conf.add_scale_ori), head_dim)  # lightglue.py:358-360
        self.transformers = nn.ModuleList([_Layer(d) for _ in range(n)])
        self.log_assignment = nn.ModuleList([_Assignment(d) for _ in range(n)])
        self.token_confidence = nn.ModuleList([_TokenConfidence(d) for _ in range(n - 1)])
        self.register_buffer("confidence_thresholds", _weights.confidence_thresholds(n))
        self._set_packed(None)
        self._ws = nat.Workspace()
        self.trace = None  # optional nat.KernelTrace (bench.py): per-launch events of the attention kernel
        self._report_host = None  # pinned [GFC_LG_MAX_RAGGED_PAIRS, 4] int32: the adaptive step's report lands here
        self.are_weights_initialized = False

        w = conf.weights
        if w is not None:
            if Path(str(w)).exists():
                self.load_state_dict(torch.load(str(w), map_location="cpu"), strict=False)
            elif isinstance(w, str) and w.startswith("synthetic"):
                seed = int(w.split(":")[1]) if ":" in w else 0
                self.load_state_dict(_weights.lightglue_state_dict(seed, input_dim=conf.input_dim, n_layers=n,
                                                                   add_scale_ori=bool(conf.add_scale_ori)), strict=False)
            else:
                # the reference downloads `{weights}_lightglue.pth` here (lightglue.py:385-392); no network
                raise FileNotFoundError(f"weights {w!r} not found (no download is attempted)")

    # -- weights ------------------------------------------------------------------------
    def load_state_dict(self, state_dict, *args, **kwargs):
        for i in range(self.conf.n_layers):  # legacy key names, lightglue.py:394-401
            state_dict = {k.replace(f"self_attn.{i}", f"transformers.{i}.self_attn"): v for k, v in state_dict.items()}
            state_dict = {k.replace(f"cross_attn.{i}", f"transformers.{i}.cross_attn"): v
                          for k, v in state_dict.items()}
        ret = super().load_state_dict(state_dict, *args, **kwargs)
        self._set_packed(None)
        self.are_weights_initialized = True
        return ret

    def _apply(self, fn, *args, **kwargs):
        self._set_packed(None)
        return super()._apply(fn, *args, **kwargs)

    def _set_packed(self, packed):
        """New packed weights (None: they are built on the next use), and with them nothing that was made for the old
        ones: the captured graphs ((b, m, n, device, has scale/ori) -> launch sequence + its static buffers) and the
        derived state."""
        self._packed = packed
        self._graphs = {}
        self._derived = _Derived()

    def is_initialized(self):
        return self.are_weights_initialized

    def __deepcopy__(self, memo):
        """Replicas (export_predictions workers) get their own parameters and workspaces; captured graphs and packed
        weight pointers belong to the original and are rebuilt by the copy on first use."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_graphs":
                new.__dict__[k] = {}
            elif k == "_derived":
                new.__dict__[k] = _Derived()
            elif k in ("_packed", "_report_host"):
                new.__dict__[k] = None
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    # -- small problems: the whole launch sequence as one HIP graph ------------------------
    def _launch_packed(self, kp, de, s0, s1, so, b, m, n, m0, m1, ms0, ms1, scores, rows, ws, trace=None):
        nat.call("gfc_lg_forward_packed", ctypes.byref(self._packed[0]), kp, de, s0, s1, so, b, m, n,
                 float(self.conf.filter_threshold), m0, m1, ms0, ms1, scores, rows, ws, ws.numel(),
                 ctypes.byref(trace.c) if trace is not None else None)

    def _graph_entry(self, key, kp, de, s0, s1, so, b, m, n):
        """Static buffers + the captured launch sequence of gfc_lg_forward_packed for one problem shape."""
        device, d = kp.device, self.conf.descriptor_dim
        m0, m1, ms0, ms1, scores = match_outputs(b, m, n, device)
        e = {"kp": torch.empty_like(kp), "de": torch.empty_like(de), "s0": torch.empty_like(s0),
             "s1": torch.empty_like(s1), "so": None if so is None else torch.empty_like(so),
             "m0": m0, "m1": m1, "ms0": ms0, "ms1": ms1, "scores": scores,
             "rows": torch.empty((b * (m + n), d), device=device),
             "ws": torch.empty(nat.call("gfc_lg_packed_workspace_bytes", b, m, n), dtype=torch.uint8, device=device)}
        for name, src in (("kp", kp), ("de", de), ("s0", s0), ("s1", s1), ("so", so)):
            if src is not None:
                e[name].copy_(src)

        def run():
            self._launch_packed(e["kp"], e["de"], e["s0"], e["s1"], e["so"], b, m, n, e["m0"], e["m1"], e["ms0"],
                                e["ms1"], e["scores"], e["rows"], e["ws"])

        # one eager run first (per-kernel attributes are set on first use), then the capture
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream(device).wait_stream(side)
        try:
            with _CAPTURE_LOCK:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    run()
            e["graph"] = graph
        except (nat.NativeError, RuntimeError) as exc:
            # RuntimeError: the capture was refused (another thread is using the device).  NativeError: raised by run()
            # inside the `with` block, i.e. always while this stream was capturing -- the eager run above has just
            # proved the same launch sequence on the same buffers, so the failure is specific to capture.  Either way
            # this shape runs with eager launches from now on (the caller does that run: nothing is repeated here), and
            # the reason is logged once per kind, never hidden.
            kind = "launch failed under capture" if isinstance(exc, nat.NativeError) else "capture refused"
            logged = LightGlue.__dict__.get("_graph_fallback_logged") or set()
            if kind not in logged:
                LightGlue._graph_fallback_logged = logged | {kind}
                print(f"glue_factory_colon_amd.lightglue: HIP graph {kind} ({exc}); problems of shape "
                      f"{key[:3]} run with eager launches", file=sys.stderr)
            e = {"graph": None}
        self._graphs[key] = e
        return e

    def _pack(self, device):
        conf = self.conf
        keep = []

        def dev(t):
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        half = conf.matmul_precision == "fp16"

        def dev2(t):
            """fp32 device copy of a matrix and, in fp16 mode, its fp16 copy: rounded once, to nearest even, from the
            fp32 matrix (after any out_proj fold).  Returns both pointers (the second None in fp32 mode)."""
            ptr = dev(t)
            if not half:
                return ptr, None
            t16 = keep[-1].half()
            keep.append(t16)
            return ptr, t16.data_ptr()

        p = nat.LgParams()
        p.n_layers, p.input_dim = conf.n_layers, conf.input_dim
        p.precision = nat.GFC_LG_FP16 if half else nat.GFC_LG_FP32
        if conf.input_dim != conf.descriptor_dim:
            p.input_proj_w, p.input_proj_w16 = dev2(self.input_proj.weight)
            p.input_proj_b = dev(self.input_proj.bias)
        p.posenc_wr = dev(self.posenc.Wr.weight)
        p.posenc_dim = 4 if self.conf.add_scale_ori else 2
        d, h = conf.descriptor_dim, conf.num_heads
        dh = d // h
        # Wqkv rows: state-dict row = head*(3*dh) + dd*3 + s  ->  packed row = s*d + head*dh + dd
        idx = torch.arange(3 * d)
        s_, rem = idx // d, idx % d
        head, dd = rem // dh, rem % dh
        src = head * (3 * dh) + dd * 3 + s_
        fold = bool(conf.fold_out_proj)
        ffn0 = self._fold_ffn0

        for i, layer in enumerate(self.transformers):
            sa, ca = layer.self_attn, layer.cross_attn
            p.wqkv[i], p.wqkv16[i] = dev2(sa.Wqkv.weight[src])
            p.bqkv[i] = dev(sa.Wqkv.bias[src])
            if not fold:
                p.s_out_w[i], p.s_out_w16[i] = dev2(sa.out_proj.weight)
                p.s_out_b[i] = dev(sa.out_proj.bias)
                p.c_out_w[i], p.c_out_w16[i] = dev2(ca.to_out.weight)
                p.c_out_b[i] = dev(ca.to_out.bias)
            w0, b0 = ffn0(sa.ffn[0], sa.out_proj)
            p.s_ffn0_w[i], p.s_ffn0_w16[i] = dev2(w0)
            p.s_ffn0_b[i] = dev(b0)
            p.s_ln_g[i], p.s_ln_b[i] = dev(sa.ffn[1].weight), dev(sa.ffn[1].bias)
            p.s_ffn3_w[i], p.s_ffn3_w16[i] = dev2(sa.ffn[3].weight)
            p.s_ffn3_b[i] = dev(sa.ffn[3].bias)
            p.c_qkv_w[i], p.c_qkv_w16[i] = dev2(torch.cat([ca.to_qk.weight, ca.to_v.weight], 0))
            p.c_qkv_b[i] = dev(torch.cat([ca.to_qk.bias, ca.to_v.bias], 0))
            w0, b0 = ffn0(ca.ffn[0], ca.to_out)
            p.c_ffn0_w[i], p.c_ffn0_w16[i] = dev2(w0)
            p.c_ffn0_b[i] = dev(b0)
            p.c_ln_g[i], p.c_ln_b[i] = dev(ca.ffn[1].weight), dev(ca.ffn[1].bias)
            p.c_ffn3_w[i], p.c_ffn3_w16[i] = dev2(ca.ffn[3].weight)
            p.c_ffn3_b[i] = dev(ca.ffn[3].bias)
        heads = []  # (parameter, its fp32 device copy, the fp16 copy of that or None): what heads_updated refreshes

        def head(param, flat=False, with_half=False):
            t = param.reshape(-1) if flat else param
            ptr, ptr16 = dev2(t) if with_half else (dev(t), None)
            heads.append((param, keep[-2] if ptr16 is not None else keep[-1], keep[-1] if ptr16 is not None else None))
            return ptr, ptr16

        for i, la in enumerate(self.log_assignment):
            p.final_proj_w[i], p.final_proj_w16[i] = head(la.final_proj.weight, with_half=True)
            p.final_proj_b[i] = head(la.final_proj.bias)[0]
            p.matchability_w[i] = head(la.matchability.weight, flat=True)[0]
            p.matchability_b[i] = head(la.matchability.bias)[0]
        for i, tc in enumerate(self.token_confidence):
            p.token_w[i], p.token_b[i] = head(tc.token[0].weight, flat=True)[0], head(tc.token[0].bias)[0]
        return p, keep, device, heads

    def _fold_ffn0(self, lin0, out):
        """ffn[0] weights with `out` (out_proj / to_out) folded into the message half when enabled."""
        if not bool(self.conf.fold_out_proj):
            return lin0.weight, lin0.bias
        d = self.conf.descriptor_dim
        w0, b0 = lin0.weight.detach().double(), lin0.bias.detach().double()
        wo, bo = out.weight.detach().double(), out.bias.detach().double()
        w = torch.cat([w0[:, :d], w0[:, d:] @ wo], 1)
        return w.float(), (b0 + w0[:, d:] @ bo).float()

    def _check_ready(self, data=None):
        if data is not None:
            for key in self.required_data_keys:
                assert key in data, f"Missing key {key} in data"
        if not self.are_weights_initialized:
            raise RuntimeError("LightGlue weights are not loaded (conf.weights or load_state_dict)")

    def _result(self, m0, m1, ms0, ms1, ref0, ref1, scores, prune0=None, prune1=None):
        n = self.conf.n_layers
        return {
            "matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1,
            "ref_descriptors0": ref0, "ref_descriptors1": ref1, "log_assignment": scores,
            "prune0": torch.full_like(ms0, n) if prune0 is None else prune0,
            "prune1": torch.full_like(ms1, n) if prune1 is None else prune1,
        }

    def ensure_packed(self, device):
        """The device copies of the weights in the library's layouts, built on the CALLING thread's current stream if
        they do not exist yet (export workers share them: the caller packs before its worker streams start)."""
        self._check_ready()
        if self._packed is None or self._packed[2] != device:
            self._set_packed(self._pack(device))
        return self._packed

    def _host_thresholds(self):
        """`confidence_thresholds` as a host list, read with the packed weights in force, once: no device-to-host read
        in the calls that follow."""
        return self._derive("thresholds", self.confidence_thresholds.tolist)

    def _derive(self, name, make):
        """Entry `name` of the derived state, made on first use with the packed weights in force."""
        entry = getattr(self._derived, name)
        if entry is None or entry[0] is not self._packed:
            entry = (self._packed, make())
            setattr(self._derived, name, entry)
        return entry[1]

    @property
    def _thresholds_host(self):
        """The entry behind `_host_thresholds` as it is held (None before the first read)."""
        return self._derived.thresholds

    def _empty_result(self, ref0, ref1):
        """The reference's early return for a side without key points (lightglue.py:298-303): all -1 / zeros, around the
        caller's zero descriptors ref0 [B,L,M,256] and ref1 [B,L,N,256]."""
        (b, _, m, _), n, device, zeros = ref0.shape, ref1.shape[2], ref0.device, torch.zeros
        return self._result(torch.full((b, m), -1, device=device, dtype=torch.long),
                            torch.full((b, n), -1, device=device, dtype=torch.long),
                            zeros((b, m), device=device), zeros((b, n), device=device), ref0, ref1,
                            zeros((b, m + 1, n + 1), device=device))

    # -- forward ------------------------------------------------------------------------
    def _uniform_rows(self, data):
        """A uniform batch as the library reads it: key points [B*M + B*N, 2], descriptors [.., input_dim] and
        (scale, orientation) [.., 2] (None without add_scale_ori) with the rows of side 0 first, and the image sizes
        [B,2] of both sides, all float32; the weights are packed for the device.  Five Nones when a side has no key
        points (the inputs are still checked)."""
        conf = self.conf
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        b, m, _ = kpts0.shape
        n = kpts1.shape[1]
        device = kpts0.device
        size0, size1 = _image_size(data, "0"), _image_size(data, "1")
        desc0 = data["descriptors0"].contiguous().float()
        desc1 = data["descriptors1"].contiguous().float()
        assert desc0.shape[-1] == conf.input_dim
        assert desc1.shape[-1] == conf.input_dim
        so0 = so1 = None
        if conf.add_scale_ori:  # lightglue.py:436-453: [x, y, scale, orientation] feeds the positional encoding
            def pack(sc, ori):
                sc = sc if sc.dim() == 3 else sc[..., None]
                ori = ori if ori.dim() == 3 else ori[..., None]
                return torch.cat([sc, ori], -1).to(device=device, dtype=torch.float32).contiguous()
            so0, so1 = pack(data["scales0"], data["oris0"]), pack(data["scales1"], data["oris1"])
        if m == 0 or n == 0:
            return None, None, None, None, None
        self.ensure_packed(device)
        s0 = torch.as_tensor(size0, device=device, dtype=torch.float32).expand(b, 2).contiguous()
        s1 = torch.as_tensor(size1, device=device, dtype=torch.float32).expand(b, 2).contiguous()
        # side-0 rows then side-1 rows: zero-copy when both views came out of ONE extractor call (adjacent
        # slices of one tensor), otherwise one concatenation each (tensor plumbing)
        kp = pack_sides(kpts0.contiguous().float(), kpts1.contiguous().float())
        de = pack_sides(desc0, desc1)
        so = pack_sides(so0, so1) if so0 is not None else None
        return kp, de, so, s0, s1

    def forward(self, data: dict) -> dict:
        self._check_ready(data)
        conf = self.conf
        if self.training:
            raise NotImplementedError("training (loss, checkpointing) is out of scope: inference path only")
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        nat.require_cuda(kpts0, "data['keypoints0']")
        b, m, _ = kpts0.shape
        b, n, _ = kpts1.shape
        device = kpts0.device
        if (conf.depth_confidence > 0 or conf.width_confidence > 0) and m > 0 and n > 0:
            return self._forward_adaptive(data)
        kp, de, so, s0, s1 = self._uniform_rows(data)
        d = conf.descriptor_dim
        if m == 0 or n == 0:  # ref_descriptors0/1 are the two halves of one row buffer, as below
            ref0, ref1 = split_sides(torch.zeros((b * (m + n), d), device=device), b, m, n)
            return self._empty_result(ref0.view(b, 1, m, d), ref1.view(b, 1, n, d))
        use_graph = 0 < b * (m + n) <= int(conf.graph_max_rows or 0) and self.trace is None
        if use_graph:
            key = (b, m, n, device.index, so is not None, torch.cuda.current_stream(device).cuda_stream)
            e = self._graphs.get(key) or self._graph_entry(key, kp, de, s0, s1, so, b, m, n)
            use_graph = e["graph"] is not None
        if use_graph:
            for name, src in (("kp", kp), ("de", de), ("s0", s0), ("s1", s1), ("so", so)):
                if src is not None:
                    e[name].copy_(src)
            e["graph"].replay()
            # the graph owns its buffers: the caller gets copies (plumbing; 6 MB at 1024 x 1024 points)
            m0, m1, ms0, ms1 = e["m0"].clone(), e["m1"].clone(), e["ms0"].clone(), e["ms1"].clone()
            scores, rows = e["scores"].clone(), e["rows"].clone()
        else:
            # every element of the outputs is written by gfc_lg_forward_packed: no fills
            m0, m1, ms0, ms1, scores = match_outputs(b, m, n, device)
            # one row buffer [b*m + b*n, 256]: the library's layers work in place on it and leave the last layer's
            # descriptors there; ref_descriptors0/1 are its two halves (no copy out)
            rows = torch.empty((b * (m + n), d), device=device)
            ws = self._ws.get(nat.call("gfc_lg_packed_workspace_bytes", b, m, n), device)
            self._launch_packed(kp, de, s0, s1, so, b, m, n, m0, m1, ms0, ms1, scores, rows, ws, self.trace)
        ref0, ref1 = split_sides(rows, b, m, n)
        return self._result(m0, m1, ms0, ms1, ref0.view(b, 1, m, d), ref1.view(b, 1, n, d), scores)

    # -- one view of a batch-1 item, rows of several views, the rows' way into the matcher --------
    def _side(self, item, side, device):
        """View `side` ("0" / "1") of a batch-1 input of `forward` as the library reads it, all float32: key points
        [m,2], descriptors [m,input_dim], (scale, orientation) [m,2] (None without add_scale_ori, lightglue.py:436-453)
        and the image size [1,2]."""
        kp = item["keypoints" + side][0].float()
        de = item["descriptors" + side][0].float()
        assert de.shape[-1] == self.conf.input_dim
        so = None
        if self.conf.add_scale_ori:
            sc, ori = item["scales" + side][0], item["oris" + side][0]
            so = torch.stack([sc.reshape(-1), ori.reshape(-1)], -1).float()
        size = torch.as_tensor(_image_size(item, side), device=device, dtype=torch.float32).reshape(-1, 2)[:1]
        return kp, de, so, size

    def _pack_views(self, views):
        """The rows of several `_side` views behind each other: key points, descriptors (a tensor of its own), scales /
        orientations (or None)."""
        kp = torch.cat([v[0] for v in views], 0).contiguous()
        de = torch.cat([v[1] for v in views], 0).contiguous()
        so = torch.cat([v[2] for v in views], 0).contiguous() if self.conf.add_scale_ori else None
        return kp, de, so

    def _input_proj(self, params, xin, out, rows):
        """out [rows,256] = input_proj(xin [rows,input_dim]) in the matcher's precision (lightglue.py:352-355,464-465)."""
        din, d = self.conf.input_dim, self.conf.descriptor_dim
        if params.precision == nat.GFC_LG_FP16:
            nat.call("gfc_linear_f16", xin, 0, din, din, None, 0, 0, 0, params.input_proj_w16, din, params.input_proj_b,
                     1.0, None, None, None, None, 0, out, 0, d, rows, d)
        else:
            nat.call("gfc_linear", xin, din, din, None, 0, 0, params.input_proj_w, din, params.input_proj_b, None, None,
                     1.0, None, None, None, 0, out, d, rows, d)

    # -- several pairs of DIFFERENT sizes through one launch sequence -----------------------------
    def forward_pairs(self, items: list) -> list:
        """MI355X addition: `[self(d) for d in items]` (each `d` a batch-1 input of `forward`) as ONE matcher pass.
        The reference's evaluation loop calls the matcher pair by pair only because the images of an HPatches-style
        list differ in size (utils/export_predictions.py:36-45, datasets/hpatches.py:60); LightGlue does not care
        about image sizes once the key points exist, so pairs with their own key-point counts run together through
        gfc_lg_forward_ragged: the layers over all rows at once, the assignment head per group of equal-shape pairs.
        Same arithmetic per pair; results are returned per pair in the order given.  Pairs without key points in one
        view and batch sizes other than 1 take the single-pair path; so does adaptive depth / width unless
        `adaptive_pair_batch` is set, which sends those pairs through `_forward_adaptive_pairs` together."""
        conf = self.conf
        adaptive = conf.depth_confidence > 0 or conf.width_confidence > 0
        batched = self._forward_ragged
        if adaptive:
            batched = self._forward_adaptive_pairs if conf.adaptive_pair_batch else None
        outs = [None] * len(items)
        rag = []
        for i, data in enumerate(items):
            self._check_ready(data)
            k0, k1 = data["keypoints0"], data["keypoints1"]
            if batched is None or k0.shape[0] != 1 or k0.shape[1] == 0 or k1.shape[1] == 0 or self.training:
                outs[i] = self(data)
            else:
                rag.append(i)
        for c in range(0, len(rag), nat.GFC_LG_MAX_RAGGED_PAIRS):
            chunk = rag[c:c + nat.GFC_LG_MAX_RAGGED_PAIRS]
            for i, out in zip(chunk, batched([items[i] for i in chunk])):
                outs[i] = out
        return outs

    def _forward_ragged(self, items):
        conf = self.conf
        device = items[0]["keypoints0"].device
        nat.require_cuda(items[0]["keypoints0"], "data['keypoints0']")
        self.ensure_packed(device)
        d = conf.descriptor_dim
        # equal shapes next to each other (stable): every run of equal (m, n) is one batched assignment head
        shapes = [(int(it["keypoints0"].shape[1]), int(it["keypoints1"].shape[1])) for it in items]
        order = sorted(range(len(items)), key=lambda i: shapes[i])
        groups = [(m, n, list(idx)) for (m, n), idx in itertools.groupby(order, key=lambda i: shapes[i])]
        view = {(i, side): self._side(items[i], side, device) for i in order for side in ("0", "1")}
        kp, de, so = self._pack_views([view[i, side] for _, _, idx in groups for side in ("0", "1") for i in idx])
        size0 = torch.cat([view[i, "0"][3] for i in order], 0).contiguous()
        size1 = torch.cat([view[i, "1"][3] for i in order], 0).contiguous()
        b = len(order)
        ms = [shapes[i][0] for i in order]
        ns = [shapes[i][1] for i in order]
        cm, cn = (ctypes.c_int32 * b)(*ms), (ctypes.c_int32 * b)(*ns)
        sm, sn = sum(ms), sum(ns)
        m0 = torch.empty((sm,), device=device, dtype=torch.long)
        m1 = torch.empty((sn,), device=device, dtype=torch.long)
        sc0, sc1 = torch.empty((sm,), device=device), torch.empty((sn,), device=device)
        scores = torch.empty((sum((a + 1) * (c + 1) for a, c in zip(ms, ns)),), device=device)
        rows = torch.empty((sm + sn, d), device=device)
        ws = self._ws.get(nat.call("gfc_lg_ragged_workspace_bytes", b, cm, cn), device)
        nat.call("gfc_lg_forward_ragged", ctypes.byref(self._packed[0]), kp, de, size0, size1, so, b, cm, cn,
                 float(conf.filter_threshold), m0, m1, sc0, sc1, scores, rows, ws, ws.numel(),
                 ctypes.byref(self.trace.c) if self.trace is not None else None)
        # per-pair views of the flat outputs; rows: group after group, side 0 then side 1 inside a group
        outs = [None] * b
        o0 = o1 = os_ = r = 0
        for m, n, idx in groups:
            cnt = len(idx)
            for j, i in enumerate(idx):
                outs[i] = self._result(
                    m0[o0:o0 + m].view(1, m), m1[o1:o1 + n].view(1, n), sc0[o0:o0 + m].view(1, m),
                    sc1[o1:o1 + n].view(1, n), rows[r + j * m: r + (j + 1) * m].view(1, 1, m, d),
                    rows[r + cnt * m + j * n: r + cnt * m + (j + 1) * n].view(1, 1, n, d),
                    scores[os_:os_ + (m + 1) * (n + 1)].view(1, m + 1, n + 1))
                o0, o1, os_ = o0 + m, o1 + n, os_ + (m + 1) * (n + 1)
            r += cnt * (m + n)
        return outs

    # -- adaptive depth / width (lightglue.py:500-521,555-580) -----------------------------------
    def _forward_adaptive(self, data):
        """Early stopping (`depth_confidence`) and point pruning (`width_confidence`); batch size 1 like the
        reference (`assert b == 1`, lightglue.py:501,507).  The host drives `gfc_lg_layer` layer by layer, takes
        the stop / prune decisions on the token confidences and matchabilities computed by `gfc_lg_rowdot`
        (one small device->host read per layer, as `check_if_stop` does in the reference) and re-packs the
        surviving rows between layers (index_select: plumbing)."""
        conf = self.conf
        b, m, _ = data["keypoints0"].shape
        n = data["keypoints1"].shape[1]
        assert b == 1
        device = data["keypoints0"].device
        params = self.ensure_packed(device)[0]
        d = conf.descriptor_dim
        do_early_stop, do_prune = conf.depth_confidence > 0, conf.width_confidence > 0
        # packed rows: image 0 first
        views = [self._side(data, "0", device), self._side(data, "1", device)]
        kp, x, so = self._pack_views(views)
        if conf.input_dim != d:
            xin, x = x, torch.empty((m + n, d), device=device, dtype=torch.float32)
            self._input_proj(params, xin, x, m + n)
        sizes = torch.cat([v[3] for v in views], 0).contiguous()
        row0 = torch.tensor([0, m], dtype=torch.int32, device=device)
        cnt = torch.tensor([m, n], dtype=torch.int32, device=device)
        cos = torch.empty((m + n, 64), device=device)
        sin = torch.empty((m + n, 64), device=device)
        nat.call("gfc_lg_posenc", kp, so, sizes, row0, cnt, 2, max(m, n), params.posenc_wr, 4 if so is not None else 2,
                 cos, sin)
        ind0 = torch.arange(m, device=device)
        ind1 = torch.arange(n, device=device)
        prune0 = torch.ones((1, m), device=device, dtype=torch.long)
        prune1 = torch.ones((1, n), device=device, dtype=torch.long)
        thresholds = self._host_thresholds()
        cm, cn = m, n
        last = conf.n_layers - 1
        for i in range(conf.n_layers):
            self_p = torch.tensor([[0, cm, 0, cm], [cm, cn, cm, cn]], dtype=torch.int32, device=device)
            cross_p = torch.tensor([[0, cm, cm, cn], [cm, cn, 0, cm]], dtype=torch.int32, device=device)
            ws = self._ws.get(nat.call("gfc_lg_layer_workspace_bytes", cm + cn), device)
            nat.call("gfc_lg_layer", ctypes.byref(params), i, x, cos, sin, cm + cn, self_p, cross_p, 2, max(cm, cn), ws,
                     ws.numel())
            last = i
            if i == conf.n_layers - 1:
                break
            tok = None
            if do_early_stop:
                tok = torch.empty((cm + cn,), device=device)
                nat.call("gfc_lg_rowdot", x, d, cm + cn, params.token_w[i], params.token_b[i], 1, tok)
                # check_if_stop (lightglue.py:569-580): the ratio is taken over the ORIGINAL m + n points
                ratio = 1.0 - (tok < thresholds[i]).float().sum() / (m + n)
                if ratio.item() > conf.depth_confidence:
                    break
            if do_prune:
                sc = torch.empty((cm + cn,), device=device)
                nat.call("gfc_lg_rowdot", x, d, cm + cn, params.matchability_w[i], params.matchability_b[i], 1, sc)
                keep = sc > (1 - conf.width_confidence)  # get_pruning_mask, lightglue.py:560-567
                if tok is not None:
                    keep = keep | (tok <= thresholds[i])
                keep0 = torch.where(keep[:cm])[0]
                keep1 = torch.where(keep[cm:])[0]
                ind0, ind1 = ind0[keep0], ind1[keep1]
                rows = torch.cat([keep0, keep1 + cm])
                x, cos, sin = x[rows].contiguous(), cos[rows].contiguous(), sin[rows].contiguous()
                prune0[:, ind0] += 1
                prune1[:, ind1] += 1
                cm, cn = int(keep0.numel()), int(keep1.numel())
                if cm == 0 or cn == 0:
                    break
        if not do_prune:
            ind0 = ind1 = prune0 = prune1 = None  # every point ran through all n_layers
        return self._finish_adaptive(params, last, x, cm, cn, m, n, ind0, ind1, prune0, prune1)

    def _finish_adaptive(self, params, layer, x, cm, cn, m, n, ind0, ind1, prune0, prune1):
        """The end of both adaptive paths for one pair of m and n points: the assignment head of `layer` on its surviving
        rows x [cm + cn, 256] (side 0 first), matches and scores scattered back through ind0 / ind1 (the survivors'
        un-pruned indices, int64; None when nothing is pruned), and the result dict with prune0/1 [1,m] / [1,n] (None:
        every point ran through all layers).  ref_descriptors0/1 are views of x."""
        conf, device = self.conf, x.device
        m0 = torch.full((1, m), -1, device=device, dtype=torch.long)
        m1 = torch.full((1, n), -1, device=device, dtype=torch.long)
        ms0 = torch.zeros((1, m), device=device)
        ms1 = torch.zeros((1, n), device=device)
        scores = torch.zeros((1, cm + 1, cn + 1), device=device)
        if cm > 0 and cn > 0:
            pm0 = torch.empty((1, cm), device=device, dtype=torch.long)
            pm1 = torch.empty((1, cn), device=device, dtype=torch.long)
            ps0, ps1 = torch.empty((1, cm), device=device), torch.empty((1, cn), device=device)
            ws = self._ws.get(nat.call("gfc_lg_assign_workspace_bytes", 1, cm, cn), device)
            nat.call("gfc_lg_assign", ctypes.byref(params), layer, x, x[cm:], 1, cm, cn, float(conf.filter_threshold),
                     pm0, pm1, ps0, ps1, scores, ws, ws.numel())
            if ind0 is not None:  # scatter back to the un-pruned indexing (lightglue.py:527-536)
                m0[:, ind0] = torch.where(pm0 == -1, -1, ind1[pm0.clamp(min=0)])
                m1[:, ind1] = torch.where(pm1 == -1, -1, ind0[pm1.clamp(min=0)])
                ms0[:, ind0], ms1[:, ind1] = ps0, ps1
            else:
                m0, m1, ms0, ms1 = pm0, pm1, ps0, ps1
        out = self._result(m0, m1, ms0, ms1, x[None, None, :cm], x[None, None, cm:], scores, prune0, prune1)
        out["stop_layer"] = torch.full((1,), layer + 1, device=device, dtype=torch.long)
        return out

    # -- adaptive depth / width over SEVERAL pairs in one pass (conf.adaptive_pair_batch) -----------------
    def _forward_adaptive_pairs(self, items):
        """`[self(d) for d in items]` for adaptive batch-1 items with key points in both views (at most
        GFC_LG_MAX_RAGGED_PAIRS of them), as one pass: every layer runs once over the live rows of all pairs, and what
        `_forward_adaptive` does between two layers on the host -- token confidences, matchabilities, the stop ratio,
        the keep masks, the re-pack -- is one call of gfc_lg_adaptive_step for all pairs, on the device, between two
        sets of row buffers.  The host reads the step's report (4 ints per pair, through a pinned buffer) once per
        layer; it tells which pairs finished and where every pair's rows went.  A pair that finishes at a layer gets that
        layer's assignment head on its rows, which the step has put behind the live region; both paths end a pair in
        `_finish_adaptive`."""
        conf = self.conf
        device = items[0]["keypoints0"].device
        nat.require_cuda(items[0]["keypoints0"], "data['keypoints0']")
        params = self.ensure_packed(device)[0]
        d, din, nb = conf.descriptor_dim, conf.input_dim, len(items)
        assert 0 < nb <= nat.GFC_LG_MAX_RAGGED_PAIRS
        do_stop, do_prune = conf.depth_confidence > 0, conf.width_confidence > 0
        ms = [int(it["keypoints0"].shape[1]) for it in items]
        ns = [int(it["keypoints1"].shape[1]) for it in items]
        total = sum(ms) + sum(ns)
        # packed rows, pair after pair: side 0 then side 1 (what gfc_lg_assign(B = 1) reads as x0, x1)
        views = [self._side(it, side, device) for it in items for side in ("0", "1")]
        kp, xa, so = self._pack_views(views)
        sizes = torch.cat([v[3] for v in views], 0).contiguous()
        if din != d:
            xin, xa = xa, torch.empty((total, d), device=device)
            self._input_proj(params, xin, xa, total)
        xb = torch.empty((total, d), device=device)
        # host tables of the first layer, one upload: segments, pairs, prune offsets, problems, un-pruned indices
        seg, pairs, self_p, cross_p, ind_parts = [], [], [], [], []
        r = 0
        for j, (m, n) in enumerate(zip(ms, ns)):
            seg += [r, m, r + m, n]
            pairs += [m + n, j]
            self_p += [r, m, r, m, r + m, n, r + m, n]
            cross_p += [r, m, r + m, n, r + m, n, r, m]
            ind_parts += [torch.arange(m, dtype=torch.int32), torch.arange(n, dtype=torch.int32)]
            r += m + n
        # two sets of tables (the step writes the next layer's): rows seg [4 nb] | pairs [2 nb] | self | cross [8 nb]
        host = torch.zeros((4, 8 * nb), dtype=torch.int32)
        for k, t in enumerate((seg, pairs, self_p, cross_p)):
            host[k, :len(t)] = torch.tensor(t, dtype=torch.int32)
        tabs = torch.empty((2, 4, 8 * nb), dtype=torch.int32, device=device)
        tabs[0].copy_(host)

        def tables(k):
            return tabs[k, 0, :4 * nb], tabs[k, 1, :2 * nb], tabs[k, 2], tabs[k, 3]

        # the segment table of layer 0 = where each image's rows start = its offsets in the prune counters
        img = tabs[0, 0, :4 * nb].view(2 * nb, 2)
        prune_off = img[:, 0].clone()
        row0, cnt = prune_off, img[:, 1].contiguous()
        inda = torch.cat(ind_parts).to(device)
        indb = torch.empty_like(inda)
        cosa, sina = torch.empty((total, 64), device=device), torch.empty((total, 64), device=device)
        cosb, sinb = torch.empty_like(cosa), torch.empty_like(sina)
        nat.call("gfc_lg_posenc", kp, so, sizes, row0, cnt, 2 * nb, max(ms + ns), params.posenc_wr,
                 4 if so is not None else 2, cosa, sina)
        prune = torch.ones((total,), dtype=torch.int32, device=device) if do_prune else None
        report = torch.empty((nb, 4), dtype=torch.int32, device=device)
        if self._report_host is None:
            self._report_host = torch.empty((nat.GFC_LG_MAX_RAGGED_PAIRS, 4), dtype=torch.int32).pin_memory()
        report_host = self._report_host
        thresholds = self._host_thresholds()
        keep_thr = float(1 - conf.width_confidence)
        step_ws_bytes = nat.call("gfc_lg_adaptive_step_workspace_bytes", nb, total)
        bufs = [(xa, cosa, sina, inda), (xb, cosb, sinb, indb)]
        cur = 0
        # live pairs in buffer order: (slot, first row, rows of side 0, rows of side 1)
        live, r = [], 0
        for j, (m, n) in enumerate(zip(ms, ns)):
            live.append((j, r, m, n))
            r += m + n
        outs = [None] * nb
        stream = torch.cuda.current_stream(device)

        def finish(slot, layer, x, ind, r0, cm, cn):
            """Pair `slot` ends at `layer` with rows [r0, r0 + cm + cn) of x."""
            m, n = ms[slot], ns[slot]
            rows = x[r0:r0 + cm + cn].clone()  # ref_descriptors0/1: the row buffers go on being re-used
            ind0 = ind1 = prune0 = prune1 = None  # without pruning every point ran through all n_layers
            if do_prune:
                ind0, ind1 = ind[r0:r0 + cm].long(), ind[r0 + cm:r0 + cm + cn].long()
                o = sum(ms[:slot]) + sum(ns[:slot])
                prune0, prune1 = prune[o:o + m].long()[None], prune[o + m:o + m + n].long()[None]
            outs[slot] = self._finish_adaptive(params, layer, rows, cm, cn, m, n, ind0, ind1, prune0, prune1)

        for i in range(conf.n_layers):
            x, cos, sin, ind = bufs[cur]
            _, _, self_t, cross_t = tables(cur)
            rows = sum(cm + cn for _, _, cm, cn in live)
            max_n = max(max(cm, cn) for _, _, cm, cn in live)
            ws = self._ws.get(max(nat.call("gfc_lg_layer_workspace_bytes", rows), step_ws_bytes), device)
            nat.call("gfc_lg_layer", ctypes.byref(params), i, x, cos, sin, rows, self_t, cross_t, 2 * len(live), max_n,
                     ws, ws.numel())
            if i == conf.n_layers - 1:
                break
            seg_t, pairs_t, _, _ = tables(cur)
            seg_o, pairs_o, self_o, cross_o = tables(1 - cur)
            xo, coso, sino, indo = bufs[1 - cur]
            nat.call("gfc_lg_adaptive_step", ctypes.byref(params), i, x, cos, sin, ind, rows, seg_t, pairs_t, prune_off,
                     nb, len(live), max_n, thresholds[i], keep_thr, float(conf.depth_confidence), int(do_stop),
                     int(do_prune), xo, coso, sino, indo, prune, total, self_o, cross_o, seg_o, pairs_o, report, ws,
                     ws.numel())
            report_host[:len(live)].copy_(report[:len(live)], non_blocking=True)
            stream.synchronize()  # the one device->host read of the layer
            rep = report_host[:len(live)].tolist()
            # the step's output order: the pairs that go on, then the pairs that finished, each group in input order
            order = [k for k, q in enumerate(rep) if q[0] == nat.GFC_LG_ADAPTIVE_LIVE]
            n_live = len(order)
            order += [k for k, q in enumerate(rep) if q[0] != nat.GFC_LG_ADAPTIVE_LIVE]
            nxt, r = [], 0
            for pos, k in enumerate(order):
                _, cm, cn, _ = rep[k]
                if pos < n_live:
                    nxt.append((live[k][0], r, cm, cn))
                else:
                    finish(live[k][0], i, xo, indo, r, cm, cn)
                r += cm + cn
            live, cur = nxt, 1 - cur
            if not live:
                break
        x, _, _, ind = bufs[cur]
        for slot, r0, cm, cn in live:  # went through every layer: the last layer's head
            finish(slot, conf.n_layers - 1, x, ind, r0, cm, cn)
        return outs


__main_model__ = LightGlue
