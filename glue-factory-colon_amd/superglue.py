"""SuperGlue matcher on MI355X -- drop-in for `gluefactory_nonfree.superglue` (inference path, reference
gluefactory_nonfree/superglue.py:223-322): the attentional graph neural network and the Sinkhorn optimal transport.

Same `default_conf` keys, `required_data_keys`, prediction keys and state-dict key names as the reference class, so
`superglue_outdoor.pth` / `superglue_indoor.pth` load unchanged.  The torch sub-modules are parameter containers only;
the forward pass is one call into libgfc_amd.so (gfc_sg_forward: key-point encoder, 18 x [projection, attention,
merge, MLP], final projection, similarity, Sinkhorn, mutual-argmax filter).

    model.matcher.name = gluefactory_nonfree.superglue

`weights` is an existing checkpoint path or "synthetic[:seed]" (name-seeded, weights.superglue_state_dict); nothing is
ever downloaded, so the reference's "indoor" / "outdoor" raise FileNotFoundError.  Training (`loss`) is out of scope.
"""
import ctypes
import itertools
from pathlib import Path

import torch
from torch import nn

from . import _native as nat
from . import weights as _weights
from .base_model import BaseModel, conf_get

_D, _HEADS = 256, 4
_ENCODER = [32, 64, 128, 256]


def _mlp(channels):
    """Conv1d(k=1) -> BatchNorm1d -> ReLU per layer, the last layer bare: indices 0,1,2, 3,4,5, ... as in the checkpoints."""
    layers = []
    for i, (cin, cout) in enumerate(zip(channels[:-1], channels[1:])):
        layers.append(nn.Conv1d(cin, cout, kernel_size=1, bias=True))
        if i < len(channels) - 2:
            layers += [nn.BatchNorm1d(cout), nn.ReLU()]
    return nn.Sequential(*layers)


class _KeypointEncoder(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.encoder = _mlp([cin, *_ENCODER, _D])


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.merge = nn.Conv1d(_D, _D, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(_D, _D, kernel_size=1) for _ in range(3)])


class _Propagation(nn.Module):
    def __init__(self):
        super().__init__()
        self.attn = _Attention()
        self.mlp = _mlp([2 * _D, 2 * _D, _D])


class _GNN(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.layers = nn.ModuleList([_Propagation() for _ in range(n)])


def fold_bn1d(bn):
    """Eval-mode BatchNorm1d as y * scale + shift, folded in float64."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return scale.float(), shift.float()


def head_major_index():
    """The reference splits heads with view(b, dim, h, -1) (superglue.py:133): channel c is head c % 4, position c // 4.
    Packed channel h * 64 + d reads state-dict channel d * 4 + h."""
    idx = torch.arange(_D)
    return (idx % (_D // _HEADS)) * _HEADS + idx // (_D // _HEADS)


class SuperGlue(BaseModel):
    default_conf = {
        "descriptor_dim": 256,
        "weights": "outdoor",
        "keypoint_encoder": [32, 64, 128, 256],
        "GNN_layers": ["self", "cross"] * 9,
        "num_sinkhorn_iterations": 50,
        "filter_threshold": 0.2,
        "use_scores": True,
        "loss": {"nll_balancing": 0.5},
    }
    required_data_keys = ["view0", "view1", "keypoints0", "keypoints1", "descriptors0", "descriptors1",
                          "keypoint_scores0", "keypoint_scores1"]

    def _init(self, conf):
        if conf.descriptor_dim != _D or list(conf.keypoint_encoder) != _ENCODER:
            raise NotImplementedError("the MI355X kernels are built for descriptor_dim 256 and the key-point encoder "
                                      "[32, 64, 128, 256]")
        names = list(conf.GNN_layers)
        if len(names) > nat.GFC_SG_MAX_LAYERS or any(n not in ("self", "cross") for n in names):
            raise NotImplementedError(f"GNN_layers: at most {nat.GFC_SG_MAX_LAYERS} entries of 'self' / 'cross'")
        self.kenc = _KeypointEncoder(3 if conf.use_scores else 2)
        self.gnn = _GNN(len(names))
        self.final_proj = nn.Conv1d(_D, _D, kernel_size=1, bias=True)
        self.register_parameter("bin_score", nn.Parameter(torch.tensor(1.0)))
        self._packed = None
        self._ws = nat.Workspace()
        w = conf_get(conf, "weights")
        if w:
            if Path(str(w)).exists():
                self.load_state_dict(torch.load(str(w), map_location="cpu"))
            elif isinstance(w, str) and w.startswith("synthetic"):
                seed = int(w.split(":")[1]) if ":" in w else 0
                self.load_state_dict(_weights.superglue_state_dict(seed, n_layers=len(names),
                                                                   use_scores=bool(conf.use_scores)))
            else:
                # the reference downloads superglue_{indoor,outdoor}.pth here (superglue.py:262-266); no network
                raise FileNotFoundError(f"weights {w!r} not found (no download is attempted)")

    # -- weights ------------------------------------------------------------------------
    def load_state_dict(self, *args, **kwargs):
        ret = super().load_state_dict(*args, **kwargs)
        self._packed = None
        return ret

    def _apply(self, fn, *args, **kwargs):
        self._packed = None
        return super()._apply(fn, *args, **kwargs)

    def __deepcopy__(self, memo):
        """Replicas (export_predictions workers) get their own parameters and workspace; the packed device pointers
        belong to the original and are rebuilt by the copy on first use."""
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k == "_packed" else copy.deepcopy(v, memo)
        return new

    def _pack(self, device):
        keep = []

        def dev(t):
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        conf = self.conf
        p = nat.SgParams()
        names = list(conf.GNN_layers)
        p.n_layers, p.use_scores = len(names), int(bool(conf.use_scores))
        enc = self.kenc.encoder
        for i in range(5):
            conv = enc[3 * i]
            w = conv.weight.detach()[:, :, 0]
            p.kenc_w[i] = dev(w if i == 4 else w.t())  # layers 0..3 transposed to [cin][cout]
            p.kenc_b[i] = dev(conv.bias)
            if i < 4:
                scale, shift = fold_bn1d(enc[3 * i + 1])
                p.kenc_scale[i], p.kenc_shift[i] = dev(scale), dev(shift)
        src = head_major_index()
        for i, (layer, name) in enumerate(zip(self.gnn.layers, names)):
            p.cross[i] = int(name == "cross")
            proj = layer.attn.proj
            p.wqkv[i] = dev(torch.cat([c.weight.detach()[:, :, 0][src] for c in proj], 0))
            p.bqkv[i] = dev(torch.cat([c.bias.detach()[src] for c in proj], 0))
            p.merge_w[i] = dev(layer.attn.merge.weight.detach()[:, :, 0][:, src])
            p.merge_b[i] = dev(layer.attn.merge.bias)
            p.mlp0_w[i] = dev(layer.mlp[0].weight.detach()[:, :, 0])
            p.mlp0_b[i] = dev(layer.mlp[0].bias)
            scale, shift = fold_bn1d(layer.mlp[1])
            p.mlp_scale[i], p.mlp_shift[i] = dev(scale), dev(shift)
            p.mlp1_w[i] = dev(layer.mlp[3].weight.detach()[:, :, 0])
            p.mlp1_b[i] = dev(layer.mlp[3].bias)
        p.final_proj_w = dev(self.final_proj.weight.detach()[:, :, 0])
        p.final_proj_b = dev(self.final_proj.bias)
        p.bin_score = float(self.bin_score.detach())
        return p, keep, device

    def ensure_packed(self, device):
        if self._packed is None or self._packed[2] != device:
            self._packed = self._pack(device)
        return self._packed

    # -- forward ------------------------------------------------------------------------
    @staticmethod
    def _size(data, side, b, device):
        """`image_size` of the view, or (w, h) of its image (superglue.py:281-286, normalize_keypoints :85-90)."""
        view = data["view" + side]
        size = view.get("image_size")
        if size is None:
            h, w = view["image"].shape[-2:]
            size = torch.tensor([[float(w), float(h)]])
        return torch.as_tensor(size, device=device, dtype=torch.float32).reshape(-1, 2).expand(b, 2).contiguous()

    def _inputs(self, data):
        kp0, kp1 = data["keypoints0"], data["keypoints1"]
        nat.require_cuda(kp0, "data['keypoints0']")
        device, b = kp0.device, kp0.shape[0]

        def f(t):
            return t.to(device=device, dtype=torch.float32).contiguous()

        sc0 = sc1 = None
        if self.conf.use_scores:
            sc0, sc1 = f(data["keypoint_scores0"]), f(data["keypoint_scores1"])
        return (f(kp0), f(kp1), sc0, sc1, f(data["descriptors0"]), f(data["descriptors1"]),
                self._size(data, "0", b, device), self._size(data, "1", b, device))

    def _run(self, kp0, kp1, sc0, sc1, d0, d1, s0, s1, taps=False):
        """The batched core: B pairs of (m, n) key points through gfc_sg_forward.  taps: also return `desc_taps`
        [4, B*m + B*n, 256], the packed rows after the encoder, layer 0, layer 1 and the last layer."""
        conf = self.conf
        device = kp0.device
        b, m = kp0.shape[:2]
        n = kp1.shape[1]
        assert d0.shape[-1] == _D and d1.shape[-1] == _D
        p = self.ensure_packed(device)[0]
        m0 = torch.empty((b, m), device=device, dtype=torch.long)
        m1 = torch.empty((b, n), device=device, dtype=torch.long)
        ms0, ms1 = torch.empty((b, m), device=device), torch.empty((b, n), device=device)
        cost = torch.empty((b, m, n), device=device)
        la = torch.empty((b, m + 1, n + 1), device=device)
        tap = torch.zeros((4, b * (m + n), _D), device=device) if taps else None
        need = nat.call("gfc_sg_workspace_bytes", b, m, n)
        if need == 0:
            raise nat.NativeError(f"gfc_sg_forward cannot run a batch of {b} x ({m}, {n}) key points")
        ws = self._ws.get(need, device)
        nat.call("gfc_sg_forward", ctypes.byref(p), kp0, kp1, sc0, sc1, d0, d1, s0, s1, b, m, n,
                 int(conf.num_sinkhorn_iterations), float(conf.filter_threshold), cost, la, m0, m1, ms0, ms1, tap, ws,
                 ws.numel())
        out = {"sinkhorn_cost": cost, "log_assignment": la, "matches0": m0, "matches1": m1, "matching_scores0": ms0,
               "matching_scores1": ms1}
        if taps:
            out["desc_taps"] = tap
        return out

    def _forward(self, data):
        if self.training:
            raise NotImplementedError("training is out of scope: inference path only")
        kp0, kp1 = data["keypoints0"], data["keypoints1"]
        if kp0.shape[1] == 0 or kp1.shape[1] == 0:  # no key points (superglue.py:272-279)
            shape0, shape1 = kp0.shape[:-1], kp1.shape[:-1]
            return {"matches0": kp0.new_full(shape0, -1, dtype=torch.int),
                    "matches1": kp1.new_full(shape1, -1, dtype=torch.int),
                    "matching_scores0": kp0.new_zeros(shape0), "matching_scores1": kp1.new_zeros(shape1)}
        return self._run(*self._inputs(data))

    def forward_pairs(self, datas: list) -> list:
        """MI355X addition: `[self(d) for d in datas]` for batch-1 pairs, the pairs of equal (m, n) stacked into one
        batch each and sent through the batched core once per group.  Per-pair dictionaries with the keys of the
        single-pair call, in the order given; pairs with an empty side or a batch size other than 1 take `self(d)`.
        Against the single-pair calls: matches identical outside near-ties, floats within 1e-4 -- not bit for bit, since
        the attention's key split and the GEMM tile follow the size of the launch (Sinkhorn alone is bit-identical)."""
        outs = [None] * len(datas)
        shapes = {}
        for i, d in enumerate(datas):
            k0, k1 = d["keypoints0"], d["keypoints1"]
            if k0.shape[0] != 1 or k0.shape[1] == 0 or k1.shape[1] == 0:
                outs[i] = self(d)
            else:
                for key in self.required_data_keys:
                    assert key in d, f"Missing key {key} in data"
                shapes[i] = (int(k0.shape[1]), int(k1.shape[1]))
        order = sorted(shapes, key=lambda i: shapes[i])
        for _, idx in itertools.groupby(order, key=lambda i: shapes[i]):
            idx = list(idx)
            ins = [self._inputs(datas[i]) for i in idx]
            stacked = [None if col[0] is None else torch.cat(col, 0) for col in zip(*ins)]
            out = self._run(*stacked)
            for j, i in enumerate(idx):
                outs[i] = {k: v[j:j + 1] for k, v in out.items()}
        return outs

    def loss(self, pred, data):
        raise NotImplementedError("training is out of scope")


__main_model__ = SuperGlue
