"""gfc_lg_head_backward / gfc_lg_token_backward alone, then `LightGlue.layer_loss_backward`, `heads_updated` and
`finetune_heads` on the GPU.

The kernels are compared with the float64 closed form of tests/head_grad_reference.py evaluated on the SAME bits, per
element within c 2^-23 abs-sum (c and the abs-sums are derived there, from the shape alone).  The module is compared
with the reference's own autograd (tests/golden/head_grad_*.npz) within (c + trunk_c) 2^-23 abs-sum, the abs-sums
evaluated by the closed form on the device's own descriptors, and with the closed form on those descriptors within
c 2^-23 abs-sum.

Shapes.  The GEMM tiles are 128 x 128 with k stepped by 16, dmd^T x is split into parts of at most 1024 rows, the column
sums into chunks of 128 rows, the log-sum-exp walks 4 rows / 32 columns per workgroup: every edge +-1 below, the four
shapes of the issue, 3 x 65535 x 1 (the largest M, where the 128-part limit of the split acts) and 2 x 1024 x 1024 as
the scale case.  Not covered: a score array past 2^31 elements (12.9 GB at 2 x 40000 x 40000, beyond a float64
reference on the host); its indices are 64-bit by construction.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endopatches_reference as er  # noqa: E402
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402
import layer_loss_reference as lr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GAMMAS = {"05": 0.5, "0": 0.0, "1": 1.0}
EPS = 0.05  # the step of the descent check (tests/test_head_grad_reference_host.py stores and derives it)
DEV = "cuda"
WORST = {}  # output -> the largest fraction of its bound any test used (printed by the last test of the file)


def model(**conf):
    return lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.0, **conf}).eval().cuda()


_SHARED = {}


def shared_model():
    if "lg" not in _SHARED:
        _SHARED["lg"] = model()
        _SHARED["params"] = _SHARED["lg"].ensure_packed(torch.device(DEV, 0))[0]
    return _SHARED["lg"], _SHARED["params"]


def rows(b, k, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, k, 256), generator=g)
    return (scale * x / x.norm(dim=-1, keepdim=True)).contiguous()


def make_labels(b, m, n, seed, mode="mixed"):
    """gt_matches0 [B,M], gt_matches1 [B,N] (int64), gt_assignment [B,M,N] bool or None."""
    g = torch.Generator().manual_seed(seed)
    gt0 = torch.full((b, m), -1, dtype=torch.long)
    gt1 = torch.full((b, n), -1, dtype=torch.long)
    for q in range(b):
        k = min(m, n) // 2
        i, j = torch.randperm(m, generator=g)[:k], torch.randperm(n, generator=g)[:k]
        gt0[q, i], gt1[q, j] = j, i
        gt0[q, torch.randperm(m, generator=g)[:m // 5]] = -2
        gt1[q, torch.randperm(n, generator=g)[:n // 5]] = -2
    gta = None
    if mode == "no_positive_pair":   # pair 0 has no positive: P is clamped
        gt0[0], gt1[0] = gt0[0].clamp(max=-1), gt1[0].clamp(max=-1)
    elif mode == "no_negative_side":  # no -1 on side 0: that clamp of Q acts alone
        gt0[gt0 == -1] = -2
    elif mode == "ignored":           # every label -2: exact zeros
        gt0[:], gt1[:] = -2, -2
    elif mode in ("assignment", "multi"):
        gta = torch.zeros((b, m, n), dtype=torch.bool)
        bi, ii = torch.nonzero(gt0 > -1, as_tuple=True)
        gta[bi, ii, gt0[bi, ii]] = True
        if mode == "multi":  # a row with three positives and a column with two
            gta[0, 1, :3] = True
            gta[0, 2:4, n - 1] = True
    return gt0, gt1, gta


def run_head(params, layer, x0, x1, gt0, gt1, gta, g, lam, want_dx=True, ws_bytes=None):
    b, m, _ = x0.shape
    n = x1.shape[1]
    c = lambda t: None if t is None else t.to(DEV).contiguous()
    out = {"dWf": torch.full((256, 256), float("nan"), device=DEV), "dbf": torch.full((256,), float("nan"), device=DEV),
           "dwm": torch.full((256,), float("nan"), device=DEV), "dbm": torch.full((1,), float("nan"), device=DEV),
           "dx": torch.full((b * (m + n), 256), float("nan"), device=DEV) if want_dx else None}
    need = nat.call("gfc_lg_head_backward_workspace_bytes", b, m, n)
    ws = torch.full((need if ws_bytes is None else ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)  # NaNs on entry
    nat.call("gfc_lg_head_backward", ctypes.byref(params), layer, c(x0.reshape(-1, 256)), c(x1.reshape(-1, 256)), c(gt0),
             c(gt1), c(gta), c(g), lam, b, m, n, out["dWf"], out["dbf"], out["dwm"], out["dbm"], out["dx"], ws, ws.numel())
    torch.cuda.synchronize()
    return out


def check_head(tag, layer, x0, x1, gt0, gt1, gta, g, lam=0.5, env=None):
    """env: (packed parameters, their state dict); default: the name-seeded weights."""
    if env is None:
        lg, params = shared_model()
        sd = {k: v.detach().cpu() for k, v in lg.state_dict().items()}
    else:
        params, sd = env
    got = run_head(params, layer, x0, x1, gt0, gt1, gta, g, lam)
    again = run_head(params, layer, x0, x1, gt0, gt1, gta, g, lam)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{tag}: {k} differs between two calls"
    b, m, n = x0.shape[0], x0.shape[1], x1.shape[1]
    want, sums = hg.head_grad(x0.double(), x1.double(), *hg.head_params(sd, layer), gt0, gt1, gta, g.double(), lam)
    want["dx"] = torch.cat([want["dx0"].reshape(-1, 256), want["dx1"].reshape(-1, 256)], 0)
    sums["dx"] = torch.cat([sums["dx0"].reshape(-1, 256), sums["dx1"].reshape(-1, 256)], 0)
    c = hg.head_c(b, m, n)
    report = []
    for k in ("dWf", "dbf", "dwm", "dbm", "dx"):
        v = got[k].double().cpu().reshape(want[k].shape)
        assert bool(torch.isfinite(v).all()), f"{tag}: {k} is not finite"
        bound = c[k] * hg.U * sums[k]
        frac = float(((v - want[k]).abs() / bound.clamp(min=1e-300)).max())
        exact_zero = bool(((sums[k] != 0) | (v == 0)).all())  # nothing added in: an exact zero
        WORST[k] = max(WORST.get(k, 0.0), frac)
        report.append(f"{k} {frac:.3f}")
        assert frac <= 1.0 and exact_zero, (tag, k, frac)
    print(f"{tag}: fraction of the bound used: " + ", ".join(report))
    return got, want


SHAPES = [(1, 1, 65), (1, 65, 1), (3, 257, 300), (2, 130, 65),            # the issue's
          (1, 127, 129), (1, 128, 128), (1, 129, 127),                    # the 128 x 128 output tile
          (1, 15, 17), (1, 16, 16), (1, 17, 15),                          # the k step of 16 (k = N and k = M)
          (1, 1023, 31), (1, 1024, 32), (1, 1025, 33),                    # the 1024-row split of dmd^T x, 32 columns
          (2, 63, 1), (2, 64, 3), (3, 43, 5),                             # 127, 128 + 6, 129 + 15 rows: the 128-row chunks
          (3, 65535, 1)]                                                  # the largest M; 192 parts of 1024 rows -> 128


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_head_backward_shapes(shape):
    b, m, n = shape
    x0, x1 = rows(b, m, 1, 3.0), rows(b, n, 2, 3.0)
    gt0, gt1, gta = make_labels(b, m, n, 3, "assignment" if m % 2 else "mixed")
    g = torch.tensor([0.7, 0.0, -0.4][:b]) if b == 3 else torch.full((b,), 1.0 / b)
    check_head("x".join(map(str, shape)), 3, x0, x1, gt0, gt1, gta, g)


def test_head_backward_scale():
    b, m, n = 2, 1024, 1024
    gt0, gt1, gta = make_labels(b, m, n, 5)
    check_head("2x1024x1024", 6, rows(b, m, 3, 3.0), rows(b, n, 4, 3.0), gt0, gt1, gta, torch.tensor([0.5, 0.5]), lam=0.3)


@pytest.mark.parametrize("mode", ["no_positive_pair", "no_negative_side", "multi"])
def test_head_backward_label_cases(mode):
    b, m, n = 3, 70, 45
    gt0, gt1, gta = make_labels(b, m, n, 7, mode)
    check_head(mode, 2, rows(b, m, 5, 3.0), rows(b, n, 6, 3.0), gt0, gt1, gta, torch.tensor([0.6, 0.0, -0.3]))


def test_head_backward_ignored_labels_give_exact_zeros():
    b, m, n = 2, 70, 45
    gt0, gt1, gta = make_labels(b, m, n, 7, "ignored")
    got, _ = check_head("ignored", 2, rows(b, m, 5, 3.0), rows(b, n, 6, 3.0), gt0, gt1, gta, torch.tensor([0.6, 0.4]))
    for k, v in got.items():
        assert bool((v == 0).all()), k


def crafted():
    """A module whose head 0 gives |S| up to about 80 on rows of norm 3 and whose heads 1 / 2 give z = +1e4 / -1e4."""
    if "crafted" not in _SHARED:
        lg = model()
        sd = {k: v.detach().cpu().clone() for k, v in lg.state_dict().items()}
        x0, x1 = rows(2, 70, 5, 3.0).double(), rows(2, 45, 6, 3.0).double()
        wf, bf, _, _ = hg.head_params(sd, 0)
        s = 0.25 * (x0 @ wf.t() + bf) @ (0.25 * (x1 @ wf.t() + bf)).transpose(1, 2)
        sd["log_assignment.0.final_proj.weight"] *= float((80.0 / s.abs().max()).sqrt())
        sd["log_assignment.0.final_proj.bias"] *= float((80.0 / s.abs().max()).sqrt())
        for layer, z in ((1, 1e4), (2, -1e4)):
            sd[f"log_assignment.{layer}.matchability.weight"].zero_()
            sd[f"log_assignment.{layer}.matchability.bias"].fill_(z)
        lg.load_state_dict(sd)
        _SHARED["crafted"] = (lg, lg.ensure_packed(torch.device(DEV, 0))[0], sd)
    return _SHARED["crafted"]


def test_head_backward_large_scores_and_saturated_sigmoids():
    lg, params, sd = crafted()
    b, m, n = 2, 70, 45
    x0, x1 = rows(b, m, 5, 3.0), rows(b, n, 6, 3.0)
    gt0, gt1, gta = make_labels(b, m, n, 7, "multi")
    wf, bf, _, _ = hg.head_params(sd, 0)
    s = 0.25 * (x0.double() @ wf.t() + bf) @ (0.25 * (x1.double() @ wf.t() + bf)).transpose(1, 2)
    print(f"largest |S| {float(s.abs().max()):.1f}")
    assert 60 <= float(s.abs().max()) <= 100
    check_head("|S| ~ 80", 0, x0, x1, gt0, gt1, gta, torch.tensor([1.0, -0.5]), env=(params, sd))
    # saturated: sigmoid(1e4) = 1 and sigmoid(-1e4) = 0 exactly, so dz = c n (z = +1e4) and dz = -a r (z = -1e4).  With
    # g = 2^-6 Q (or P) the pair's c (or a) is 2^-7 and every sum of such terms is exact in fp32: dbm is known exactly.
    w = gta.double()
    p_sum = w.sum((1, 2)).clamp(min=1)
    negatives = (gt0 == -1).sum(1) + (gt1 == -1).sum(1)
    q_sum = (gt0 == -1).sum(1).clamp(min=1) + (gt1 == -1).sum(1).clamp(min=1)
    up, _ = check_head("z = +1e4", 1, x0, x1, gt0, gt1, gta, (q_sum * 2.0 ** -6).float(), env=(params, sd))
    down, _ = check_head("z = -1e4", 2, x0, x1, gt0, gt1, gta, (p_sum * 2.0 ** -6).float(), env=(params, sd))
    assert float(up["dbm"].cpu()) == float(2.0 ** -7 * negatives.sum())
    assert float(down["dbm"].cpu()) == float(-(2.0 ** -7) * 2 * w.sum())


def test_head_backward_refusals():
    _, params = shared_model()
    x0, x1 = rows(1, 4, 1), rows(1, 5, 2)
    gt0, gt1, _ = make_labels(1, 4, 5, 1)
    g = torch.ones(1)
    need = nat.call("gfc_lg_head_backward_workspace_bytes", 1, 4, 5)
    with pytest.raises(nat.NativeError, match="GFC_ERR_WORKSPACE"):
        run_head(params, 0, x0, x1, gt0, gt1, None, g, 0.5, ws_bytes=need - 1)
    run_head(params, 0, x0, x1, gt0, gt1, None, g, 0.5, ws_bytes=need)
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
        run_head(params, 9, x0, x1, gt0, gt1, None, g, 0.5)
    lib, null = nat.lib(), None
    buf = torch.zeros(4096, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for b, m, n in ((0, 4, 5), (1, 0, 5), (1, 4, 0), (65536, 1, 1), (1, 65536, 1), (1, 1, 65536), (128, 65535, 1)):
        assert lib.gfc_lg_head_backward_workspace_bytes(b, m, n) == 0
        st = lib.gfc_lg_head_backward(ctypes.byref(params), 0, P(buf), P(buf), P(buf), P(buf), null, P(buf), 0.5, b, m, n,
                                      P(buf), P(buf), P(buf), P(buf), null, P(buf), 1 << 40, null)
        assert nat.STATUS[st] == "GFC_ERR_INVALID", (b, m, n)
        st = lib.gfc_lg_token_backward(P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), 9, b, m, n, P(buf), P(buf),
                                       P(buf), 1 << 40, null)
        assert nat.STATUS[st] == "GFC_ERR_INVALID", (b, m, n)
    half = model(matmul_precision="fp16")
    with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):  # the packed parameters of the fp16 matcher
        run_head(half.ensure_packed(torch.device(DEV, 0))[0], 0, x0, x1, gt0, gt1, None, g, 0.5)


def run_token(x0, x1, logit0, logit1, c0, c1, g, nl, ws_bytes=None):
    b, m, _ = x0.shape
    n = x1.shape[1]
    c = lambda t: t.to(DEV).contiguous()
    dw, db = torch.full((256,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    need = nat.call("gfc_lg_token_backward_workspace_bytes", b, m, n)
    ws = torch.full((need if ws_bytes is None else ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    nat.call("gfc_lg_token_backward", c(x0.reshape(-1, 256)), c(x1.reshape(-1, 256)), c(logit0), c(logit1),
             c(c0.to(torch.uint8)), c(c1.to(torch.uint8)), c(g), nl, b, m, n, dw, db, ws, ws.numel())
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("shape", [(1, 1, 65), (3, 257, 300), (2, 63, 1), (2, 64, 3), (2, 1024, 1024)],
                         ids=["1x1x65", "3x257x300", "2x63x1", "2x64x3", "2x1024x1024"])
def test_token_backward(shape):
    b, m, n = shape
    g0 = torch.Generator().manual_seed(9)
    x0, x1 = rows(b, m, 1, 3.0), rows(b, n, 2, 3.0)
    logit0, logit1 = 3 * torch.randn((b, m), generator=g0), 3 * torch.randn((b, n), generator=g0)
    logit0[0, 0], logit1[0, 0] = 1e4, -1e4  # saturated: sigmoid exactly 1 and 0
    c0, c1 = torch.rand((b, m), generator=g0) < 0.6, torch.rand((b, n), generator=g0) < 0.6
    g = torch.tensor([0.7, 0.0, -0.4][:b]) if b == 3 else torch.full((b,), 1.0 / b)
    dw, db = run_token(x0, x1, logit0, logit1, c0, c1, g, 9)
    dw2, db2 = run_token(x0, x1, logit0, logit1, c0, c1, g, 9)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    tw = torch.zeros(256, dtype=torch.float64)
    want, sums = hg.token_grad(x0.double(), x1.double(), tw, tw[0], c0, c1, g.double(), 9, logit0=logit0.double(),
                               logit1=logit1.double())
    c = hg.token_c(b, m, n)
    for k, v in (("dw", dw), ("db", db)):
        v = v.double().cpu().reshape(want[k].shape)
        assert bool(torch.isfinite(v).all())
        frac = float(((v - want[k]).abs() / (c * hg.U * sums[k])).max())
        WORST["token " + k] = max(WORST.get("token " + k, 0.0), frac)
        print(f"token {k}: fraction of the bound used {frac:.3f}")
        assert frac <= 1.0
    need = nat.call("gfc_lg_token_backward_workspace_bytes", b, m, n)
    with pytest.raises(nat.NativeError, match="GFC_ERR_WORKSPACE"):
        run_token(x0, x1, logit0, logit1, c0, c1, g, 9, ws_bytes=need - 1)


# ---- the module -------------------------------------------------------------------------------------------------------
def inputs(case):
    c = lambda k: case[k].cuda()  # noqa: E731
    return {"keypoints0": c("keypoints0"), "keypoints1": c("keypoints1"), "descriptors0": c("descriptors0"),
            "descriptors1": c("descriptors1"), "view0": {"image_size": c("size")}, "view1": {"image_size": c("size")}}


def labels(case):
    out = {"gt_matches0": case["gt_matches0"].cuda(), "gt_matches1": case["gt_matches1"].cuda()}
    if case["gt_assignment"] is not None:
        out["gt_assignment"] = case["gt_assignment"].cuda()
    return out


@pytest.fixture(scope="module", params=["a", "b"])
def fx(request):
    """A fixture batch and ONE forward_layers prediction shared by the tests (never changed)."""
    name = request.param
    z = np.load(os.path.join(GOLDEN, f"head_grad_{name}_gamma1.npz"))
    case = lc.make_case(name, int(z["seed"]))
    assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"]))
    lg = model()
    with torch.no_grad():
        pred = lg.forward_layers(inputs(case))
    torch.cuda.synchronize()
    xs0 = [pred["ref_descriptors0"][:, i].double().cpu() for i in range(lc.N_LAYERS)]
    xs1 = [pred["ref_descriptors1"][:, i].double().cpu() for i in range(lc.N_LAYERS)]
    sd = {k: v.detach().double().cpu() for k, v in lg.state_dict().items()}
    cpu_labels = {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"],
                  "gt_assignment": case["gt_assignment"]}
    return name, case, pred, xs0, xs1, sd, cpu_labels


def stored(z):
    t = lambda k: torch.from_numpy(z[k]).double()
    out = {}
    for i in range(lc.N_LAYERS):
        p = f"log_assignment.{i}."
        out[p + "final_proj.bias"], out[p + "matchability.weight"] = t("bf")[i], t("wm")[i].reshape(1, 256)
        out[p + "matchability.bias"] = t("bm")[i].reshape(1)
    for i in range(lc.N_LAYERS - 1):
        p = f"token_confidence.{i}.token.0."
        out[p + "weight"], out[p + "bias"] = t("tw")[i].reshape(1, 256), t("tb")[i].reshape(1)
    return out


@pytest.mark.parametrize("tag", list(GAMMAS))
def test_layer_loss_backward_on_the_fixture(fx, tag):
    name, case, pred, xs0, xs1, sd, cpu_labels = fx
    z = np.load(os.path.join(GOLDEN, f"head_grad_{name}_gamma{tag}.npz"))
    lg = model(loss={"gamma": GAMMAS[tag]})
    grads = lg.layer_loss_backward(pred, labels(case), descriptor_grads=True, accumulate=False)
    torch.cuda.synchronize()
    want, sums, cs = hg.model_grads(xs0, xs1, sd, cpu_labels, gamma=GAMMAS[tag], descriptor_grads=True)
    assert set(grads) == set(want)
    trunk = hg.trunk_c(lc.N_LAYERS)
    same, ref = 0.0, 0.0
    for k, w in want.items():  # the closed form on the device's own descriptors: the same bits
        v = grads[k].double().cpu()
        assert v.shape == w.shape, k
        frac = float(((v - w).abs() / (cs[k] * hg.U * sums[k])).max())
        key = "module " + k.split(".", 2)[-1]
        WORST[key] = max(WORST.get(key, 0.0), frac)
        same = max(same, frac)
    rows_, cols, u, v_ = (torch.from_numpy(z[k]) for k in ("rows", "cols", "u", "v"))
    for k, r in stored(z).items():  # the reference's autograd (float64 run)
        ref = max(ref, float(((grads[k].double().cpu() - r).abs() / ((cs[k] + trunk) * hg.U * sums[k])).max()))
    for i in range(lc.N_LAYERS):
        k = f"log_assignment.{i}.final_proj.weight"
        g, s, tol = grads[k].double().cpu(), sums[k], (cs[k] + trunk) * hg.U
        ref = max(ref, float(((g[rows_] - torch.from_numpy(z["wf_rows"][i])).abs() / (tol * s[rows_])).max()),
                  float(((g[:, cols] - torch.from_numpy(z["wf_cols"][i])).abs() / (tol * s[:, cols])).max()),
                  float((u @ g @ v_ - float(z["wf_bilinear"][i])).abs() / (tol * (u.abs() @ s @ v_.abs()))))
    if tag == "05":
        d = np.load(os.path.join(GOLDEN, f"head_grad_dx_{name}.npz"))
        for side in ("0", "1"):
            k = "grad_ref_descriptors" + side
            g = grads[k].permute(1, 0, 2, 3).reshape(lc.N_LAYERS, -1, 256).double().cpu()
            s = sums[k].permute(1, 0, 2, 3).reshape(lc.N_LAYERS, -1, 256)
            r = torch.from_numpy(d["rows" + side])
            tol = (cs[k] + trunk) * hg.U
            ref = max(ref, float(((g[:, r] - torch.from_numpy(d["dx" + side])).abs() / (tol * s[:, r])).max()))
    print(f"case {name} gamma {GAMMAS[tag]}: fraction of the bound used: {same:.3f} against the closed form on the "
          f"device's descriptors, {ref:.3f} against the reference's autograd")
    assert same <= 1.0 and ref <= 1.0
    # the token targets on the device are the reference's
    assert torch.equal(lr.token_targets(hg.head_forward(xs0[0], xs1[0], *hg.head_params(sd, 0)),
                                        hg.head_forward(xs0[-1], xs1[-1], *hg.head_params(sd, 8)))[0],
                       torch.from_numpy(z["correct0"][0]))


def test_accumulation_layout_and_refusals(fx):
    name, case, pred, _, _, _, _ = fx
    lg = model()
    once = lg.layer_loss_backward(pred, labels(case), accumulate=False)
    assert all(p.grad is None for p in lg.parameters())
    assert "grad_ref_descriptors0" not in once and len(once) == 4 * 9 + 2 * 8
    twice = lg.layer_loss_backward(pred, labels(case))
    lg.layer_loss_backward(pred, labels(case), descriptor_grads=True)
    for k, g in once.items():
        p = lg.get_parameter(k)
        assert torch.equal(twice[k], g) and p.grad.shape == p.shape
        assert bool(((p.grad - 2 * g).abs() <= 2.0 ** -22 * g.abs()).all()), k  # one rounding of the addition
    assert all(p.grad is None for n, p in lg.named_parameters() if n not in once)
    b, m = case["keypoints0"].shape[:2]
    n = case["keypoints1"].shape[1]
    full = lg.layer_loss_backward(pred, labels(case), descriptor_grads=True, accumulate=False)
    d0, d1 = full["grad_ref_descriptors0"], full["grad_ref_descriptors1"]
    assert d0.shape == (b, 9, m, 256) and d1.shape == (b, 9, n, 256)
    assert d0.untyped_storage().data_ptr() == d1.untyped_storage().data_ptr()
    assert d0.stride() == (m * 256, b * (m + n) * 256, 256, 1) and d1.stride() == (n * 256, b * (m + n) * 256, 256, 1)
    # grad_total: linear, and a zero entry removes the pair
    w = torch.arange(b, dtype=torch.float32) * 0.5
    scaled = lg.layer_loss_backward(pred, labels(case), grad_total=w, descriptor_grads=True, accumulate=False)
    assert bool((scaled["grad_ref_descriptors0"][0] == 0).all())
    with pytest.raises(ValueError, match="grad_total"):
        lg.layer_loss_backward(pred, labels(case), grad_total=torch.ones(b + 1), accumulate=False)
    with pytest.raises(NotImplementedError, match="fp32 matcher"):
        model(matmul_precision="fp16").layer_loss_backward(pred, labels(case))
    with pytest.raises(NotImplementedError, match="depth_confidence"):
        model(depth_confidence=0.9).layer_loss_backward(pred, labels(case))
    with pytest.raises(ValueError, match="forward_layers"):
        lg.layer_loss_backward({**pred, "ref_descriptors0": pred["ref_descriptors0"][:, -1:]}, labels(case))


@pytest.mark.parametrize("where", ["cuda", "cpu", "fp16", "graph"])
def test_sgd_step_heads_updated_and_descent(where):
    """An SGD step of the stored EPS on every head and token, `heads_updated()`, and `forward_layers` is what a fresh
    module loaded from `state_dict()` gives; the loss of that module has fallen by EPS |grad|^2 within [0.9, 1.1] (the
    host test holds the float64 ratio to [0.95, 1.05]; the rest covers fp32 rounding of a loss difference of relative
    size >= 1e-3).  Parameters on the device (the kernels read them where they are), on the host (device copies,
    refreshed in place), with fp16 copies, and under a captured graph."""
    z = np.load(os.path.join(GOLDEN, "head_grad_a_gamma1.npz"))
    case = lc.make_case("a", int(z["seed"]))
    conf = {"weights": "synthetic", "filter_threshold": 0.0}
    if where == "fp16":
        conf["matmul_precision"] = "fp16"
    if where == "graph":
        conf["graph_max_rows"] = 4096
    lg = lightglue.LightGlue(conf).eval()
    if where != "cpu":
        lg = lg.cuda()
    data = inputs(case)
    with torch.no_grad():
        pred = lg.forward_layers(data)
        plain = lg(data)
        before, _ = lg.layer_loss(pred, labels(case))
    if where == "fp16":  # gradients are built for the fp32 matcher: they come from an fp32 module of the same weights
        donor = model()
        with torch.no_grad():
            grads = donor.layer_loss_backward(donor.forward_layers(data), labels(case), accumulate=False)
        for k, g in grads.items():
            lg.get_parameter(k).grad = g.clone()
    else:
        grads = lg.layer_loss_backward(pred, labels(case))
    names = set(grads)
    opt = torch.optim.SGD([p for k, p in lg.named_parameters() if k in names], lr=EPS)
    opt.step()
    lg.heads_updated()
    fresh = lightglue.LightGlue(conf).eval()
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in lg.state_dict().items()})
    fresh = fresh.cuda()
    with torch.no_grad():
        new, want = lg.forward_layers(data), fresh.forward_layers(data)
        new_plain, want_plain = lg(data), fresh(data)
        after, _ = fresh.layer_loss(want, labels(case))
    for k in want:
        assert torch.equal(new[k], want[k]), k
        assert torch.equal(new_plain[k], want_plain[k]), k
    assert not torch.equal(new_plain["log_assignment"], plain["log_assignment"])
    assert torch.equal(new["ref_descriptors0"], pred["ref_descriptors0"])  # the trunk has not moved
    if where != "fp16":
        sq = sum(float((g.double() ** 2).sum()) for g in grads.values())
        ratio = float((after["total"].double().mean() - before["total"].double().mean())) / (-EPS * sq)
        print(f"{where}: descent ratio {ratio:.4f}: total {float(before['total'].mean()):.6f} -> "
              f"{float(after['total'].mean()):.6f}")
        assert 0.9 <= ratio <= 1.1


def test_finetune_heads_on_a_generated_directory(tmp_path, capsys):
    import shutil

    from glue_factory_colon_amd import finetune_heads, weights

    names = er.make_tree(tmp_path, per_sequence=3, hw=(120, 160))
    for n in names:
        shutil.copy(tmp_path / "frames" / "test" / n, tmp_path / "frames" / "val" / n)
    out = tmp_path / "tuned.pth"
    before, after = finetune_heads.main(["--data_dir", str(tmp_path / "frames"), "--pair_batch", "4",
                                         "--max_num_keypoints", "128", "--num_workers", "0", "--params", "tokens",
                                         "--epochs", "2", "--max_steps", "2", "--out", str(out)])
    text = capsys.readouterr().out
    assert "before: loss/total_deep" in text and "after 2 steps: loss/total_deep" in text
    assert len([ln for ln in text.splitlines() if ln.startswith("layer index")]) == 2
    tuned = torch.load(str(out), map_location="cpu")
    start = weights.lightglue_state_dict(0)
    moved = [k for k, v in start.items() if k in tuned and not torch.equal(tuned[k], v)]
    assert moved and all(k.startswith("token_confidence.") for k in moved), moved
    assert len(moved) == 2 * 8
    assert after["loss/confidence"] != before["loss/confidence"]
    assert abs(after["loss/assignment_nll"] - before["loss/assignment_nll"]) <= 1e-6  # the heads have not moved
    loaded = lightglue.LightGlue({"weights": str(out)}).eval().cuda()
    for k, v in tuned.items():
        assert torch.equal(loaded.state_dict()[k].cpu(), v), k


def test_layer_loss_and_backward_in_either_order():
    """`layer_loss` and `layer_loss_backward` build the same layer pass (one set of per-layer buffers, the module's one
    workspace): on one prediction, loss then backward on one module and backward then loss on a fresh one give the same
    bits, and `.grad` after two accumulating calls is the sum of two non-accumulating results added in that order.
    2 x (130 + 65) points, 3 layers: no multiple of the 64-row tiles, M != N."""
    b, m, n = 2, 130, 65
    g = torch.Generator().manual_seed(11)
    size = torch.tensor([[640.0, 480.0]] * b).cuda()
    data = {"keypoints0": (torch.rand((b, m, 2), generator=g) * 479).cuda(),
            "keypoints1": (torch.rand((b, n, 2), generator=g) * 479).cuda(), "descriptors0": rows(b, m, 12).cuda(),
            "descriptors1": rows(b, n, 13).cuda(), "view0": {"image_size": size}, "view1": {"image_size": size}}
    gt0, gt1, gta = make_labels(b, m, n, 14, "assignment")
    lab = {"gt_matches0": gt0.cuda(), "gt_matches1": gt1.cuda(), "gt_assignment": gta.cuda()}

    def run(order):
        lg = model(n_layers=3)
        with torch.no_grad():
            pred = lg.forward_layers(data)
        out = {}
        for what in order:
            if what == "loss":
                with torch.no_grad():
                    out["losses"], out["report"] = lg.layer_loss(pred, lab)
            else:
                out["grads"] = lg.layer_loss_backward(pred, lab, accumulate=False)
        return lg, pred, out

    lg, pred, first = run(("loss", "backward"))
    _, other_pred, second = run(("backward", "loss"))
    for k in pred:
        assert torch.equal(pred[k], other_pred[k]), k
    assert len(first["grads"]) == 4 * 3 + 2 * 2 and any(k.startswith("token_confidence.") for k in first["grads"])
    for part in ("losses", "report", "grads"):
        assert set(first[part]) == set(second[part])
        for k, v in first[part].items():
            assert bool(torch.isfinite(v).all()) and torch.equal(v, second[part][k]), (part, k)
    assert all(p.grad is None for p in lg.parameters())
    lg.layer_loss_backward(pred, lab)
    lg.layer_loss_backward(pred, lab)
    for k, v in first["grads"].items():
        want = v.clone()
        want += second["grads"][k]
        assert bool((v != 0).any()) and torch.equal(lg.get_parameter(k).grad, want), k


def test_print_the_worst_fractions():
    """Last in the file: the largest fraction of a bound that any test above used, per output."""
    for k in sorted(WORST):
        print(f"worst fraction of the bound, {k}: {WORST[k]:.3f}")
