"""The head and exit-token gradients without a GPU: tests/head_grad_reference.py (the float64 closed form the GPU tests
compare with, and its per-element bounds) against the gradients the reference's own autograd produced
(tests/golden/head_grad_*.npz, made by make_head_grad_golden.py), the wrong variants it must reject, a descent check,
and the contracts of the new entry points (refusals, the binding's header).  Nothing is launched.

The descriptors of every layer are not stored (7 MB in float64): they are recomputed in float64 by the oracle's
LightGlue (oracle/lightglue.py) from the inputs of tests/layer_loss_cases.py, and held to the rows the per-layer loss
fixture sampled from the reference's own float64 run (tests/golden/layer_loss_rows.npz).

Comparisons.  Against the reference's FLOAT64 gradients the closed form is held to 1e-10 relative: per element
|difference| <= 1e-10 x (abs-sum of the element), the scale its terms have before they cancel, and per tensor
||difference|| <= 1e-10 ||reference||.  The exit tokens are the exception: the reference evaluates the token loss in
FLOAT32 in both of its runs (BCEWithLogitsLoss takes its output type from the float32 target `correct.float()`,
lightglue.py:93-94), so the token gradients of its float64 run carry float32 roundings of every term and are held to
4 x 2^-23 x abs-sum instead.  The reference's FLOAT32 gradients must stay inside the per-element bound
c 2^-23 abs-sum that the GPU is held to, with c + trunk_c(L): the float32 run of the reference also computes the trunk
in float32, which the bound of the head alone (exact descriptors) does not cover (head_grad_reference.trunk_c).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue, two_view_pipeline, weights  # noqa: E402
from oracle import lightglue as olg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GAMMAS = {"05": 0.5, "0": 0.0, "1": 1.0}
C_TRUNK = hg.trunk_c(lc.N_LAYERS)
# the descent check: total(theta - EPS grad) - total(theta) = -EPS |grad|^2 (1 + O(EPS)) on case `a`, gamma 1.0
EPS = 0.05
_CACHE = {}


def state_dict64():
    if "sd" not in _CACHE:
        _CACHE["sd"] = {k: v.double() for k, v in weights.lightglue_state_dict(0).items()}
    return _CACHE["sd"]


def layers64(name):
    """(case, xs0, xs1): the inputs of case `name` and the float64 descriptors of every layer."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"head_grad_{name}_gamma1.npz"))
        case = lc.make_case(name, int(z["seed"]))
        assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"]))
        f = lambda t: t.double()
        out = olg.match(state_dict64(), f(case["keypoints0"]), f(case["keypoints1"]), f(case["descriptors0"]),
                        f(case["descriptors1"]), f(case["size"]), f(case["size"]), n_layers=lc.N_LAYERS,
                        return_layers=True)
        _CACHE[name] = (case, [x0 for x0, _ in out["layers"]], [x1 for _, x1 in out["layers"]])
    return _CACHE[name]


def labels(case):
    return {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"], "gt_assignment": case["gt_assignment"]}


def stored(z, suffix=""):
    """{state-dict name: stored gradient, or for final_proj.weight the dict of its stored parts} of one fixture."""
    nl = lc.N_LAYERS
    t = lambda k: torch.from_numpy(z[k + suffix]).double()
    out = {}
    for i in range(nl):
        p = f"log_assignment.{i}."
        out[p + "final_proj.bias"] = t("bf")[i]
        out[p + "matchability.weight"] = t("wm")[i].reshape(1, 256)
        out[p + "matchability.bias"] = t("bm")[i].reshape(1)
        out[p + "final_proj.weight"] = {"rows": t("wf_rows")[i], "cols": t("wf_cols")[i], "sumsq": t("wf_sumsq")[i],
                                        "bilinear": t("wf_bilinear")[i]}
    for i in range(nl - 1):
        p = f"token_confidence.{i}.token.0."
        out[p + "weight"] = t("tw")[i].reshape(1, 256)
        out[p + "bias"] = t("tb")[i].reshape(1)
    return out


def fractions(z, grads, sums, scale, suffix="", norm_tol=None):
    """The largest |stored - grads| / (scale[name] x abs-sum) over every stored element (the bilinear checksum against
    u^T abs-sum v); with norm_tol also asserts the sum of squares of final_proj.weight."""
    rows, cols = torch.from_numpy(z["rows"]), torch.from_numpy(z["cols"])
    u, v = torch.from_numpy(z["u"]), torch.from_numpy(z["v"])
    worst = 0.0
    for name, ref in stored(z, suffix).items():
        g, s, k = grads[name], sums[name], scale(name)
        if isinstance(ref, dict):
            worst = max(worst, float(((g[rows] - ref["rows"]).abs() / (k * s[rows])).max()),
                        float(((g[:, cols] - ref["cols"]).abs() / (k * s[:, cols])).max()),
                        float((u @ g @ v - ref["bilinear"]).abs() / (k * (u.abs() @ s @ v.abs()))))
            if norm_tol is not None:
                assert abs(float((g ** 2).sum() / ref["sumsq"]) - 1.0) <= norm_tol, name
        else:
            worst = max(worst, float(((g - ref).abs() / (k * s)).max()))
            if norm_tol is not None and "token" not in name:
                assert float((g - ref).norm()) <= norm_tol * float(ref.norm()), name
    return worst


@pytest.mark.parametrize("name", ["a", "b"])
def test_oracle_layers_are_the_reference_layers(name):
    _, xs0, xs1 = layers64(name)
    z = np.load(os.path.join(GOLDEN, "layer_loss_rows.npz"))
    rows0, rows1 = lc.sample_rows(name)
    for side, xs, rows in (("0", xs0, rows0), ("1", xs1, rows1)):
        flat = torch.stack([x.reshape(-1, 256) for x in xs])
        assert np.allclose(flat[:, rows].numpy(), z[f"{name}_ref{side}_rows"], rtol=0, atol=2e-7 * float(flat.abs().max()))
        assert np.allclose((flat ** 2).sum((1, 2)).numpy(), z[f"{name}_ref{side}_sumsq"], rtol=1e-11)


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("tag", list(GAMMAS))
def test_closed_form_is_the_reference_autograd(name, tag):
    case, xs0, xs1 = layers64(name)
    z = np.load(os.path.join(GOLDEN, f"head_grad_{name}_gamma{tag}.npz"))
    grads, sums, cs = hg.model_grads(xs0, xs1, state_dict64(), labels(case), gamma=GAMMAS[tag], descriptor_grads=True)
    w64 = fractions(z, grads, sums, lambda k: 4 * hg.U if "token" in k else 1e-10, norm_tol=1e-10)
    w32 = fractions(z, grads, sums, lambda k: (cs[k] + C_TRUNK) * hg.U, suffix="_f32")
    print(f"case {name} gamma {GAMMAS[tag]}: float64 run uses {w64:.3f} of 1e-10 x abs-sum, float32 run {w32:.3f} of "
          f"its bound")
    assert w64 <= 1.0 and w32 <= 1.0
    # the token targets the closed form derived are the reference's
    import layer_loss_reference as lr
    las = [hg.head_forward(xs0[i], xs1[i], *hg.head_params(state_dict64(), i)) for i in range(lc.N_LAYERS)]
    for i in range(lc.N_LAYERS - 1):
        c0, c1 = lr.token_targets(las[i], las[-1])
        assert torch.equal(c0, torch.from_numpy(z["correct0"][i])) and torch.equal(c1, torch.from_numpy(z["correct1"][i]))
    if tag == "05":  # the direct gradient at the descriptors
        d = np.load(os.path.join(GOLDEN, f"head_grad_dx_{name}.npz"))
        for side in ("0", "1"):
            k = "grad_ref_descriptors" + side
            g = grads[k].permute(1, 0, 2, 3).reshape(lc.N_LAYERS, -1, 256)
            s = sums[k].permute(1, 0, 2, 3).reshape(lc.N_LAYERS, -1, 256)
            rows = torch.from_numpy(d["rows" + side])
            ref, ref32 = torch.from_numpy(d["dx" + side]), torch.from_numpy(d[f"dx{side}_f32"]).double()
            assert float(((g[:, rows] - ref).abs() / (1e-10 * s[:, rows])).max()) <= 1.0
            assert np.allclose((g ** 2).sum((1, 2)).numpy(), d[f"dx{side}_sumsq"], rtol=1e-10)
            assert float(((g[:, rows] - ref32).abs() / ((cs[k] + C_TRUNK) * hg.U * s[:, rows])).max()) <= 1.0


def _synthetic(seed=3):
    """B = 2, 7 + 6 points: pair 0 has a row with three positives and a column with two; pair 1 has no positive."""
    g = torch.Generator().manual_seed(seed)
    # descriptors of norm 0.8: |S| stays below 1, so the soft-max factors are as well conditioned as fp32 allows
    x0 = 0.05 * torch.randn((2, 7, 256), generator=g, dtype=torch.float64)
    x1 = 0.05 * torch.randn((2, 6, 256), generator=g, dtype=torch.float64)
    gta = torch.zeros((2, 7, 6), dtype=torch.bool)
    gta[0, 1, 0] = gta[0, 1, 2] = gta[0, 1, 3] = gta[0, 4, 3] = gta[0, 5, 5] = True
    gt0 = torch.tensor([[-1, 0, -1, -2, 3, 5, -1], [-1, -1, -2, -1, -1, -2, -1]])
    gt1 = torch.tensor([[1, -1, 1, 1, -2, 5], [-1, -1, -1, -2, -1, -1]])
    return x0, x1, gt0, gt1, gta


def _autograd(x0, x1, params, gt0, gt1, gta, g, lam):
    """The same gradients from torch autograd of the float64 forward (layer_loss_reference's nll)."""
    import layer_loss_reference as lr
    leaves = [t.clone().requires_grad_(True) for t in (x0, x1, *params)]
    la = hg.head_forward(*leaves)
    data = {"gt_matches0": gt0, "gt_matches1": gt1, "gt_assignment": gta}
    nll = lr.weighted_nll(la, lr.nll_weights(la.detach(), data), lam)["assignment_nll"]
    (nll * g).sum().backward()
    return dict(zip(("dx0", "dx1", "dWf", "dbf", "dwm", "dbm"), [t.grad for t in leaves]))


def test_closed_form_on_repeated_positives_and_an_empty_pair():
    x0, x1, gt0, gt1, gta = _synthetic()
    params = hg.head_params(state_dict64(), 4)
    g = torch.tensor([0.7, -0.3], dtype=torch.float64)
    want = _autograd(x0, x1, params, gt0, gt1, gta, g, 0.3)
    grads, sums = hg.head_grad(x0, x1, *params, gt0, gt1, gta, g, 0.3)
    for k, ref in want.items():
        assert float(((grads[k] - ref).abs() / (1e-10 * sums[k] + 1e-300)).max()) <= 1.0, k


def _variant_worst(variant):
    """The largest fraction of a bound that the variant's closed form misses by, over the fixtures (float64 run, the
    GPU's constant c) and the synthetic case (against autograd)."""
    worst = 0.0
    for name in ("a", "b"):
        case, xs0, xs1 = layers64(name)
        for tag in ("05", "1"):
            z = np.load(os.path.join(GOLDEN, f"head_grad_{name}_gamma{tag}.npz"))
            grads, _, _ = hg.model_grads(xs0, xs1, state_dict64(), labels(case), gamma=GAMMAS[tag], variant=variant)
            _, sums, cs = hg.model_grads(xs0, xs1, state_dict64(), labels(case), gamma=GAMMAS[tag])
            w = fractions(z, grads, sums, lambda k: cs[k] * hg.U)
            worst = max(worst, w if math.isfinite(w) else float("inf"))
    x0, x1, gt0, gt1, gta = _synthetic()
    params = hg.head_params(state_dict64(), 4)
    g = torch.tensor([0.7, -0.3], dtype=torch.float64)
    want = _autograd(x0, x1, params, gt0, gt1, gta, g, 0.3)
    grads, _ = hg.head_grad(x0, x1, *params, gt0, gt1, gta, g, 0.3, variant=variant)
    _, sums = hg.head_grad(x0, x1, *params, gt0, gt1, gta, g, 0.3)
    c = hg.head_c(2, 7, 6)
    for k, ref in want.items():
        w = float(((grads[k] - ref).abs() / (c["dx" if k.startswith("dx") else k] * hg.U * sums[k] + 1e-300)).max())
        worst = max(worst, w if math.isfinite(w) else float("inf"))
    return worst


@pytest.mark.parametrize("variant", hg.VARIANTS)
def test_wrong_variants_miss_a_bound(variant):
    worst = _variant_worst(variant)
    print(f"{variant}: misses a bound by {worst:.3g} x")
    assert worst >= 100.0


def test_no_variant_is_the_closed_form_itself():
    assert _variant_worst(None) <= 1.0


def test_descent_along_the_gradient():
    """total(theta - EPS grad) - total(theta), divided by -EPS |grad|^2, lies in [0.95, 1.05] (float64, case a)."""
    case, xs0, xs1 = layers64("a")
    sd = state_dict64()
    grads, _, _ = hg.model_grads(xs0, xs1, sd, labels(case), gamma=1.0)
    before = hg.total_loss(xs0, xs1, sd, labels(case), gamma=1.0).mean()
    stepped = {k: (v - EPS * grads[k].reshape(v.shape) if k in grads else v) for k, v in sd.items()}
    after = hg.total_loss(xs0, xs1, stepped, labels(case), gamma=1.0).mean()
    sq = sum(float((g ** 2).sum()) for g in grads.values())
    ratio = float(after - before) / (-EPS * sq)
    print(f"descent ratio {ratio:.4f} at eps {EPS}: total {float(before):.6f} -> {float(after):.6f}, |grad|^2 {sq:.4e}")
    assert 0.95 <= ratio <= 1.05
    assert abs(float(after - before)) >= 1e-3 * abs(float(before))  # large enough to be seen in fp32 on the GPU


def test_layer_weights():
    assert hg.layer_weights(3, 1.0) == [1 / 3, 1 / 3, 1 / 3]
    assert hg.layer_weights(3, 0.0) == [1 / 4, 2 / 4, 1 / 4]
    assert hg.layer_weights(3, 0.5) == [0.25 / 1.75, 0.5 / 1.75, 1 / 1.75]


def _pred(nl, m, n, b=1):
    return {"ref_descriptors0": torch.zeros(b, nl, m, 256), "ref_descriptors1": torch.zeros(b, nl, n, 256),
            "log_assignment": torch.zeros(b, m + 1, n + 1), "matches0": torch.zeros(b, m).long(),
            "matching_scores0": torch.zeros(b, m)}


def _labels(m, n, b=1):
    return {"gt_matches0": torch.full((b, m), -1), "gt_matches1": torch.full((b, n), -1)}


def test_refusals_of_layer_loss_backward():
    lg = lightglue.LightGlue({"weights": "synthetic"}).eval()
    with pytest.raises(ValueError, match="forward_layers"):
        lg.layer_loss_backward(_pred(1, 3, 4), _labels(3, 4))
    with pytest.raises(ValueError, match="without key points"):
        lg.layer_loss_backward(_pred(9, 0, 4), _labels(0, 4))
    for conf in ({"depth_confidence": 0.95}, {"width_confidence": 0.99}):
        with pytest.raises(NotImplementedError, match="depth_confidence / width_confidence"):
            lightglue.LightGlue({"weights": "synthetic", **conf}).layer_loss_backward(_pred(9, 3, 4), _labels(3, 4))
    with pytest.raises(NotImplementedError, match="only 'nll'"):
        lightglue.LightGlue({"weights": "synthetic", "loss": {"fn": "focal"}}).layer_loss_backward(_pred(9, 3, 4),
                                                                                                   _labels(3, 4))
    with pytest.raises(NotImplementedError, match="fp32 matcher"):
        lightglue.LightGlue({"weights": "synthetic", "matmul_precision": "fp16"}).layer_loss_backward(_pred(9, 3, 4),
                                                                                                      _labels(3, 4))
    with pytest.raises(nat.NativeError, match="no CPU implementation"):
        lg.layer_loss_backward(_pred(9, 3, 4), _labels(3, 4))
    lg.heads_updated()  # nothing packed yet: nothing to refresh
    pipe = two_view_pipeline.TwoViewPipeline({"matcher": {"name": "matchers.lightglue", "weights": "synthetic"},
                                              "allow_no_extract": True})
    with pytest.raises(ValueError, match="forward_layers"):
        pipe.layer_loss_backward(_pred(1, 3, 4), _labels(3, 4), accumulate=False)


def test_the_head_backward_header_is_parsed_by_the_same_grammar_and_exported():
    assert sorted(nat.HEAD_BACKWARD_FUNCTIONS) == ["gfc_lg_head_backward", "gfc_lg_head_backward_workspace_bytes",
                                                   "gfc_lg_token_backward", "gfc_lg_token_backward_workspace_bytes"]
    earlier = (set(nat.FUNCTIONS) | set(nat.VALIDATION_FUNCTIONS) | set(nat.SPARSE_MAP_FUNCTIONS)
               | set(nat.DENSE_WARP_FUNCTIONS) | set(nat.CROSS_ATTENTION_FUNCTIONS) | set(nat.LAYER_SCORES_FUNCTIONS))
    assert not set(nat.HEAD_BACKWARD_FUNCTIONS) & earlier
    with open(nat.HEAD_BACKWARD_HEADER_PATH) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert funcs == nat.HEAD_BACKWARD_FUNCTIONS and not structs and not enums and not consts
    ret, params = funcs["gfc_lg_head_backward"]
    assert ret == "int" and [p for p, _ in params] == [
        "p", "layer", "x0", "x1", "gt_matches0", "gt_matches1", "gt_assignment", "g", "nll_balancing", "B", "M", "N",
        "dWf", "dbf", "dwm", "dbm", "dx", "ws", "ws_bytes", "stream"]
    ret, params = funcs["gfc_lg_token_backward"]
    assert ret == "int" and [p for p, _ in params] == [
        "x0", "x1", "logit0", "logit1", "correct0", "correct1", "g", "n_layers", "B", "M", "N", "dtoken_w", "dtoken_b",
        "ws", "ws_bytes", "stream"]
    lib = nat.lib()
    for name in nat.HEAD_BACKWARD_FUNCTIONS:
        assert getattr(lib, name).argtypes == nat.HEAD_BACKWARD_SIGNATURES[name][1]
    # the size queries run on the host: refused shapes give 0; the formula is the header's
    for size in (lib.gfc_lg_head_backward_workspace_bytes, lib.gfc_lg_token_backward_workspace_bytes):
        assert size(0, 4, 4) == 0 and size(1, 0, 4) == 0 and size(1, 4, 0) == 0 and size(1, 65536, 4) == 0
        assert size(1, 4, 65536) == 0 and size(65536, 4, 4) == 0 and size(1, 1, 1) > 0
        assert size(128, 65535, 1) == 0 < size(127, 65535, 513)  # B (M + N) <= 8388607
    al = lambda x: (x + 255) // 256 * 256

    def parts(rows):
        k = -(-(-(-rows // min(-(-rows // 1024), 128))) // 16) * 16
        return -(-rows // k)

    def head_bytes(b, m, n):
        r = b * (m + n)
        return (2 * al(r * 1024) + 2 * al(r * 4) + al(b * m * n * 4) + 2 * al(b * m * 4) + 2 * al(b * n * 4) + al(b * 8)
                + al((parts(b * m) + parts(b * n)) * 262144) + al(-(-r // 128) * 2080))

    for b, m, n in ((1, 1, 65), (3, 257, 300), (2, 1024, 1025), (32, 2048, 2048), (5, 30000, 7)):
        assert lib.gfc_lg_head_backward_workspace_bytes(b, m, n) == head_bytes(b, m, n), (b, m, n)
        r = b * (m + n)
        assert lib.gfc_lg_token_backward_workspace_bytes(b, m, n) == al(r * 4) + al(-(-r // 128) * 2080)
    with pytest.raises(nat.NativeError, match="must be on a 'cuda'"):
        nat.call("gfc_lg_token_backward", torch.zeros(1, 256), torch.zeros(1, 256), torch.zeros(1), torch.zeros(1),
                 torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), torch.zeros(1), 9, 1, 1, 1,
                 torch.zeros(256), torch.zeros(1), torch.zeros(4096, dtype=torch.uint8), 4096)
