"""The per-layer loss without a GPU: tests/layer_loss_reference.py (the float64 restatement the GPU tests compare with)
against vectors the reference project produced in training mode (tests/golden/layer_loss*.npz, made by
make_layer_loss_golden.py), the wrong variants it must reject, the fixture's margin condition, and the contracts of
the new entry points (refusals, the binding's header).  Nothing is launched.

Bound of the float comparison.  The fixture stores the log assignments of the reference's float64 run rounded to
float32 -- every entry within u = 2^-24 relative of what the reference summed -- and the token logits in float64.  So
  nll_pos, nll_neg, assignment_nll, per-layer nll : u x the same weighted mean taken over |la| (a mean of entries each
                                                    off by at most u |la|),
  row_norm                                        : u x mean_i sum_j |la| exp(la) (exp(la (1 + d)) to first order),
  confidence                                      : the reference evaluates the token loss in FLOAT32 in both of its runs
                                                    (BCEWithLogitsLoss takes its output type from the float32 target
                                                    `correct.float()`, lightglue.py:93-94), so its own value carries:
                                                    the logit cast (u mean|x|: the loss has slope <= 1), one rounding
                                                    per element, ceil(log2 max(M, N)) of the pairwise mean and its
                                                    division, the sum of the two sides and the division by L - 1
                                                    (together ceil(log2 max(M, N)) + 4 roundings of the term), and
                                                    L - 1 float32 additions into the running sum (each <= u confidence),
  total                                           : the weighted mean of the layers' bounds plus that of confidence,
plus 1e-12 (1 + |value|) for the float64 arithmetic of either side.  The test prints the largest fraction of its bound
that any value used.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_loss_cases as lc  # noqa: E402
import layer_loss_reference as lr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue, losses, two_view_pipeline  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
F64 = 1e-12
GAMMAS = {"05": 0.5, "0": 0.0, "1": 1.0}
FILES = {"a": "layer_loss", "b": "layer_loss_b1"}


@pytest.fixture(scope="module", params=["a", "b"])
def fx(request):
    name = request.param
    z = np.load(os.path.join(ROOT, "tests", "golden", FILES[name] + ".npz"))
    case = lc.make_case(name, int(z["seed"]))
    return name, z, case


def restate(z, case, gamma, variant=None):
    la = torch.from_numpy(z["la"]).double()
    data = {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"], "gt_assignment": case["gt_assignment"]}
    return lr.layer_loss(list(la), list(torch.from_numpy(z["logit0"])), list(torch.from_numpy(z["logit1"])), data,
                         [float(t) for t in z["thresholds"]], gamma=gamma, variant=variant)


def bounds(z, case, gamma):
    """{key: [B] bound} for the losses and `nll` [L,B], as derived in the module docstring."""
    la = torch.from_numpy(z["la"]).double()
    data = {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"], "gt_assignment": case["gt_assignment"]}
    w = lr.nll_weights(la[-1], data)
    mag = [lr.weighted_nll(x.abs(), w) for x in la]
    nl = la.shape[0]
    out = {k: U * mag[-1][k].abs() for k in ("assignment_nll", "nll_pos", "nll_neg")}
    out["last"] = out["assignment_nll"]
    out["nll"] = torch.stack([U * m["assignment_nll"].abs() for m in mag])
    out["row_norm"] = U * (la[-1].abs() * la[-1].exp())[:, :-1].sum(2).mean(1)
    conf = torch.from_numpy(z["losses_gamma1"])[list(z["loss_keys"]).index("confidence")]
    x0, x1 = torch.from_numpy(z["logit0"]).abs().mean(-1), torch.from_numpy(z["logit1"]).abs().mean(-1)  # [L-1,B]
    roundings = math.ceil(math.log2(max(la.shape[2], la.shape[3]) - 1)) + 4 + (nl - 1)
    out["confidence"] = U * (roundings * conf + ((x0 + x1) / 2.0 / (nl - 1)).sum(0))
    weights = [gamma ** (nl - i - 1) if gamma > 0 else i + 1 for i in range(nl - 1)]
    out["total"] = (out["nll"][-1] + sum(wt * out["nll"][i] for i, wt in enumerate(weights))) / (1.0 + sum(weights)) \
        + out["confidence"]
    out["num_matchable"] = out["num_unmatchable"] = torch.zeros_like(out["last"])
    return out


def misses(z, case, variant=None):
    """(a stored boolean or count differs, the largest |difference| / bound over every stored float)."""
    changed, worst = False, 0.0
    for tag, gamma in GAMMAS.items():
        got, report, targets = restate(z, case, gamma, variant)
        bd = bounds(z, case, gamma)
        want = dict(zip([str(k) for k in z["loss_keys"]], torch.from_numpy(z[f"losses_gamma{tag}"])))
        for k, ref in want.items():
            tol = bd[k] + F64 * (1 + ref.abs())
            worst = max(worst, float(((got[k] - ref).abs() / tol).max()))
        ref = torch.from_numpy(z["nll"])
        worst = max(worst, float(((report["layer_nll"].t() - ref).abs() / (bd["nll"] + F64 * (1 + ref.abs()))).max()))
        c0 = torch.stack([t[0] for t in targets])
        c1 = torch.stack([t[1] for t in targets])
        changed |= not torch.equal(c0, torch.from_numpy(z["correct0"])) or not torch.equal(c1, torch.from_numpy(z["correct1"]))
        m, n = c0.shape[-1], c1.shape[-1]
        conf = torch.from_numpy(z["conf0"] + z["conf1"]).t().double() / (m + n)
        changed |= not torch.equal(report["layer_ratio_confident"], conf)
        agree = (c0.sum(-1) + c1.sum(-1)).t().double() / (m + n)
        changed |= not torch.equal(report["layer_agree"], agree)
    if "probe_logits" in z.files:  # float32, as the reference evaluates the predicate
        x = torch.from_numpy(z["probe_logits"])
        n0, _ = lr.confident_counts(x, x, torch.from_numpy(z["probe_threshold"]), variant)
        changed |= not torch.equal(n0, torch.from_numpy(z["probe_count"]))
    return changed, worst


def test_the_inputs_are_the_ones_the_fixture_was_made_from(fx):
    _, z, case = fx
    assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"]))
    la = z["la"]
    assert la.shape == (lc.N_LAYERS, case["keypoints0"].shape[0], case["keypoints0"].shape[1] + 1,
                        case["keypoints1"].shape[1] + 1)


def test_restatement_reproduces_every_stored_value(fx):
    name, z, case = fx
    changed, worst = misses(z, case)
    print(f"case {name}: largest fraction of the bound used {worst:.3f}")
    assert not changed and worst <= 1.0, (changed, worst)
    # the matches of every layer's own head, which the report's recall / precision are made from
    la = torch.from_numpy(z["la"]).double()
    for i in range(la.shape[0]):
        assert torch.equal(lr.filter_matches(la[i])[0], torch.from_numpy(z["layer_matches0"][i]))
    # the float32 run of the reference is within the suite's parity bound of its float64 run
    for tag in GAMMAS:
        a, b = z[f"losses_gamma{tag}_f32"], z[f"losses_gamma{tag}"]
        assert np.all(np.abs(a - b) <= 1e-4 * (1 + np.abs(b)))


@pytest.mark.parametrize("variant", lr.VARIANTS)
def test_wrong_variants_miss_the_fixture(variant):
    """Each deliberate mistake changes a stored boolean / count or misses a stored float by at least 100 x its bound, in
    at least one of the two batches (joint_neg_clamp shows in batch b only: side 0 has no unmatched point there)."""
    seen = []
    for name, fname in FILES.items():
        z = np.load(os.path.join(ROOT, "tests", "golden", fname + ".npz"))
        changed, worst = misses(z, lc.make_case(name, int(z["seed"])), variant)
        seen.append((name, changed, worst))
    print(variant, seen)
    assert any(changed or worst >= 100.0 for _, changed, worst in seen), seen


def test_margin_condition_of_the_fixture(fx):
    """Every row (dustbin column included) and every column (dustbin row included) of every layer's log assignment has
    its two largest entries at least 1e-3 apart: no target can flip under a 1e-4 (1 + |la|) parity of the assignment
    unless |la| at the top exceeds 4 -- which the second assertion rules out at the gap each line has."""
    _, z, _ = fx
    la = torch.from_numpy(z["la"]).double()
    worst = float("inf")
    for x in la:
        for part, dim in ((x[:, :-1, :], 2), (x[:, :, :-1], 1)):
            top = part.topk(2, dim).values
            gap = top.select(dim, 0) - top.select(dim, 1)
            worst = min(worst, float(gap.min()))
            # both entries may move by 1e-4 (1 + |entry|) against each other
            room = 1e-4 * (2 + top.select(dim, 0).abs() + top.select(dim, 1).abs())
            assert bool((gap > room).all()), float((gap - room).min())
    print(f"smallest top-2 gap {worst:.3e}")
    assert worst >= 1e-3 and abs(worst - float(z["min_gap"])) < 1e-4


def test_argmax_rule_of_the_restatement():
    x = torch.tensor([[1.0, 3.0, 3.0, float("nan")], [float("-inf")] * 4, [float("nan"), -1.0, float("inf"), float("inf")]])
    assert lr.argmax_low(x, 1).tolist() == [1, 0, 2]
    assert lr.argmax_low(x.t(), 0).tolist() == [1, 0, 2]


def _pred(nl, m, n, b=1):
    return {"ref_descriptors0": torch.zeros(b, nl, m, 256), "ref_descriptors1": torch.zeros(b, nl, n, 256),
            "log_assignment": torch.zeros(b, m + 1, n + 1), "matches0": torch.zeros(b, m).long(),
            "matching_scores0": torch.zeros(b, m)}


def _labels(m, n, b=1):
    return {"gt_matches0": torch.full((b, m), -1), "gt_matches1": torch.full((b, n), -1)}


def test_refusals_of_the_new_entry_points():
    lg = lightglue.LightGlue({"weights": "synthetic"}).eval()
    with pytest.raises(ValueError, match="forward_layers"):
        lg.layer_loss(_pred(1, 3, 4), _labels(3, 4))
    with pytest.raises(ValueError, match="without key points"):
        lg.layer_loss(_pred(9, 0, 4), _labels(0, 4))
    for conf in ({"depth_confidence": 0.95}, {"width_confidence": 0.99}):
        adaptive = lightglue.LightGlue({"weights": "synthetic", **conf}).eval()
        with pytest.raises(NotImplementedError, match="depth_confidence / width_confidence"):
            adaptive.forward_layers({"keypoints0": torch.zeros(1, 3, 2), "keypoints1": torch.zeros(1, 3, 2),
                                     "descriptors0": torch.zeros(1, 3, 256), "descriptors1": torch.zeros(1, 3, 256)})
        with pytest.raises(NotImplementedError, match="depth_confidence / width_confidence"):
            adaptive.layer_loss(_pred(9, 3, 4), _labels(3, 4))
    other = lightglue.LightGlue({"weights": "synthetic", "loss": {"fn": "focal"}}).eval()
    with pytest.raises(NotImplementedError, match="only 'nll'"):
        other.layer_loss(_pred(9, 3, 4), _labels(3, 4))
    with pytest.raises(NotImplementedError, match="only 'nll'"):
        other.loss({}, {})
    # CPU tensors: the binding's refusal, in either mode (the new entry points do not look at self.training)
    data = {"keypoints0": torch.zeros(1, 3, 2), "keypoints1": torch.zeros(1, 4, 2),
            "descriptors0": torch.zeros(1, 3, 256), "descriptors1": torch.zeros(1, 4, 256)}
    for model in (lg, lightglue.LightGlue({"weights": "synthetic"}).train()):
        with pytest.raises(nat.NativeError, match="no CPU implementation"):
            model.forward_layers(data)
        with pytest.raises(nat.NativeError, match="no CPU implementation"):
            model.layer_loss(_pred(9, 3, 4), _labels(3, 4))
    with pytest.raises(RuntimeError, match="weights are not loaded"):
        lightglue.LightGlue({}).forward_layers(data)


def test_existing_training_refusals_still_hold():
    lg = lightglue.LightGlue({"weights": "synthetic"})
    d = {"keypoints0": torch.zeros(1, 3, 2), "keypoints1": torch.zeros(1, 3, 2), "descriptors0": torch.zeros(1, 3, 256),
         "descriptors1": torch.zeros(1, 3, 256)}
    with pytest.raises(NotImplementedError, match="training"):
        lg.train()(d)
    with pytest.raises(NotImplementedError, match="training"):
        lg.train().loss({}, {})
    with pytest.raises(NotImplementedError, match="re-used weights"):
        losses.NLLLoss({}).forward({}, {}, weights=torch.zeros(1))
    assert set(lightglue.LightGlue.default_conf) == {
        "name", "input_dim", "add_scale_ori", "descriptor_dim", "n_layers", "num_heads", "flash", "mp",
        "depth_confidence", "width_confidence", "filter_threshold", "checkpointed", "weights", "weights_from_version",
        "loss", "fold_out_proj", "graph_max_rows", "matmul_precision", "adaptive_pair_batch"}
    assert lightglue.LightGlue.default_conf["loss"] == {"gamma": 1.0, "fn": "nll", "nll_balancing": 0.5}


def test_pipeline_forwards_to_the_matcher():
    pipe = two_view_pipeline.TwoViewPipeline({"matcher": {"name": "matchers.lightglue", "weights": "synthetic"},
                                              "allow_no_extract": True})
    with pytest.raises(ValueError, match="forward_layers"):
        pipe.layer_loss(_pred(1, 3, 4), _labels(3, 4))
    with pytest.raises(AssertionError, match="Missing key view0"):
        pipe.forward_layers({})


def test_the_layer_scores_header_is_parsed_by_the_same_grammar_and_exported():
    assert sorted(nat.LAYER_SCORES_FUNCTIONS) == ["gfc_lg_layer_pairs", "gfc_lg_layer_pairs_workspace_bytes",
                                                  "gfc_lg_layer_scores", "gfc_lg_layer_scores_workspace_bytes"]
    earlier = (set(nat.FUNCTIONS) | set(nat.VALIDATION_FUNCTIONS) | set(nat.SPARSE_MAP_FUNCTIONS)
               | set(nat.DENSE_WARP_FUNCTIONS) | set(nat.CROSS_ATTENTION_FUNCTIONS))
    assert not set(nat.LAYER_SCORES_FUNCTIONS) & earlier
    with open(nat.LAYER_SCORES_HEADER_PATH) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert funcs == nat.LAYER_SCORES_FUNCTIONS and not structs and not enums and not consts
    ret, params = funcs["gfc_lg_layer_scores"]
    assert ret == "int" and [p for p, _ in params] == [
        "la_layer", "la_final", "logit0", "logit1", "threshold", "B", "M", "N", "out", "correct0", "correct1", "ws",
        "ws_bytes", "stream"]
    lib = nat.lib()
    for name in nat.LAYER_SCORES_FUNCTIONS:
        assert getattr(lib, name).argtypes == nat.LAYER_SCORES_SIGNATURES[name][1]
    # the size query runs on the host: refused shapes give 0, and the layout grows with each of its three edges
    size = lib.gfc_lg_layer_scores_workspace_bytes
    assert size(0, 4, 4) == 0 and size(1, 0, 4) == 0 and size(1, 4, 0) == 0 and size(1, 65536, 4) == 0
    assert size(1, 4, 65536) == 0 and size(65536, 4, 4) == 0 and size(65535, 1, 1) > 0
    assert size(1, 16, 8) == size(1, 1, 8) < size(1, 17, 2048)
    assert size(1, 127, 2048) < size(1, 128, 2048)  # M + 1 = 129 rows: a second row chunk
    # gfc_lg_layer_pairs: one layer's workspace, plus the score array where the whole matcher evaluates sim once (from 8
    # pairs with min(M, N) >= 128 on) -- the sizes gfc_lg_packed_workspace_bytes grows by at the same shapes
    pairs, layer, packed = lib.gfc_lg_layer_pairs_workspace_bytes, lib.gfc_lg_layer_workspace_bytes, \
        lib.gfc_lg_packed_workspace_bytes
    assert pairs(0, 4, 4) == 0 and pairs(1, 0, 4) == 0 and pairs(2, 130, 65) == layer(2 * 195)
    assert pairs(7, 1024, 1024) == layer(7 * 2048) and pairs(8, 1024, 127) == layer(8 * 1151)
    assert pairs(8, 1024, 1024) - layer(8 * 2048) == packed(8, 1024, 1024) - packed(7, 1024, 1024) - (
        packed(7, 1024, 1024) - packed(6, 1024, 1024)) > 0
    # tensors are checked before the call: a CPU tensor never reaches the library
    with pytest.raises(nat.NativeError, match="must be on a 'cuda'"):
        nat.call("gfc_lg_layer_scores", torch.zeros(1, 2, 2), torch.zeros(1, 2, 2), torch.zeros(1, 1),
                 torch.zeros(1, 1), 0.5, 1, 1, 1, torch.zeros(1, 6), None, None, torch.zeros(4096, dtype=torch.uint8),
                 4096)
