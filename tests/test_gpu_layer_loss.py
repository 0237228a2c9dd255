"""`LightGlue.forward_layers` / `layer_loss`, their pipeline forms and `validate --layer_report` on the GPU, against the
vectors the reference produced in training mode (tests/golden/layer_loss*.npz, made by make_layer_loss_golden.py on
the inputs of tests/layer_loss_cases.py) and against `forward` / `loss` on the same inputs.

Bounds: 1e-4 (1 + |ref|), the suite's bound for log assignments, for every layer's log assignment, the sampled
descriptor rows, the token logits and every loss value (each a mean of entries that are themselves within that bound);
1e-4 relative for the descriptors' sums of squares.  The targets correct0 / correct1 and every count are equal: the
fixture has no top-2 gap below 1e-3 (asserted by its maker and by the host test).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endopatches_reference as er  # noqa: E402
import layer_loss_cases as lc  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import lightglue, synthetic  # noqa: E402
from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = {"a": "layer_loss", "b": "layer_loss_b1"}
GAMMAS = {"05": 0.5, "0": 0.0, "1": 1.0}
FINAL_KEYS = ("last", "assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable", "row_norm")


def close(got, ref, what, rel=1e-4):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    err = (got - ref).abs() / (1 + ref.abs())
    print(f"{what}: worst error / (1 + |ref|) = {float(err.max()):.2e}")
    assert bool((err <= rel).all()), (what, float(err.max()))


def model(**conf):
    return lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.0, **conf}).eval().cuda()


def inputs(case):
    c = lambda k: case[k].cuda()  # noqa: E731
    return {"keypoints0": c("keypoints0"), "keypoints1": c("keypoints1"), "descriptors0": c("descriptors0"),
            "descriptors1": c("descriptors1"), "view0": {"image_size": c("size")}, "view1": {"image_size": c("size")}}


def labels(case, assignment=True):
    out = {"gt_matches0": case["gt_matches0"].cuda(), "gt_matches1": case["gt_matches1"].cuda()}
    if assignment and case["gt_assignment"] is not None:
        out["gt_assignment"] = case["gt_assignment"].cuda()
    return out


@pytest.fixture(scope="module", params=["a", "b"])
def fx(request):
    """A fixture batch, its regenerated inputs and ONE forward_layers prediction shared by the tests (never changed)."""
    name = request.param
    z = np.load(os.path.join(ROOT, "tests", "golden", FILES[name] + ".npz"))
    rows = np.load(os.path.join(ROOT, "tests", "golden", "layer_loss_rows.npz"))
    case = lc.make_case(name, int(z["seed"]))
    assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"]))
    lg = model()
    with torch.no_grad():
        pred = lg.forward_layers(inputs(case))
    torch.cuda.synchronize()
    return name, z, rows, case, lg, pred


def head(lg, pred, layer):
    """Layer `layer`'s own log assignment through the head path (gfc_lg_assign), and its token logits."""
    ref0, ref1 = pred["ref_descriptors0"], pred["ref_descriptors1"]
    b, _, m, d = ref0.shape
    n = ref1.shape[2]
    dev = ref0.device
    params = lg.ensure_packed(dev)[0]
    x = torch.cat([ref0[:, layer].reshape(b * m, d), ref1[:, layer].reshape(b * n, d)], 0).contiguous()
    la = torch.empty((b, m + 1, n + 1), device=dev)
    m0, m1 = torch.empty((b, m), dtype=torch.long, device=dev), torch.empty((b, n), dtype=torch.long, device=dev)
    s0, s1 = torch.empty((b, m), device=dev), torch.empty((b, n), device=dev)
    ws = torch.empty(nat.call("gfc_lg_assign_workspace_bytes", b, m, n), dtype=torch.uint8, device=dev)
    nat.call("gfc_lg_assign", ctypes.byref(params), layer, x, x[b * m:], b, m, n, 0.0, m0, m1, s0, s1, la, ws, ws.numel())
    logits = None
    if layer < lg.conf.n_layers - 1:
        logits = torch.empty((b * (m + n),), device=dev)
        nat.call("gfc_lg_rowdot", x, d, b * (m + n), params.token_w[layer], params.token_b[layer], 0, logits)
    return la, m0, logits


def test_forward_layers_on_the_fixture(fx):
    name, z, rows, case, lg, pred = fx
    b, m = case["keypoints0"].shape[:2]
    n = case["keypoints1"].shape[1]
    nl = lc.N_LAYERS
    assert pred["ref_descriptors0"].shape == (b, nl, m, 256) and pred["ref_descriptors1"].shape == (b, nl, n, 256)
    assert set(pred) == {"matches0", "matches1", "matching_scores0", "matching_scores1", "ref_descriptors0",
                         "ref_descriptors1", "log_assignment", "prune0", "prune1"}
    # permuted views of ONE stack buffer [L, B*M + B*N, 256], no transposing copy
    r0, r1 = pred["ref_descriptors0"], pred["ref_descriptors1"]
    assert r0.untyped_storage().data_ptr() == r1.untyped_storage().data_ptr()
    assert r0.stride() == (m * 256, b * (m + n) * 256, 256, 1) and r1.stride() == (n * 256, b * (m + n) * 256, 256, 1)
    i0, i1 = lc.sample_rows(name)
    flat0 = r0.permute(1, 0, 2, 3).reshape(nl, b * m, 256)
    flat1 = r1.permute(1, 0, 2, 3).reshape(nl, b * n, 256)
    close(flat0[:, i0.cuda()], rows[f"{name}_ref0_rows"], "sampled rows of side 0")
    close(flat1[:, i1.cuda()], rows[f"{name}_ref1_rows"], "sampled rows of side 1")
    for side, flat in (("0", flat0), ("1", flat1)):
        got, ref = (flat.double() ** 2).sum((1, 2)).cpu(), torch.from_numpy(rows[f"{name}_ref{side}_sumsq"])
        rel = ((got - ref).abs() / ref).max()
        print(f"sum of squares, side {side}: worst relative error {float(rel):.2e}")
        assert float(rel) <= 1e-4
    dev = r0.device
    ws = torch.empty(nat.call("gfc_lg_layer_scores_workspace_bytes", b, m, n), dtype=torch.uint8, device=dev)
    final = pred["log_assignment"]
    for i in range(nl):
        la, m0, logits = head(lg, pred, i)
        close(la, z["la"][i], f"log assignment of layer {i}")
        assert torch.equal(m0.cpu(), torch.from_numpy(z["layer_matches0"][i])), i
        if i == nl - 1:
            assert torch.equal(la, final)
            continue
        close(logits[:b * m].view(b, m), z["logit0"][i], f"token logits 0 of layer {i}")
        close(logits[b * m:].view(b, n), z["logit1"][i], f"token logits 1 of layer {i}")
        out = torch.empty((b, 6), device=dev)
        c0 = torch.empty((b, m), dtype=torch.uint8, device=dev)
        c1 = torch.empty((b, n), dtype=torch.uint8, device=dev)
        nat.call("gfc_lg_layer_scores", la, final, logits, logits[b * m:], float(z["thresholds"][i]), b, m, n, out, c0, c1,
                 ws, ws.numel())
        assert torch.equal(c0.bool().cpu(), torch.from_numpy(z["correct0"][i])), i
        assert torch.equal(c1.bool().cpu(), torch.from_numpy(z["correct1"][i])), i
        assert torch.equal(out[:, 4].long().cpu(), torch.from_numpy(z["conf0"][i])), i
        assert torch.equal(out[:, 5].long().cpu(), torch.from_numpy(z["conf1"][i])), i


@pytest.mark.parametrize("tag", list(GAMMAS))
def test_layer_loss_on_the_fixture(fx, tag):
    name, z, _, case, lg, pred = fx
    b, m = case["keypoints0"].shape[:2]
    n = case["keypoints1"].shape[1]
    lg_g = model(loss={"gamma": GAMMAS[tag]})
    want = dict(zip([str(k) for k in z["loss_keys"]], z[f"losses_gamma{tag}"]))
    variants = [True, False] if case["gt_assignment"] is not None else [False]
    for assignment in variants:  # without gt_assignment the labels name the same positives
        with torch.no_grad():
            losses, report = lg_g.layer_loss(pred, labels(case, assignment))
        torch.cuda.synchronize()
        assert set(losses) == set(want)
        for k, ref in want.items():
            assert losses[k].shape == (b,)
            if k in ("num_matchable", "num_unmatchable"):
                assert torch.equal(losses[k].double().cpu(), torch.from_numpy(ref)), k
            else:
                close(losses[k], ref, f"{name} gamma {GAMMAS[tag]} assignment {assignment}: {k}")
        close(report["layer_nll"].t(), z["nll"], "per-layer nll")
        assert report["layer_nll"].shape == (b, lc.N_LAYERS) and report["layer_agree"].shape == (b, lc.N_LAYERS - 1)
        agree = (z["correct0"].sum(-1) + z["correct1"].sum(-1)).T  # [B, L-1] counts
        assert torch.equal((report["layer_agree"] * (m + n)).round().long().cpu(), torch.from_numpy(agree))
        conf = (z["conf0"] + z["conf1"]).T
        assert torch.equal((report["layer_ratio_confident"] * (m + n)).round().long().cpu(), torch.from_numpy(conf))
        # the final-layer keys are what `loss` returns on the same prediction, bit for bit
        with torch.no_grad():
            plain, metrics = lg_g.loss({**pred, "ref_descriptors0": pred["ref_descriptors0"][:, -1:],
                                        "ref_descriptors1": pred["ref_descriptors1"][:, -1:]}, labels(case, assignment))
        for k in FINAL_KEYS:
            assert torch.equal(losses[k], plain[k]), k
        for k, v in metrics.items():
            assert torch.equal(report[k], v), k
        assert torch.equal(report["layer_recall"][:, -1], metrics["match_recall"])
        assert torch.equal(report["layer_precision"][:, -1], metrics["match_precision"])


def test_layer_loss_reads_the_thresholds_once(fx):
    """The confidence thresholds reach the host with the packed weights, once: a later call makes no read of its own (the
    validation pass counts one device-to-host read per group), and a move of the weights renews them."""
    _, _, _, case, _, pred = fx
    lg = model()
    with torch.no_grad():
        lg.layer_loss(pred, labels(case))
        first = lg._thresholds_host
        lg.layer_loss(pred, labels(case))
    assert lg._thresholds_host is first and first[1] == lg.confidence_thresholds.tolist()
    lg.load_state_dict(lg.state_dict())
    with torch.no_grad():
        lg.layer_loss(pred, labels(case))
    assert lg._thresholds_host is not first and lg._thresholds_host[1] == first[1]


def pair(b, m, n, seed, din=256):
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor([[640.0, 480.0]]).expand(b, 2)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)  # noqa: E731
    d = {"keypoints0": torch.rand((b, m, 2), generator=g) * 479, "keypoints1": torch.rand((b, n, 2), generator=g) * 479,
         "descriptors0": unit(torch.randn((b, m, din), generator=g)),
         "descriptors1": unit(torch.randn((b, n, din), generator=g))}
    d = {k: v.cuda() for k, v in d.items()}
    return {**d, "view0": {"image_size": size.cuda()}, "view1": {"image_size": size.cuda()}}


@pytest.mark.parametrize("shape", [(2, 130, 65), (2, 1024, 1024), (8, 300, 257), (33, 1024, 1024)],
                         ids=["130x65", "2x1024x1024", "8x300x257", "33x1024x1024"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_forward_layers_against_forward(shape, precision):
    """Same launches at the same sizes: matches, scores, the log assignment and the last layer's descriptors are
    `forward`'s, bit for bit (fp16: the contract asks for the matches and the last layer).  From 8 pairs with min(M, N)
    >= 128 on `forward` evaluates the cross attention's scores once, in chunks of pairs (one chunk at 8 x 300 + 257, 32
    + 1 pairs at 33 x 1024 + 1024), and `forward_layers` follows it through gfc_lg_layer_pairs."""
    lg = model(matmul_precision=precision, filter_threshold=0.1)
    data = pair(*shape, seed=3)
    with torch.no_grad():
        a, f = lg.forward_layers(data), lg(data)
    torch.cuda.synchronize()
    assert f["ref_descriptors0"].shape[1] == 1 and a["ref_descriptors0"].shape[1] == 9
    assert torch.equal(a["matches0"], f["matches0"]) and torch.equal(a["matches1"], f["matches1"])
    assert torch.equal(a["ref_descriptors0"][:, -1], f["ref_descriptors0"][:, 0])
    assert torch.equal(a["ref_descriptors1"][:, -1], f["ref_descriptors1"][:, 0])
    for k in ("matching_scores0", "matching_scores1", "log_assignment", "prune0", "prune1"):
        assert torch.equal(a[k], f[k]), k
    # every layer differs from the one before: the stack holds L different outputs
    r = a["ref_descriptors0"]
    assert all(not torch.equal(r[:, i], r[:, i + 1]) for i in range(8))


def test_forward_layers_input_forms():
    """input_dim != 256 with scales and orientations, and an empty side."""
    lg = model(input_dim=128, add_scale_ori=True)
    data = pair(1, 70, 33, seed=4, din=128)
    g = torch.Generator().manual_seed(8)
    for s, k in (("0", 70), ("1", 33)):
        data["scales" + s] = (1 + torch.rand((1, k), generator=g)).cuda()
        data["oris" + s] = (6.28 * torch.rand((1, k), generator=g)).cuda()
    with torch.no_grad():
        a, f = lg.forward_layers(data), lg(data)
    for k in ("matches0", "matches1", "matching_scores0", "log_assignment"):
        assert torch.equal(a[k], f[k]), k
    assert torch.equal(a["ref_descriptors1"][:, -1], f["ref_descriptors1"][:, 0])
    empty = {**data, "keypoints1": data["keypoints1"][:, :0], "descriptors1": data["descriptors1"][:, :0],
             "scales1": data["scales1"][:, :0], "oris1": data["oris1"][:, :0]}
    with torch.no_grad():
        a, f = lg.forward_layers(empty), lg(empty)
    assert a["ref_descriptors0"].shape == (1, 9, 70, 256) and a["ref_descriptors1"].shape == (1, 9, 0, 256)
    for k in ("matches0", "matches1", "matching_scores0", "log_assignment", "prune0"):
        assert torch.equal(a[k], f[k]), k
    with pytest.raises(ValueError, match="without key points"):
        lg.layer_loss(a, {"gt_matches0": torch.zeros(1, 70).long().cuda(), "gt_matches1": torch.zeros(1, 0).long().cuda()})


PIPE_CONF = {"extractor": {"name": "extractors.superpoint_open", "weights": "synthetic", "max_num_keypoints": 256,
                           "detection_threshold": 0.0, "nms_radius": 3},
             "matcher": {"name": "matchers.lightglue", "weights": "synthetic", "filter_threshold": 0.1},
             "ground_truth": {"name": "matchers.homography_matcher", "th_positive": 3, "th_negative": 5}}


def test_pipeline_layer_loss_with_a_homography_ground_truth():
    v0, v1 = synthetic.synthetic_pairs(2, 240, 320, seed=5)  # view 1 is view 0 shifted by (16, 8)
    H = torch.tensor([[1.0, 0, 16], [0, 1, 8], [0, 0, 1]]).repeat(2, 1, 1).cuda()
    size = torch.tensor([[320.0, 240.0]] * 2).cuda()
    data = {"view0": {"image": v0.cuda(), "image_size": size}, "view1": {"image": v1.cuda(), "image_size": size},
            "H_0to1": H}
    pipe = TwoViewPipeline(PIPE_CONF).eval().cuda()
    with torch.no_grad():
        pred = pipe.forward_layers(data)
        losses, report = pipe.layer_loss(pred, data)
        plain_pred = pipe(data)
        plain, metrics = pipe.loss(plain_pred, data)
    torch.cuda.synchronize()
    assert pred["ref_descriptors0"].shape[:2] == (2, 9) and torch.equal(pred["matches0"], plain_pred["matches0"])
    for k in FINAL_KEYS:
        assert torch.equal(losses[k], plain[k]), k
    for k, v in metrics.items():
        assert torch.equal(report[k], v), k
    assert bool(torch.isfinite(losses["total"]).all()) and bool((losses["confidence"] > 0).all())
    for k in ("layer_agree", "layer_ratio_confident", "layer_recall", "layer_precision"):
        assert bool(((report[k] >= 0) & (report[k] <= 1)).all()), k


def test_validate_layer_report_on_a_generated_directory(tmp_path, capsys):
    """`layer_report` on the generated `homographies` tree of the existing validation test: the per-layer table, the two
    extra losses and the extra TSV columns, still one device-to-host read per group.  Without the flag the run makes the
    calls it made before (forward_pairs with the matcher, `loss`; never `forward_layers`), and its summary and TSV are
    byte for byte those of a pipeline built without the argument."""
    import shutil

    from glue_factory_colon_amd import validate
    from glue_factory_colon_amd.registry import get_dataset

    names = er.make_tree(tmp_path, per_sequence=3, hw=(120, 160))
    for n in names:
        shutil.copy(tmp_path / "frames" / "test" / n, tmp_path / "frames" / "val" / n)
    conf = {"data_dir": "frames", "photometric": {"name": "identity"}, "reseed": True, "val_size": 5,
            "homography": {"difficulty": 0.5, "max_angle": 30, "patch_shape": [96, 72]}}
    ds = get_dataset("homographies")(conf, tmp_path, split="val")
    model_conf = {"extractor": {"max_num_keypoints": 128}}

    def run(tsv, **kw):
        vp = validate.ValidationPipeline(model_conf, pair_batch=4, **kw)
        calls = []
        for obj, name in ((vp.model, "loss"), (vp.model, "layer_loss"), (vp.model.matcher, "forward_layers"),
                          (vp.model.matcher, "forward_pairs")):
            inner = getattr(obj, name)
            setattr(obj, name, lambda *a, _f=inner, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
        res = vp.run(ds.feeder(batch=4, num_workers=0), log_metrics=tmp_path / tsv, step=7)
        validate._print(res)
        return res, capsys.readouterr().out, (tmp_path / tsv).read_bytes(), calls, vp.reads

    plain, out_plain, tsv_plain, calls_plain, reads_plain = run("plain.tsv")
    again, out_again, tsv_again, _, _ = run("again.tsv", layer_report=False)
    assert out_plain == out_again and tsv_plain == tsv_again
    assert set(calls_plain) == {"loss", "forward_pairs"} and "layer" not in out_plain
    assert tsv_plain.decode().splitlines()[0] == validate.TSV_HEADER.rstrip("\n")
    deep, out_deep, tsv_deep, calls_deep, reads_deep = run("deep.tsv", layer_report=True)
    assert set(calls_deep) == {"layer_loss", "forward_layers"} and reads_deep == reads_plain
    with pytest.raises(ValueError, match="other columns"):  # wider rows never go under the plain header
        run("plain.tsv", layer_report=True)
    assert (tmp_path / "plain.tsv").read_bytes() == tsv_plain
    assert calls_deep.count("layer_loss") == reads_deep  # one call and one read per (M, N) group
    for k, v in plain.items():  # everything the plain run reports is there: the same kernels on the same launches
        assert abs(deep[k] - v) <= 1e-5 * max(1.0, abs(v)) or (v != v and deep[k] != deep[k]), (k, deep[k], v)
    assert deep["loss/total_deep"] > deep["loss/confidence"] > 0
    assert {k for k in deep if not k.startswith("layer/")} == set(plain) | {"loss/confidence", "loss/total_deep"}
    table = [ln for ln in out_deep.splitlines() if ln.startswith("layer ")]
    assert len(table) == 1 + 9 and table[0].split() == ["layer", "index", "nll", "recall", "precision", "agree",
                                                        "token_bce", "ratio_confident"]
    assert table[-1].split()[-3:] == ["-", "-", "-"] and "-" not in table[1].split()  # the last layer has no token head
    assert abs(float(table[-1].split()[2]) - deep["loss/assignment_nll"]) <= 1e-6
    lines_plain, lines_deep = tsv_plain.decode().splitlines(), tsv_deep.decode().splitlines()
    assert len(lines_deep) == len(lines_plain) == 6 and lines_deep[0].startswith(lines_plain[0] + "\t")
    extra = lines_deep[0].split("\t")[8:]
    assert extra[:2] == ["confidence", "total_deep"] and len(extra) == 2 + 9 * 3 + 8 * 3
    for lp, ld in zip(lines_plain[1:], lines_deep[1:]):
        assert ld.split("\t")[:4] == lp.split("\t")[:4] and len(ld.split("\t")) == 8 + len(extra)
        for a, b in zip(ld.split("\t")[4:8], lp.split("\t")[4:8]):
            assert abs(float(a) - float(b)) <= 1e-5
