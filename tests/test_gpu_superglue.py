"""The SuperGlue matcher on the GPU (csrc/superglue.hip, the BatchNorm + ReLU form of the fused FFN kernel in
csrc/gemm.hip, glue_factory_colon_amd/superglue.py).

Yardsticks: tests/golden/superglue.npz / superglue_1024.npz, which the reference class itself produced
(make_golden_superglue.py), and tests/superglue_reference.py in float64 (pinned to those vectors by
test_superglue_reference_host.py).  Bound on every float: 1e-4 * (1 + |ref|), the project's log-assignment bound; the
reference's own fp32 error on these inputs is 4e-6 of 1 + |ref| (stored in the fixtures), which leaves about 20x for
the MFMA summation order.  For the kernels in isolation the same bound holds by the same argument: a chain of K <= 512
fp32 products rounds to about sqrt(K) * 2^-24 = 1.3e-6 of the magnitudes summed, and the log-domain Sinkhorn update is
non-expansive in the maximum norm, so its rounding errors add up over the iterations (100 x a few 1e-7) instead of
growing.  Matches are compared exactly; matching scores on the rows outside the gap band (superglue_reference.gap_band).
The worst measured ratios go to profiles/superglue_parity.json when GFC_WRITE_PROFILES=1.
"""
import ctypes
import functools
import gc
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import superglue_reference as sgr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import superglue, synthetic, weights  # noqa: E402
from glue_factory_colon_amd.two_view_pipeline import TwoViewPipeline  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-4
THRESHOLD = 0.2
_parity = {}


def ratio(got, ref):
    """max |got - ref| / (1 + |ref|)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (1 + ref.abs())).max())


def record(case, **ratios):
    for k, v in ratios.items():
        print(f"{case}: {k} {v:.3e}" if isinstance(v, float) else f"{case}: {k} {v}")
    _parity.setdefault(case, {}).update(ratios)
    if os.environ.get("GFC_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "superglue_parity.json"), "w") as f:
            json.dump({"what": "largest |kernel - reference| / (1 + |reference|) per test case of tests/test_gpu_superglue.py; "
                               "bound 1e-4; name-seeded weights (weights.superglue_state_dict(0)); integers are counts, "
                               "booleans observations (informational)",
                       "device": torch.cuda.get_device_name(0), "bound": BOUND, "cases": _parity}, f, indent=1)


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """The models cached below (weights packed as many small device tensors) would otherwise stay alive for the rest of
    the session and change where every later test's tensors land in torch's caching allocator."""
    yield
    model.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def model(iters=50):
    return superglue.SuperGlue({"weights": "synthetic", "num_sinkhorn_iterations": iters}).eval().cuda()


@functools.lru_cache(maxsize=None)
def state_dict():
    return weights.superglue_state_dict(0)


@functools.lru_cache(maxsize=None)
def ref64(shape):
    b, m, n, iters = shape
    inp = sgr.make_inputs(0, b, m, n)
    with torch.no_grad():
        return inp, sgr.forward(state_dict(), inp, iters, THRESHOLD, dtype=torch.float64)


def run(shape, taps=False):
    b, m, n, iters = shape
    inp, _ = ref64(shape)
    mod = model(iters)
    with torch.no_grad():
        out = mod._run(*mod._inputs(sgr.as_data(inp, "cuda")), taps=taps)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def scores_ratio(got, ref, la_ref):
    """matching scores outside the gap band: max |got - ref| (absolute: scores live in [0, 1])"""
    rows, cols = sgr.gap_band(la_ref)
    d0 = (got["matching_scores0"].double() - ref["matching_scores0"].double()).abs()[~rows]
    d1 = (got["matching_scores1"].double() - ref["matching_scores1"].double()).abs()[~cols]
    return float(max(d0.max(), d1.max()))


# ------------------------------------------------------------------------------------------ 1. the two small shapes
@pytest.mark.parametrize("shape", sgr.SHAPES[:2], ids=lambda s: f"{s[1]}x{s[2]}")
def test_forward_against_the_reference_vectors(golden, shape):
    b, m, n, _ = shape
    fx, tag = golden("superglue"), f"{m}x{n}"
    out = run(shape, taps=True)
    _, r64 = ref64(shape)
    ref = {k: fx[f"{tag}/{k}"] for k in ("matches0", "matches1", "matching_scores0", "matching_scores1",
                                         "log_assignment", "sinkhorn_cost")}
    idx = fx[f"{tag}/tap_rows"]
    r = {"log_assignment": ratio(out["log_assignment"], ref["log_assignment"]),
         "sinkhorn_cost": ratio(out["sinkhorn_cost"], ref["sinkhorn_cost"]),
         "matching_scores_abs": scores_ratio(out, ref, ref["log_assignment"])}
    for i, name in enumerate(("encoder", "layer0", "layer1", "last")):
        r[f"desc_{name}_sampled_rows"] = ratio(out["desc_taps"][i][idx], fx[f"{tag}/taps"][i])
        r[f"desc_{name}_all_rows_vs_float64"] = ratio(out["desc_taps"][i], r64["taps"][i])
    record(f"forward_{tag}", **r)
    assert torch.equal(out["matches0"], ref["matches0"]) and torch.equal(out["matches1"], ref["matches1"])
    assert out["matches0"].dtype == torch.long and int((out["matches0"] >= 0).sum()) > 0
    for k, v in r.items():
        assert v <= BOUND, (k, v)


# ---------------------------------------------------------------------------------------------- 2. 1024 x 1024, B = 2
def test_forward_1024_against_the_reference_vectors_and_float64(golden):
    shape = sgr.SHAPES[2]
    b, m, n, iters = shape
    assert (b, m, n, iters) == (2, 1024, 1024, 100)
    fx, tag = golden("superglue_1024"), "1024x1024"
    out = run(shape)
    _, r64 = ref64(shape)
    la = out["log_assignment"]
    ref_scores = {k: fx[f"{tag}/{k}"] for k in ("matching_scores0", "matching_scores1")}
    r = {"la_rows": ratio(la[:, fx[f"{tag}/rows"]], fx[f"{tag}/la_rows"]),
         "la_cols": ratio(la[:, :, fx[f"{tag}/cols"]], fx[f"{tag}/la_cols"]),
         "la_row_sum": ratio(la.double().sum(2), fx[f"{tag}/la_row_sum"]),
         "la_row_abs_sum": ratio(la.double().abs().sum(2), fx[f"{tag}/la_row_abs_sum"]),
         "log_assignment_vs_float64": ratio(la, r64["log_assignment"]),
         "sinkhorn_cost_vs_float64": ratio(out["sinkhorn_cost"], r64["sinkhorn_cost"]),
         "matching_scores_abs": scores_ratio(out, ref_scores, r64["log_assignment"])}
    record("forward_1024x1024", **r)
    assert torch.equal(out["matches0"], fx[f"{tag}/matches0"]) and torch.equal(out["matches1"], fx[f"{tag}/matches1"])
    for k, v in r.items():
        assert v <= BOUND, (k, v)


# --------------------------------------------------------------------------------------------------- 3. Sinkhorn alone
def sinkhorn_gpu(cost, bin_score, iters):
    lib = nat.lib()
    b, m, n = cost.shape
    c = cost.float().cuda().contiguous()
    out = torch.full((b, m + 1, n + 1), float("nan"), device="cuda")
    need = lib.gfc_sg_sinkhorn_workspace_bytes(b, m, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    nat.check(lib.gfc_sg_sinkhorn(nat.ptr(c), float(bin_score), b, m, n, iters, nat.ptr(out), nat.ptr(ws), need,
                                  nat.stream_ptr(c.device)), "gfc_sg_sinkhorn")
    torch.cuda.synchronize()
    return out.cpu()


SINKHORN_CASES = [  # (B, M, N, iterations, half-width of the uniform cost)
    (1, 1, 1, 50, 4.0), (1, 1, 1030, 50, 4.0), (3, 301, 258, 1, 4.0), (3, 301, 258, 50, 4.0), (3, 301, 258, 100, 4.0),
    (1, 301, 258, 50, 120.0),  # spans +-120: exp overflows / underflows without the maximum subtraction
    # the edges of the row-block plan (PLAN_EDGES below)
    (1, 2048, 70, 20, 4.0), (2, 21, 4600, 20, 4.0), (1, 3, 20463, 5, 4.0), (2, 16, 40, 20, 4.0),
    (2, 16, 40, 0, 4.0),  # no iteration: u = v = 0, the result is Z - norm
]
SK_LDS_MAX = 160 * 1024


def sk_plan(m, n):
    """sk_plan of csrc/superglue.hip restated: (rows per workgroup, row blocks, rows of the last block, bytes of dynamic
    LDS of the rows kernel), or None where a row of N + 1 floats plus v does not fit."""
    row = (n + 1) * 4
    fit = (SK_LDS_MAX - 32 * 4) // row
    if fit < 2:
        return None
    rb = min(max((m + 64) // 64, 8), 32, fit - 1, m + 1)
    nblk = (m + rb) // rb
    return rb, nblk, m + 1 - (nblk - 1) * rb, (rb + 1) * row + rb * 4


PLAN_EDGES = {  # (M, N): what the shape is in SINKHORN_CASES for
    (2048, 70): (32, 65, 1, 33 * 71 * 4 + 128),  # the cap of 32 rows; the last block is the dustbin row alone
    (21, 4600): (7, 4, 1, 8 * 4601 * 4 + 28),    # 8 rows fit: clipped to 7 beside v; the dustbin row alone again
    (3, 20463): (1, 4, 1, 163716),               # the last N admitted: one row per workgroup, 124 bytes below the limit
    (16, 40): (8, 3, 1, 9 * 41 * 4 + 32),        # the default 8 rows, 17 rows in all
}


def test_sinkhorn_plan_edges_are_what_the_cases_are_for():
    """If sk_plan changes, the shapes above must move with it: this restates it (no kernel runs)."""
    for shape, want in PLAN_EDGES.items():
        assert sk_plan(*shape) == want, (shape, sk_plan(*shape))
        assert shape in {(c[1], c[2]) for c in SINKHORN_CASES}
    assert sk_plan(3, 20463)[3] <= SK_LDS_MAX and sk_plan(3, 20464) is None
    assert sk_plan(8, 4546)[0] == 8 and sk_plan(8, 4547)[0] == 7  # where the LDS clip starts
    lib = nat.lib()
    for (m, n), (rb, nblk, _, _) in PLAN_EDGES.items():  # u | v | partials, each slot rounded up to 256 bytes
        up = lambda x: (x + 255) // 256 * 256  # noqa: E731
        for b in (1, 2):
            assert lib.gfc_sg_sinkhorn_workspace_bytes(b, m, n) == (up(b * (m + 1) * 4) + up(b * (n + 1) * 4)
                                                                   + up(b * nblk * (n + 1) * 8)), (b, m, n)


@pytest.mark.parametrize("case", SINKHORN_CASES, ids=lambda c: "B{}_{}x{}_it{}_w{:g}".format(*c))
def test_sinkhorn_against_float64(case):
    b, m, n, iters, width = case
    g = torch.Generator().manual_seed(1000 * m + n)
    cost = (torch.rand(b, m, n, generator=g) * 2 - 1) * width  # B different matrices: a batch stride error shows
    if width > 100 and m > 1:
        cost[0, 0, 0], cost[0, 1, 1] = 120.0, -120.0
    bin_score = 0.7
    ref = sgr.sinkhorn(cost.float().double(), bin_score, iters)
    got = sinkhorn_gpu(cost, bin_score, iters)
    assert bool(torch.isfinite(got).all())
    r = ratio(got, ref)
    record("sinkhorn_B{}_{}x{}_it{}_w{:g}".format(*case), log_assignment=r)
    assert r <= BOUND, r


def test_sinkhorn_refuses_what_its_plan_cannot_hold():
    """N = 20 464 is the first row that does not fit in LDS beside v: no workspace size, GFC_ERR_UNSUPPORTED, nothing
    launched; the whole matcher names no workspace either.  M + 1 = 65 536 rows exceed the finalize kernel's grid."""
    lib = nat.lib()
    ws = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    for (b, m, n), status in (((1, 3, 20464), "GFC_ERR_UNSUPPORTED"), ((1, 65535, 4), "GFC_ERR_INVALID")):
        cost = torch.zeros((b, m, n), device="cuda")
        out = torch.full((b, m + 1, n + 1), float("nan"), device="cuda")
        got = lib.gfc_sg_sinkhorn(nat.ptr(cost), 0.7, b, m, n, 20, nat.ptr(out), nat.ptr(ws), ws.numel(),
                                  nat.stream_ptr(cost.device))
        torch.cuda.synchronize()
        assert nat.STATUS[got] == status, (b, m, n, got)
        assert bool(torch.isnan(out).all()) and bool((ws == 0xA5).all())
    assert lib.gfc_sg_sinkhorn_workspace_bytes(1, 3, 20464) == 0 and lib.gfc_sg_workspace_bytes(1, 3, 20464) == 0
    assert lib.gfc_sg_sinkhorn_workspace_bytes(1, 3, 20463) > 0 and lib.gfc_sg_workspace_bytes(1, 3, 20463) > 0


def test_sinkhorn_of_a_matrix_does_not_depend_on_its_batch():
    """The row-block plan is a function of (M, N) alone and no kernel sums across matrices: matrix i of a batched call
    equals the call on that matrix alone, bit for bit."""
    b, m, n, iters = 3, 301, 258, 50
    cost = (torch.rand(b, m, n, generator=torch.Generator().manual_seed(1000 * m + n)) * 2 - 1) * 4.0
    batched = sinkhorn_gpu(cost, 0.7, iters)
    assert bool(torch.isfinite(batched).all())
    for i in range(b):
        assert torch.equal(batched[i:i + 1], sinkhorn_gpu(cost[i:i + 1], 0.7, iters)), i


# ------------------------------------------------------------------------------ 4. the MLP and the encoder alone
def _mlp_weights(g):
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    w0, b0 = r(512, 512) / 512 ** 0.5 * 2 ** 0.5, r(512) * 0.1
    # BatchNorm statistics far from (0, 1)
    bn = {"weight": torch.rand(512, generator=g) * 1.5 + 0.3, "bias": r(512) * 0.5, "running_mean": r(512) * 2 + 1,
          "running_var": torch.rand(512, generator=g) * 8 + 0.05}
    w1, b1 = r(256, 512) / 512 ** 0.5, r(256) * 0.1
    return w0, b0, bn, w1, b1


@pytest.mark.parametrize("rows", (1, 127, 300))
@pytest.mark.parametrize("alias", (False, True), ids=("separate", "residual_is_Y"))
def test_mlp_against_float64(rows, alias):
    lib = nat.lib()
    g = torch.Generator().manual_seed(rows)
    w0, b0, bn, w1, b1 = _mlp_weights(g)
    x, msg, res = (torch.randn(rows, 256, generator=g) for _ in range(3))
    d = lambda t: t.double()  # noqa: E731
    h = torch.cat([x, msg], 1).double() @ d(w0).t() + d(b0)
    h = torch.relu((h - d(bn["running_mean"])) / torch.sqrt(d(bn["running_var"]) + 1e-5) * d(bn["weight"]) + d(bn["bias"]))
    ref = d(res) + h @ d(w1).t() + d(b1)
    scale = d(bn["weight"]) / torch.sqrt(d(bn["running_var"]) + 1e-5)
    shift = d(bn["bias"]) - d(bn["running_mean"]) * scale
    dev = [t.float().cuda().contiguous() for t in (x, msg, w0, b0, scale, shift, w1, b1, res)]
    xg, mg, w0g, b0g, scg, shg, w1g, b1g, rg = dev
    guard = torch.full((rows + 2, 256), 7.0, device="cuda")  # a row before and after Y: nothing may be written there
    y = guard[1:rows + 1]
    if alias:
        y.copy_(rg)
        rg = y
    nat.check(lib.gfc_sg_mlp(nat.ptr(xg), 256, nat.ptr(mg), 256, nat.ptr(w0g), nat.ptr(b0g), nat.ptr(scg), nat.ptr(shg),
                             nat.ptr(w1g), nat.ptr(b1g), nat.ptr(rg), ctypes.c_void_p(y.data_ptr()), 256, rows,
                             nat.stream_ptr(xg.device)), "gfc_sg_mlp")
    torch.cuda.synchronize()
    assert bool((guard[0] == 7.0).all()) and bool((guard[-1] == 7.0).all())
    r = ratio(y, ref)
    record(f"mlp_rows{rows}_{'alias' if alias else 'separate'}", y=r)
    assert r <= BOUND, r


@pytest.mark.parametrize("rows_per_image", (1, 127, 300))
@pytest.mark.parametrize("use_scores", (True, False), ids=("scores", "no_scores"))
def test_keypoint_encoder_against_float64(rows_per_image, use_scores):
    lib = nat.lib()
    n, b = rows_per_image, 2
    sd = dict(weights.superglue_state_dict(5, n_layers=0, use_scores=use_scores))
    g = torch.Generator().manual_seed(n)
    for i in (1, 4, 7, 10):  # BatchNorm statistics far from (0, 1)
        c = sd[f"kenc.encoder.{i}.weight"].numel()
        sd[f"kenc.encoder.{i}.running_mean"] = torch.randn(c, generator=g) * 2 + 1
        sd[f"kenc.encoder.{i}.running_var"] = torch.rand(c, generator=g) * 8 + 0.05
    mod = superglue.SuperGlue({"weights": None, "GNN_layers": [], "use_scores": use_scores}).eval()
    mod.load_state_dict(sd, strict=True)
    p = mod.cuda().ensure_packed(torch.device("cuda", 0))[0]
    sizes = torch.tensor([[640.0, 480.0], [300.0, 500.0]])  # two images of different sizes: the per-image table
    kp = torch.rand(b, n, 2, generator=g) * sizes[:, None]
    sc = torch.rand(b, n, generator=g) if use_scores else None
    desc = torch.randn(b, n, 256, generator=g)
    ref = desc.double() + sgr.keypoint_encoder({k: v.double() for k, v in sd.items() if v.is_floating_point()},
                                               sgr.normalize_keypoints(kp.double(), sizes),
                                               None if sc is None else sc.double())
    guard = torch.full((b * n + 2, 256), 7.0, device="cuda")
    y = guard[1:b * n + 1]
    y.copy_(desc.reshape(-1, 256))
    need = lib.gfc_sg_keypoint_encoder_workspace_bytes(b * n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    kpg, szg = kp.cuda().contiguous(), sizes.cuda().contiguous()
    scg = None if sc is None else sc.cuda().contiguous()
    nat.check(lib.gfc_sg_keypoint_encoder(ctypes.byref(p), nat.ptr(kpg), nat.ptr(scg), nat.ptr(szg), b, n,
                                          ctypes.c_void_p(y.data_ptr()), nat.ptr(ws), need, nat.stream_ptr(kpg.device)),
              "gfc_sg_keypoint_encoder")
    torch.cuda.synchronize()
    assert bool((guard[0] == 7.0).all()) and bool((guard[-1] == 7.0).all())
    r = ratio(y, ref.reshape(-1, 256))
    record(f"encoder_rows{b * n}_{'scores' if use_scores else 'no_scores'}", desc=r)
    assert r <= BOUND, r


# ------------------------------------------------------------------------------------ 5. heads that differ grossly
def test_one_loud_head_rules_out_a_head_order_mix_up():
    """The query projection rows of ONE head (reference channels c with c % 4 == 1) are scaled by 50: that head's
    soft-max turns peaky while the others stay flat, so head-major and interleaved channel orders give grossly
    different messages."""
    names = ["self", "cross"] * 2
    sd = dict(weights.superglue_state_dict(0, n_layers=len(names)))
    for i in range(len(names)):
        for part in ("weight", "bias"):
            t = sd[f"gnn.layers.{i}.attn.proj.0.{part}"].clone()
            t[1::4] *= 50
            sd[f"gnn.layers.{i}.attn.proj.0.{part}"] = t
    mod = superglue.SuperGlue({"weights": None, "GNN_layers": names}).eval()
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda()
    inp = sgr.make_inputs(3, 2, 65, 130)
    with torch.no_grad():
        ref = sgr.forward(sd, inp, 50, THRESHOLD, layer_names=names, dtype=torch.float64)
        # the soft-max of the loud head is far from uniform (otherwise this test would prove nothing)
        x = ref["taps"][0][:65].double()[None]
        q = sgr._lin({k: v.double() for k, v in sd.items() if v.is_floating_point()}, "gnn.layers.0.attn.proj.0", x)
        k = sgr._lin({k: v.double() for k, v in sd.items() if v.is_floating_point()}, "gnn.layers.0.attn.proj.1", x)
        logits = torch.einsum("bndh,bmdh->bhnm", q.reshape(1, 65, 64, 4), k.reshape(1, 65, 64, 4)) / 8
        peak = torch.softmax(logits, -1).amax(-1).mean(-1)[0]
        assert peak[1] > 4 * peak[0] and peak[1] > 0.2, peak
        out = mod._run(*mod._inputs(sgr.as_data(inp, "cuda")), taps=True)
    torch.cuda.synchronize()
    r = {"log_assignment": ratio(out["log_assignment"], ref["log_assignment"]),
         "desc_layer0": ratio(out["desc_taps"][1], ref["taps"][1]), "desc_last": ratio(out["desc_taps"][3], ref["taps"][3])}
    record("loud_head", **r)
    for k_, v in r.items():
        assert v <= BOUND, (k_, v)


# ------------------------------------------------------------------------------------------------ 6. forward_pairs
def att_partition(b, m, n, nk):
    """(key split, key tiles per split) of the attention launch of gfc_sg_forward for B pairs of (m, n) points, keys of
    a side with nk points: the integer arithmetic of gfc_attention / gfc_att_split / sg_ws restated."""
    heads, problems, max_nq = 4, 2 * b, max(m, n)
    wgs = lambda aq: (max_nq + aq - 1) // aq * heads * problems  # noqa: E731
    tiles = (nk + 63) // 64
    if wgs(256) >= 1024 or wgs(128) >= 256:  # 256 queries per workgroup / enough workgroups of 128: no split
        return 1, tiles
    split = min((511 + wgs(128)) // wgs(128), 8)
    rows = b * (m + n)
    scratch = rows * heads * 8 * 66 * 4 if rows <= 8192 else 0  # sg_ws: the full split of B (M + N) query slots
    while split > 1 and scratch < problems * max_nq * heads * split * 66 * 4:
        split -= 1
    return split, (tiles + split - 1) // split


def test_forward_pairs_equals_single_pair_calls():
    """Bit equality holds at these shapes because both runs take the same key partition in the attention (asserted
    first) and the same GEMM tile; it is not a contract (test_a_pair_in_a_batch_of_six_... states that one)."""
    for nk in (65, 130):
        assert att_partition(1, 65, 130, nk) == att_partition(2, 65, 130, nk) == (6, 1)
    mod = model(50)
    shapes = [(65, 130), (40, 17), (65, 130), (12, 0)]  # three distinct (m, n), one pair empty on one side
    datas = []
    for i, (m, n) in enumerate(shapes):
        d = sgr.as_data(sgr.make_inputs(10 + i, 1, m, max(n, 1)), "cuda")
        if n == 0:
            for k in ("keypoints1", "descriptors1", "keypoint_scores1"):
                d[k] = d[k][:, :0]
        datas.append(d)
    with torch.no_grad():
        single = [mod(d) for d in datas]
        batched = mod.forward_pairs(datas)
    torch.cuda.synchronize()
    assert len(batched) == len(single)
    for s, b in zip(single, batched):
        assert sorted(s) == sorted(b)
        for k in s:
            assert s[k].dtype == b[k].dtype and torch.equal(s[k], b[k]), k
    assert sorted(single[3]) == ["matches0", "matches1", "matching_scores0", "matching_scores1"]
    assert single[3]["matches0"].dtype == torch.int and int((single[0]["matches0"] >= 0).sum()) > 0


def test_a_pair_in_a_batch_of_six_against_float64_and_its_single_call():
    """What a pair's result may depend on its batch for.  Six pairs of 300 + 300 points run the attention with a 4-way
    key split of two 64-key tiles each, one such pair alone with an 8-way split of one tile (asserted from the
    dispatch arithmetic first: if that changes, this test compares a kernel with itself and must be given another
    shape).  The partial soft-maxes are then merged in another order, so the floats may differ in their last bits.  The
    contract: every run within the bound of float64; integers identical to float64's and to each other outside the
    near-ties (gap_band of the float64 log-assignment); matching scores within 1e-4.  Sinkhorn alone is bit-identical
    across batches (test_sinkhorn_of_a_matrix_does_not_depend_on_its_batch)."""
    shape = (6, 300, 300, 50)
    b, m, n, iters = shape
    assert att_partition(1, m, n, 300) == (8, 1) and att_partition(b, m, n, 300) == (4, 2)
    inp, r64 = ref64(shape)
    rows, cols = sgr.gap_band(r64["log_assignment"])
    # condition on the inputs: near-ties are rare (the restatement alone: 0 rows and 1 column of 3600)
    assert int(rows.sum()) <= 0.01 * rows.numel() and int(cols.sum()) <= 0.01 * cols.numel()
    mod = model(iters)

    def gpu(sub):
        with torch.no_grad():
            out = mod._run(*mod._inputs(sgr.as_data(sub, "cuda")))
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    batched = gpu(inp)
    single = [gpu({k: v[i:i + 1] for k, v in inp.items()}) for i in range(b)]
    single = {k: torch.cat([s[k] for s in single], 0) for k in batched}
    r = {}
    for name, out in (("batched", batched), ("single", single)):
        r[f"{name}_log_assignment"] = ratio(out["log_assignment"], r64["log_assignment"])
        r[f"{name}_sinkhorn_cost"] = ratio(out["sinkhorn_cost"], r64["sinkhorn_cost"])
        r[f"{name}_matching_scores_abs"] = scores_ratio(out, r64, r64["log_assignment"])
    d0 = (batched["matching_scores0"].double() - single["matching_scores0"].double()).abs()
    d1 = (batched["matching_scores1"].double() - single["matching_scores1"].double()).abs()
    r["batched_vs_single_matching_scores_abs"] = float(max(d0.max(), d1.max()))
    r["batched_vs_single_log_assignment"] = ratio(batched["log_assignment"], single["log_assignment"])
    record("pair_in_batch_of_six_300x300", **r, band_rows=int(rows.sum()), band_cols=int(cols.sum()),
           batched_log_assignment_bit_equal_to_single=bool(torch.equal(batched["log_assignment"],
                                                                       single["log_assignment"])))
    for name, out in (("batched", batched), ("single", single)):
        assert out["matches0"].dtype == torch.long and int((out["matches0"] >= 0).sum()) > 0
        assert torch.equal(out["matches0"][~rows], r64["matches0"][~rows]), name
        assert torch.equal(out["matches1"][~cols], r64["matches1"][~cols]), name
    assert torch.equal(batched["matches0"][~rows], single["matches0"][~rows])
    assert torch.equal(batched["matches1"][~cols], single["matches1"][~cols])
    for k in ("batched_log_assignment", "batched_sinkhorn_cost", "single_log_assignment", "single_sinkhorn_cost",
              "batched_vs_single_matching_scores_abs"):
        assert r[k] <= BOUND, (k, r[k])


# --------------------------------------------------------------------------------------------- 7. TwoViewPipeline
def test_two_view_pipeline_superpoint_superglue():
    k, h, w = 256, 160, 208
    pipe = TwoViewPipeline({
        "extractor": {"name": "gluefactory_nonfree.superpoint", "weights": "synthetic", "max_num_keypoints": k,
                      "detection_threshold": 0.0, "nms_radius": 3},
        "matcher": {"name": "gluefactory_nonfree.superglue", "weights": "synthetic"},
    }).eval().cuda()
    assert isinstance(pipe.matcher, superglue.SuperGlue)
    datas = []
    for seed in (41, 42):
        v0, v1 = synthetic.synthetic_pairs(1, h, w, seed=seed)
        size = torch.tensor([[float(w), float(h)]]).cuda()
        datas.append({"view0": {"image": v0.cuda(), "image_size": size}, "view1": {"image": v1.cuda(), "image_size": size}})
    with torch.no_grad():
        single = [pipe(d) for d in datas]
        batched = pipe.forward_pairs(datas)
    torch.cuda.synchronize()
    pred = single[0]
    m, n = pred["keypoints0"].shape[1], pred["keypoints1"].shape[1]
    assert m > 0 and n > 0
    want = {"keypoints0": (1, m, 2), "keypoints1": (1, n, 2), "keypoint_scores0": (1, m), "keypoint_scores1": (1, n),
            "descriptors0": (1, m, 256), "descriptors1": (1, n, 256), "matches0": (1, m), "matches1": (1, n),
            "matching_scores0": (1, m), "matching_scores1": (1, n), "log_assignment": (1, m + 1, n + 1),
            "sinkhorn_cost": (1, m, n)}
    for key, shape in want.items():
        assert key in pred and tuple(pred[key].shape) == shape, (key, pred.get(key, torch.empty(0)).shape)
    assert pred["matches0"].dtype == torch.long
    timing = ("time_ms", "memory_mb")
    for s, b in zip(single, batched):
        for key in want:
            assert torch.equal(s[key], b[key]), key
        assert {x for x in s if not x.endswith(timing)} == {x for x in b if not x.endswith(timing)}
