"""The batched adaptive depth / width path: `gfc_lg_adaptive_step` alone on planted decisions, and
`LightGlue.forward_pairs(adaptive_pair_batch=True)` against the oracle's match_adaptive loop pair by pair.

Everything a comparison excuses is decided on the oracle alone (tests/adaptive_pairs_reference.py,
tests/test_adaptive_pairs_host.py) before a GPU output is looked at.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import adaptive_pairs_reference as apr  # noqa: E402
import adaptive_reference as ar  # noqa: E402
from glue_factory_colon_amd import _native as nat  # noqa: E402

DEV = "cuda"
TOL = 1e-4
LIVE, STOPPED, EMPTIED = nat.GFC_LG_ADAPTIVE_LIVE, nat.GFC_LG_ADAPTIVE_STOPPED, nat.GFC_LG_ADAPTIVE_EMPTIED
SENTINEL = -7


def st():
    return nat.stream_ptr(torch.device(DEV))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ============================================================================================ B. the step alone
def _f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def _run_step(x, cos, sin, ind, seg, pairs, prune_off, prune, tw, tb, mw, mb, thr, keep_thr, depth, do_stop, do_prune,
              max_n=None):
    """One gfc_lg_adaptive_step on host tensors; every output starts as NaN / SENTINEL.  Returns CPU tensors.  `max_n`
    defaults to the longest segment."""
    lib = nat.lib()
    B, rows = pairs.shape[0], x.shape[0]
    keep = [t.to(DEV).contiguous() for t in (x, cos, sin, ind, seg, pairs, prune_off, prune, tw, tb, mw, mb)]
    dx, dcos, dsin, dind, dseg, dpairs, doff, dprune, dtw, dtb, dmw, dmb = keep
    p = nat.LgParams()
    p.n_layers = 9
    layer = 3
    p.token_w[layer], p.token_b[layer] = dtw.data_ptr(), dtb.data_ptr()
    p.matchability_w[layer], p.matchability_b[layer] = dmw.data_ptr(), dmb.data_ptr()
    out = {"x": torch.full_like(dx, float("nan")), "cos": torch.full_like(dcos, float("nan")),
           "sin": torch.full_like(dsin, float("nan")), "ind": torch.full_like(dind, SENTINEL),
           "self_p": torch.full((2 * B, 4), SENTINEL, dtype=torch.int32, device=DEV),
           "cross_p": torch.full((2 * B, 4), SENTINEL, dtype=torch.int32, device=DEV),
           "seg": torch.full((2 * B, 2), SENTINEL, dtype=torch.int32, device=DEV),
           "pairs": torch.full((B, 2), SENTINEL, dtype=torch.int32, device=DEV),
           "report": torch.full((B, 4), SENTINEL, dtype=torch.int32, device=DEV)}
    nbytes = lib.gfc_lg_adaptive_step_workspace_bytes(B, rows)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    max_n = int(seg[:, 1].max()) if max_n is None else max_n
    args = [ctypes.byref(p), layer, nat.ptr(dx), nat.ptr(dcos), nat.ptr(dsin), nat.ptr(dind), rows, nat.ptr(dseg),
            nat.ptr(dpairs), nat.ptr(doff), doff.shape[0], B, max_n, thr, keep_thr, depth, int(do_stop), int(do_prune),
            nat.ptr(out["x"]), nat.ptr(out["cos"]), nat.ptr(out["sin"]), nat.ptr(out["ind"]), nat.ptr(dprune),
            dprune.numel(), nat.ptr(out["self_p"]), nat.ptr(out["cross_p"]), nat.ptr(out["seg"]), nat.ptr(out["pairs"]),
            nat.ptr(out["report"]), nat.ptr(ws), ws.numel(), st()]
    nat.check(lib.gfc_lg_adaptive_step(*args), "gfc_lg_adaptive_step")
    torch.cuda.synchronize()
    # bad arguments are status codes, and launch nothing: no criterion, the input as the output, a short workspace, a
    # layer without a decision
    bad = list(args); bad[16] = bad[17] = 0
    assert lib.gfc_lg_adaptive_step(*bad) == 1
    bad = list(args); bad[18] = args[2]
    assert lib.gfc_lg_adaptive_step(*bad) == 1
    bad = list(args); bad[30] = nbytes - 1
    assert lib.gfc_lg_adaptive_step(*bad) == 2
    bad = list(args); bad[1] = 8
    assert lib.gfc_lg_adaptive_step(*bad) == 1
    bad = list(args); bad[11] = nat.GFC_LG_MAX_RAGGED_PAIRS + 1
    assert lib.gfc_lg_adaptive_step(*bad) == 1
    assert lib.gfc_lg_adaptive_step_workspace_bytes(nat.GFC_LG_MAX_RAGGED_PAIRS + 1, rows) == 0
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res["prune"] = dprune.cpu()
    return res


def _expected(x, cos, sin, ind, seg, pairs, prune_off, prune, low, keepc, depth, do_stop, do_prune):
    """The documented result of the step from per-row decisions `low` (tok < thr) and `keepc` (the keep mask)."""
    B = pairs.shape[0]
    info = []
    prune = prune.clone()
    for b in range(B):
        (r0, n0), (r1, n1) = seg[2 * b].tolist(), seg[2 * b + 1].tolist()
        denom, slot = pairs[b].tolist()
        cnt, stop = 0, False
        if do_stop:
            cnt = int(low[r0:r0 + n0].sum() + low[r1:r1 + n1].sum())
            ratio = 1.0 - torch.tensor(float(cnt), dtype=torch.float32) / denom  # the torch expression of check_if_stop
            stop = ratio.item() > depth
        sides = []
        for s, (r, n) in enumerate(((r0, n0), (r1, n1))):
            k = torch.ones(n, dtype=torch.bool) if (stop or not do_prune) else keepc[r:r + n]
            rows = r + k.nonzero().flatten()
            sides.append(rows)
            if do_prune and not stop:
                prune[prune_off[slot, s] + ind[rows].long()] += 1
        cm, cn = len(sides[0]), len(sides[1])
        state = STOPPED if stop else (EMPTIED if cm == 0 or cn == 0 else LIVE)
        info.append((state, cm, cn, cnt, sides, (denom, slot)))
    order = [b for b in range(B) if info[b][0] == LIVE] + [b for b in range(B) if info[b][0] != LIVE]
    n_live = sum(1 for q in info if q[0] == LIVE)
    gather, seg_o, pairs_o, self_p, cross_p = [], [], [], [], []
    r = 0
    for pos, b in enumerate(order):
        state, cm, cn, _, sides, pr = info[b]
        gather += [sides[0], sides[1]]
        seg_o += [[r, cm], [r + cm, cn]]
        pairs_o.append(list(pr))
        if pos < n_live:
            self_p += [[r, cm, r, cm], [r + cm, cn, r + cm, cn]]
            cross_p += [[r, cm, r + cm, cn], [r + cm, cn, r, cm]]
        r += cm + cn
    gather = torch.cat(gather)
    return {"report": torch.tensor([q[:4] for q in info], dtype=torch.int32), "rows": gather, "x": x[gather],
            "cos": cos[gather], "sin": sin[gather], "ind": ind[gather], "prune": prune,
            "seg": torch.tensor(seg_o, dtype=torch.int32), "pairs": torch.tensor(pairs_o, dtype=torch.int32),
            "self_p": torch.tensor(self_p, dtype=torch.int32).reshape(-1, 4),
            "cross_p": torch.tensor(cross_p, dtype=torch.int32).reshape(-1, 4), "n_live": n_live}


def _check_step(got, want, tag):
    n = want["rows"].numel()
    assert torch.equal(got["report"], want["report"]), (tag, got["report"].tolist(), want["report"].tolist())
    for k in ("x", "cos", "sin", "ind"):
        assert torch.equal(got[k][:n], want[k]), (tag, k)
    assert bool(got["x"][n:].isnan().all()) and bool(got["cos"][n:].isnan().all()) and bool(got["sin"][n:].isnan().all()), tag
    assert bool((got["ind"][n:] == SENTINEL).all()), tag
    assert torch.equal(got["prune"], want["prune"]), tag
    assert torch.equal(got["seg"], want["seg"]) and torch.equal(got["pairs"], want["pairs"]), tag
    nl = 2 * want["n_live"]
    for k in ("self_p", "cross_p"):
        assert torch.equal(got[k][:nl], want[k]), (tag, k)
        assert bool((got[k][nl:] == SENTINEL).all()), (tag, k)


def _layout(shapes, extra, g):
    """Rows pair after pair (side 0, side 1); un-pruned lists `extra` points longer than the live ones, `ind` a random
    injection into them; slots in an order of their own."""
    B = len(shapes)
    slots = torch.randperm(B + 3, generator=g)[:B].tolist()
    seg, pairs, ind = [], [], []
    un = {}
    r = 0
    for b, (m, n) in enumerate(shapes):
        seg += [[r, m], [r + m, n]]
        pairs.append([m + n + 2 * extra, slots[b]])
        for s, k in enumerate((m, n)):
            un[(slots[b], s)] = k + extra
            ind.append(torch.randperm(k + extra, generator=g)[:k].int())
        r += m + n
    prune_off = torch.zeros((B + 3, 2), dtype=torch.int32)
    o = 5  # counters of unused slots and a few leading elements stay as they are
    for slot in range(B + 3):
        for s in range(2):
            prune_off[slot, s] = o
            o += un.get((slot, s), 4)
    prune = torch.randint(1, 6, (o + 5,), generator=g, dtype=torch.int32)
    return torch.tensor(seg, dtype=torch.int32), torch.tensor(pairs, dtype=torch.int32), torch.cat(ind), prune_off, prune, r


def _planted(mode, max_n=None):
    """gfc_lg_adaptive_step with planted logits: token_w = e0, matchability_w = e1, zero biases, so tok = sigmoid(x[:,0])
    and sc = sigmoid(x[:,1]); the logits lie at least 0.05 from logit(thr) and logit(keep_thr), so a float64 reference
    decides every row.  Five pairs in one call: (65, 64) and (300, 257) mixed, (63, 129) with every row kept, (256, 256)
    planted to stop (10 low rows of 526 points), (1, 40) whose side 0 is pruned to nothing.  report, the re-packed rows
    (a copy: torch.equal), ind, the prune counters and the next layer's tables exact; the tail of every output
    untouched."""
    do_stop, do_prune = mode != "prune_only", mode != "stop_only"
    g = gen(20240 + len(mode))
    shapes = ((65, 64), (300, 257), (63, 129), (256, 256), (1, 40))
    seg, pairs, ind, prune_off, prune, rows = _layout(shapes, 7, g)
    thr, keep_thr, depth = _f32(0.9), _f32(1 - 0.95), 0.95
    lt, lk = math.log(thr / (1 - thr)), math.log(keep_thr / (1 - keep_thr))

    def away(n, positive):
        """n logits offsets at least 0.05 from 0 on the wanted side"""
        return (0.05 + 3 * torch.rand(n, generator=g)) * (positive * 2.0 - 1.0)

    x = torch.randn((rows, 256), generator=g)
    high_tok = torch.rand(rows, generator=g) < 0.6   # tok > thr: confident
    high_sc = torch.rand(rows, generator=g) < 0.5    # sc > keep_thr: matchable
    (a0, n0), (a1, n1) = seg[4].tolist(), seg[5].tolist()      # (63, 129): every row kept
    high_sc[a0:a1 + n1] = True
    (a0, n0), (a1, n1) = seg[6].tolist(), seg[7].tolist()      # (256, 256): 10 low rows of 526 -> ratio 0.981 > 0.95
    high_tok[a0:a1 + n1] = True
    high_tok[a0 + 3:a0 + 8] = False
    high_tok[a1 + 250:a1 + 255] = False
    a0 = seg[8, 0].item()                                      # (1, 40): the one row of side 0 confident and unmatchable
    high_tok[a0], high_sc[a0] = True, False
    x[:, 0] = lt + away(rows, high_tok.float())
    x[:, 1] = lk + away(rows, high_sc.float())
    cos, sin = torch.randn((rows, 64), generator=g), torch.randn((rows, 64), generator=g)
    tok, sc = torch.sigmoid(x[:, 0].double()), torch.sigmoid(x[:, 1].double())
    assert float((tok - thr).abs().min()) > 1e-3 and float((sc - keep_thr).abs().min()) > 1e-3
    low = tok < thr
    keepc = sc > keep_thr
    if do_stop:
        keepc = keepc | (tok <= thr)
    e0 = torch.zeros(256); e0[0] = 1
    e1 = torch.zeros(256); e1[1] = 1
    zero = torch.zeros(1)
    want = _expected(x, cos, sin, ind, seg, pairs, prune_off, prune, low, keepc, depth, do_stop, do_prune)
    states = want["report"][:, 0].tolist()
    assert states == {"both": [LIVE, LIVE, LIVE, STOPPED, EMPTIED], "prune_only": [LIVE, LIVE, LIVE, LIVE, EMPTIED],
                      "stop_only": [LIVE, LIVE, LIVE, STOPPED, LIVE]}[mode], states
    if do_prune:
        assert want["report"][2, 1:3].tolist() == [63, 129] and want["report"][4, 1].item() == 0
        assert 0 < want["report"][0, 1] < 65 and 0 < want["report"][1, 2] < 257
    got = _run_step(x, cos, sin, ind, seg, pairs, prune_off, prune, e0, zero, e1, zero, thr, keep_thr, depth, do_stop,
                    do_prune, max_n)
    _check_step(got, want, (mode, max_n))


@pytest.mark.parametrize("mode", ("both", "prune_only", "stop_only"))
def test_step_planted(mode):
    _planted(mode)


@pytest.mark.parametrize("mode", ("both", "stop_only"))
def test_step_planted_understated_max_n(mode):
    """max_n only sizes the launch: with 256 for segments of 300 and 257 rows the workgroups of the re-pack take a second
    256-row chunk each (re-counting the kept rows in front of it when pruning, copying straight when not), and the
    result is the same."""
    _planted(mode, max_n=256)


def test_step_decides_on_the_bits_of_rowdot():
    """Random rows and heads: the step's decisions are the ones taken on gfc_lg_rowdot(apply_sigmoid = 1)'s output,
    bit for bit -- thresholds placed inside the values' range so that hundreds of rows sit on either side."""
    lib = nat.lib()
    g = gen(515)
    shapes = ((200, 131), (77, 260))
    seg, pairs, ind, prune_off, prune, rows = _layout(shapes, 0, g)
    x = torch.randn((rows, 256), generator=g)
    cos, sin = torch.randn((rows, 64), generator=g), torch.randn((rows, 64), generator=g)
    tw, mw = torch.randn(256, generator=g) / 16, torch.randn(256, generator=g) / 16
    tb, mb = torch.tensor([0.1]), torch.tensor([-0.2])
    dx = x.to(DEV)
    vals = []
    keep = []
    for w, b in ((tw, tb), (mw, mb)):
        dw, db = w.to(DEV), b.to(DEV)
        keep += [dw, db]
        out = torch.full((rows,), float("nan"), device=DEV)
        nat.check(lib.gfc_lg_rowdot(nat.ptr(dx), 256, rows, nat.ptr(dw), nat.ptr(db), 1, nat.ptr(out), st()), "rowdot")
        vals.append(out.cpu())
    tok, sc = vals
    # thresholds that ARE values of the outputs: the comparisons < / <= / > meet equality on the GPU's own bits
    thr, keep_thr = tok.sort().values[rows // 2].item(), sc.sort().values[rows // 3].item()
    low = tok < thr
    keepc = (sc > keep_thr) | (tok <= thr)
    assert 100 < int(low.sum()) < rows - 100 and 100 < int(keepc.sum()) < rows - 50
    for depth in (0.3, 0.6):  # ratio ~ 0.5: both pairs stop, neither stops
        want = _expected(x, cos, sin, ind, seg, pairs, prune_off, prune, low, keepc, depth, True, True)
        got = _run_step(x, cos, sin, ind, seg, pairs, prune_off, prune, tw, tb, mw, mb, thr, keep_thr, depth, True, True)
        _check_step(got, want, depth)


# ============================================================================================ C. forward_pairs
def _model(depth, width, pz, **kw):
    from glue_factory_colon_amd import lightglue

    m = lightglue.LightGlue({"filter_threshold": ar.FILTER_THRESHOLD, "depth_confidence": depth,
                             "width_confidence": width, **kw}).eval()
    m.load_state_dict(ar.state_dict(pz), strict=False)
    return m.to(DEV)


def _items():
    out = []
    for d in apr.inputs():
        size = d["size"].to(DEV)
        out.append({"keypoints0": d["keypoints0"].to(DEV), "keypoints1": d["keypoints1"].to(DEV),
                    "descriptors0": d["descriptors0"].to(DEV), "descriptors1": d["descriptors1"].to(DEV),
                    "view0": {"image_size": size}, "view1": {"image_size": size}})
    return out


def relerr(a, ref):
    ref = ref.double().cpu()
    return ((a.double().cpu() - ref).abs() / (1 + ref.abs())).max().item() if ref.numel() else 0.0


def maxerr(a, b):
    assert tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    return (a.double().cpu() - b.double().cpu()).abs().max().item() if a.numel() else 0.0


_EXCUSED = []   # (config, pair) that took the band exit, over the whole module
MAX_EXCUSED = 2  # of the 12 (pair, config) cases


def _first_divergence(pred, final, layers, bands, prune):
    """None when the GPU pair took the oracle's decisions (prune0/1 and stop_layer equal).  Otherwise the first decision
    layer at which they part, asserted to be a pruning layer at which EVERY point that parts lies in the oracle's band;
    returns a description with the oracle's margins."""
    s_g, s_r = int(pred["stop_layer"]), final["stop_layer"]
    if not prune:
        assert s_g == s_r, ("stop layer differs without pruning", s_g, s_r)
        return None
    pg = [pred["prune0"][0].cpu().long(), pred["prune1"][0].cpu().long()]
    pr = [final["prune0"][0].long(), final["prune1"][0].long()]
    if s_g == s_r and all(torch.equal(a, b) for a, b in zip(pg, pr)):
        return None
    first = [torch.minimum(a, b) - 1 for a, b in zip(pg, pr)]  # per point: the decision layer where the two part
    diff = [a != b for a, b in zip(pg, pr)]
    L = min(int(f[d].min()) for f, d in zip(first, diff) if bool(d.any()))
    # a stop decision that differs with nothing excused before it is a failure: the host test keeps every ratio two
    # points or more from depth_confidence
    assert L < min(s_g, s_r) - 1, ("the stop decision differs first", L, s_g, s_r)
    rec, bd = layers[L], bands[L]
    thr = ar.thresholds().tolist()
    desc = []
    for side in (0, 1):
        pts = (diff[side] & (first[side] == L)).nonzero().flatten()
        unsure = torch.zeros(pg[side].numel(), dtype=torch.bool)
        unsure[rec[f"ind{side}"]] = bd[f"unsure{side}"]
        assert bool(unsure[pts].all()), ("differs outside the band", L, side, pts[~unsure[pts]].tolist()[:10])
        row_of = {int(p): i for i, p in enumerate(rec[f"ind{side}"].tolist())}
        for p in pts.tolist():
            i = row_of[p]
            tok = rec[f"tok{side}"]
            desc.append((L, side, p, float(rec[f"sc{side}"][i]), None if tok is None else float(tok[i]) - thr[L]))
    return desc


def _compare_pair(cfg, p, pred, run, shape, prune):
    """One GPU pair against its oracle trace `run` = (layers, final, bands): the comparison the docstring of
    test_forward_pairs_adaptive_batched describes.  A pair that took the band exit is recorded in _EXCUSED."""
    layers, final, bands = run
    m, n = shape
    parted = _first_divergence(pred, final, layers, bands, prune)
    if parted is not None:
        _EXCUSED.append((cfg, p))
        print(f"config {cfg} pair {p}: parts from the oracle inside the band, (layer, side, point, matchability, "
              f"token confidence - threshold): {parted}; stop layer {int(pred['stop_layer'])} / {final['stop_layer']}")
        return
    assert int(pred["stop_layer"]) == final["stop_layer"]
    assert pred["log_assignment"].shape == final["log_assignment"].shape
    assert pred["ref_descriptors0"].shape == final["ref_descriptors0"].shape
    assert pred["ref_descriptors1"].shape == final["ref_descriptors1"].shape
    assert pred["matches0"].shape == (1, m) and pred["matches1"].shape == (1, n)
    e_la = relerr(pred["log_assignment"], final["log_assignment"])
    e_s = max(maxerr(pred["matching_scores0"], final["matching_scores0"]),
              maxerr(pred["matching_scores1"], final["matching_scores1"]))
    e_x = max(maxerr(pred["ref_descriptors0"], final["ref_descriptors0"]),
              maxerr(pred["ref_descriptors1"], final["ref_descriptors1"]))
    print(f"config {cfg} pair {p}: stop {final['stop_layer']}, survivors {tuple(final['log_assignment'].shape[1:])}, "
          f"log_assignment rel {e_la:.2e}, scores {e_s:.2e}, rows {e_x:.2e}")
    assert e_la < 1e-4, (p, e_la)
    assert e_s < TOL and e_x < TOL, (p, e_s, e_x)
    skip0, skip1 = ar.near_tie_rows(final["log_assignment"])
    full0, full1 = torch.zeros(m, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    if prune:
        full0[final["ind0"]], full1[final["ind1"]] = skip0, skip1
    else:
        full0, full1 = skip0, skip1
    for side, (got, ref, skip) in enumerate(((pred["matches0"], final["matches0"], full0),
                                             (pred["matches1"], final["matches1"], full1))):
        bad = (got.cpu().flatten() != ref.flatten()) & ~skip
        assert not bool(bad.any()), (p, side, bad.nonzero().flatten().tolist()[:10])


@pytest.mark.parametrize("cfg", range(len(apr.CONFIGS)))
def test_forward_pairs_adaptive_batched(cfg):
    """forward_pairs(adaptive_pair_batch=True) on the four shared pairs against the oracle trace of each pair.  A pair
    whose prune0/1 and stop_layer equal the oracle's is compared in full: log_assignment's shape, log_assignment within
    1e-4 (1 + |x|), matching scores within 1e-4, matches equal outside the oracle's near-tie rows.  A pair that differs
    must part from the oracle first at a pruning layer where every parting point lies in the oracle's band (bands(),
    fixed before any GPU output); at most MAX_EXCUSED of the 12 (pair, config) cases may.  With the key off the same
    call returns what the single-pair call returns, bit for bit."""
    depth, width, pz = apr.CONFIGS[cfg]
    runs = apr.traced(depth, width, pz)
    items = _items()
    model = _model(depth, width, pz, adaptive_pair_batch=True)
    off = _model(depth, width, pz)
    assert off.conf.adaptive_pair_batch is False
    with torch.no_grad():
        preds = model.forward_pairs(items)
        single = [off(d) for d in items]
        preds_off = off.forward_pairs(items)
    for a, b, c in zip(single, preds_off, preds):
        assert set(a) == set(b) == set(c), (sorted(a), sorted(c))
        for k in a:
            assert torch.equal(a[k], b[k]), k
            assert c[k].dtype == a[k].dtype and c[k].dim() == a[k].dim(), k
    for p, (pred, run) in enumerate(zip(preds, runs)):
        _compare_pair(cfg, p, pred, run, apr.SHAPES[p], width > 0)
    assert len(_EXCUSED) <= MAX_EXCUSED, _EXCUSED


# ============================================================================================ D. fp16, chunking
def _fp16_batched_matches_sequential(a_all, b_all):
    """Two fp16 launch sets on the same pairs: stop layers equal, matches agreeing on 99 % of the points, floats within
    2e-2 (1 + |x|)."""
    for i, (a, b) in enumerate(zip(a_all, b_all)):
        print(f"fp16 pair {i}: stop {int(a['stop_layer'])} / {int(b['stop_layer'])}, log_assignment "
              f"{tuple(a['log_assignment'].shape)} / {tuple(b['log_assignment'].shape)}")
        assert int(a["stop_layer"]) == int(b["stop_layer"]), i
        for k in ("matches0", "matches1"):
            agree = float((a[k] == b[k]).double().mean())
            assert agree >= 0.99, (i, k, agree)
        for k in ("matching_scores0", "matching_scores1", "log_assignment"):
            assert a[k].shape == b[k].shape, (i, k, a[k].shape, b[k].shape)
            assert ((a[k] - b[k]).abs() <= 2e-2 * (1 + a[k].abs())).all(), (i, k)


def test_adaptive_batched_fp16_and_chunking():
    """matmul_precision fp16: the batched path against the sequential fp16 path on the shared pairs -- stop layers equal,
    matches agreeing on 99 % of the points and floats within 2e-2 (1 + |x|), the tolerance
    tests/test_gpu_lightglue_fp16.py allows between two fp16 launch sets.  Then 130 tiny pairs (8 + 8 points), fp32,
    across the 128-pair chunk: every pair's result at its own position."""
    depth, width, pz = apr.CONFIGS[0]
    items = _items()
    seq = _model(depth, width, pz, matmul_precision="fp16")
    bat = _model(depth, width, pz, matmul_precision="fp16", adaptive_pair_batch=True)
    with torch.no_grad():
        a_all = [seq(d) for d in items]
        b_all = bat.forward_pairs(items)
    _fp16_batched_matches_sequential(a_all, b_all)

    src = apr.inputs()
    tiny = []
    for k in range(130):
        d = src[k % 4]
        o0, o1 = (3 * k) % 50, (5 * k) % 50
        size = d["size"].to(DEV)
        tiny.append({"keypoints0": d["keypoints0"][:, o0:o0 + 8].contiguous().to(DEV),
                     "keypoints1": d["keypoints1"][:, o1:o1 + 8].contiguous().to(DEV),
                     "descriptors0": d["descriptors0"][:, o0:o0 + 8].contiguous().to(DEV),
                     "descriptors1": d["descriptors1"][:, o1:o1 + 8].contiguous().to(DEV),
                     "view0": {"image_size": size}, "view1": {"image_size": size}})
    seq = _model(depth, width, pz)
    bat = _model(depth, width, pz, adaptive_pair_batch=True)
    with torch.no_grad():
        a_all = [seq(d) for d in tiny]
        b_all = bat.forward_pairs(tiny)
    assert len(b_all) == 130
    stops = set()
    for i, (a, b) in enumerate(zip(a_all, b_all)):
        stops.add(int(a["stop_layer"]))
        assert int(a["stop_layer"]) == int(b["stop_layer"]), i
        assert torch.equal(a["prune0"], b["prune0"]) and torch.equal(a["prune1"], b["prune1"]), i
        assert a["log_assignment"].shape == b["log_assignment"].shape, i
        assert relerr(b["log_assignment"], a["log_assignment"]) < 1e-4, i
        assert maxerr(b["matching_scores0"], a["matching_scores0"]) < TOL, i
        assert maxerr(b["matching_scores1"], a["matching_scores1"]) < TOL, i
        for k in ("matches0", "matches1"):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (i, k)
    agree = torch.cat([(a[k] == b[k]).flatten() for a, b in zip(a_all, b_all) for k in ("matches0", "matches1")])
    assert float(agree.double().mean()) >= 0.99
    print(f"130 tiny pairs: stop layers seen {sorted(stops)}")


# ============================================================================================ E. input_proj, scale / ori
def _items128():
    out = []
    for d in apr.inputs128():
        size = d["size"].to(DEV)
        out.append({"keypoints0": d["keypoints0"].to(DEV), "keypoints1": d["keypoints1"].to(DEV),
                    "descriptors0": d["descriptors0"].to(DEV), "descriptors1": d["descriptors1"].to(DEV),
                    "view0": {"image_size": size}, "view1": {"image_size": size}})
    return out


def _model128(**kw):
    from glue_factory_colon_amd import lightglue

    depth, width = apr.CONFIG_128
    m = lightglue.LightGlue({"filter_threshold": ar.FILTER_THRESHOLD, "input_dim": 128, "depth_confidence": depth,
                             "width_confidence": width, **kw}).eval()
    m.load_state_dict(apr.state_dict128(), strict=False)
    return m.to(DEV)


def test_adaptive_input_dim_128():
    """input_dim 128 (the input projection in front of both adaptive paths), fp32: the pairs (65, 64) and (190, 333) with
    128-d descriptors, `model(d)` pair by pair and forward_pairs(adaptive_pair_batch=True), each against the oracle's
    match_adaptive trace with the comparisons and the cap of test_forward_pairs_adaptive_batched.  On the oracle both
    pairs prune at four layers, stop after the fifth and have no band row (tests/test_adaptive_fold_host.py)."""
    runs = apr.traced128()
    items = _items128()
    with torch.no_grad():
        seq = _model128()
        single = [seq(d) for d in items]
        batched = _model128(adaptive_pair_batch=True).forward_pairs(items)
    for tag, preds in (("128-d single", single), ("128-d batched", batched)):
        for p, (pred, run) in enumerate(zip(preds, runs)):
            _compare_pair(tag, p, pred, run, apr.SHAPES[apr.PAIRS_128[p]], True)
    assert len(_EXCUSED) <= MAX_EXCUSED, _EXCUSED


def test_adaptive_input_dim_128_fp16():
    """The same two 128-d pairs with matmul_precision fp16 (input projection on the fp16 MFMA): the batched path against
    the sequential one, as the first half of test_adaptive_batched_fp16_and_chunking."""
    items = _items128()
    with torch.no_grad():
        seq = _model128(matmul_precision="fp16")
        a_all = [seq(d) for d in items]
        b_all = _model128(matmul_precision="fp16", adaptive_pair_batch=True).forward_pairs(items)
    _fp16_batched_matches_sequential(a_all, b_all)


def test_adaptive_add_scale_ori():
    """add_scale_ori through both adaptive paths.  The oracle's match_adaptive takes no scales / orientations, so the
    configuration prunes and stops nothing (depth_confidence -1, keep threshold 1e-3 against matchabilities above 0.7:
    tests/test_adaptive_fold_host.py) and oracle.lightglue.match(scale_ori0=, scale_ori1=) is the reference: matches
    equal outside near-tie rows, scores and rows within the tolerances of test_lightglue_add_scale_ori_golden, every
    point through all layers."""
    from glue_factory_colon_amd import lightglue

    d, sd, ref = apr.scale_ori_case()
    m, n = apr.SCALE_ORI_SHAPE
    data = {k: d[k].to(DEV) for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "scales0", "scales1",
                                      "oris0", "oris1")}
    data["view0"] = data["view1"] = {"image_size": d["size"].to(DEV)}
    conf = {"weights": None, "filter_threshold": ar.FILTER_THRESHOLD, "add_scale_ori": True, "depth_confidence": -1,
            "width_confidence": apr.SCALE_ORI_WIDTH}
    skip = ar.near_tie_rows(ref["log_assignment"])
    for tag, extra in (("single", {}), ("batched", {"adaptive_pair_batch": True})):
        model = lightglue.LightGlue({**conf, **extra}).eval()
        model.load_state_dict(sd, strict=False)
        model = model.to(DEV)
        with torch.no_grad():
            out = model(data) if tag == "single" else model.forward_pairs([data])[0]
        e_s = max(maxerr(out["matching_scores0"], ref["matching_scores0"]),
                  maxerr(out["matching_scores1"], ref["matching_scores1"]))
        e_x = max(maxerr(out["ref_descriptors0"], ref["ref_descriptors0"]),
                  maxerr(out["ref_descriptors1"], ref["ref_descriptors1"]))
        print(f"add_scale_ori {tag}: scores {e_s:.2e}, rows {e_x:.2e}")
        for side, cnt in ((0, m), (1, n)):
            bad = (out[f"matches{side}"].cpu().flatten() != ref[f"matches{side}"].flatten()) & ~skip[side]
            assert not bool(bad.any()), (tag, side, bad.nonzero().flatten().tolist()[:10])
            assert out[f"prune{side}"].shape == (1, cnt) and bool((out[f"prune{side}"] == model.conf.n_layers).all()), tag
        assert e_s < TOL and e_x < 1e-4, (tag, e_s, e_x)
        assert out["log_assignment"].shape == (1, m + 1, n + 1)
        assert int(out["stop_layer"]) == model.conf.n_layers, tag
