"""Host helper (test infrastructure): the oracle's `match_adaptive` loop with its intermediates kept.

`oracle.lightglue.match_adaptive` returns only the final outputs.  The teacher-forced GPU test of the adaptive
depth / width path needs what the loop saw at every layer: the rows after the layer, the token confidences and
matchabilities, the keep sets and the stop ratio.  `trace()` runs the same loop from the same oracle functions
(`self_block`, `cross_block`, `_linear`, `positional_encoding`, `match_assignment`, `filter_matches`; no arithmetic of
its own) and records them.  Its final outputs equal `match_adaptive`'s bit for bit
(tests/test_adaptive_reference_host.py asserts it).

`inputs()` builds the evaluation-size case the tests share and `bands()` derives, from the oracle alone, which points
lie too close to a decision threshold for an fp32 implementation with another summation order to be held to the
oracle's decision.
"""
import functools

import numpy as np
import torch

from oracle import lightglue as olg
from oracle import superpoint as osp

DELTA = 1e-4            # a decision is compared only where the oracle's value is farther than this from its threshold
FILTER_THRESHOLD = 0.1
# (depth_confidence, width_confidence, prune_z of weights.lightglue_adaptive_state_dict)
CONFIGS = ((0.95, 0.95, 1.5), (-1.0, 0.95, 0.84), (0.95, 0.99, 0.84))


def thresholds(n_layers=9):
    """confidence_thresholds buffer (lightglue.py:555-558), as match_adaptive builds it."""
    thr = [float(np.clip(0.8 + 0.1 * np.exp(-4.0 * i / n_layers), 0, 1)) for i in range(n_layers)]
    return torch.tensor(thr, dtype=torch.float32)


@functools.lru_cache(maxsize=1)
def inputs():
    """One synthetic VGA pair, 1024 key points per image from the oracle's SuperPoint (open variant)."""
    from glue_factory_colon_amd import synthetic, weights

    v0, v1 = synthetic.synthetic_pairs(1, 480, 640, seed=1234)
    sd = weights.superpoint_open_state_dict(0)
    out = {}
    for side, img in ((0, v0), (1, v1)):
        f = osp.extract(sd, img, variant="open", nms_radius=3, max_num_keypoints=1024, detection_threshold=0.0)
        assert len(f["keypoints"][0]) == 1024
        out[f"keypoints{side}"] = f["keypoints"][0][None].contiguous()
        out[f"descriptors{side}"] = f["descriptors"][0][None].contiguous()
    out["size"] = torch.tensor([[640.0, 480.0]])
    return out


def state_dict(prune_z):
    from glue_factory_colon_amd import weights

    return weights.lightglue_adaptive_state_dict(0, prune_z=prune_z)


def trace(sd, kpts0, kpts1, desc0, desc1, size0, size1, depth_confidence=-1.0, width_confidence=-1.0, n_layers=9,
          heads=4, filter_threshold=0.0):
    """match_adaptive (oracle/lightglue.py) statement by statement, keeping per layer
    {x0, x1 (rows after the layer, before pruning), tok0, tok1, sc0, sc1 (None when unused), ratio, stop,
     keep0, keep1 (indices into the layer's rows, None when nothing is pruned), m, n (rows of the layer)}.
    Returns (layers, final outputs as match_adaptive, e0, e1 = the un-pruned rotary tables [2,1,1,N,64])."""
    with torch.no_grad():
        b, m, _ = kpts0.shape
        n = kpts1.shape[1]
        assert b == 1
        thr = thresholds(n_layers)
        x0, x1 = desc0.contiguous(), desc1.contiguous()
        if "input_proj.weight" in sd:
            x0, x1 = olg._linear(sd, "input_proj", x0), olg._linear(sd, "input_proj", x1)
        e0 = olg.positional_encoding(sd["posenc.Wr.weight"], olg.normalize_keypoints(kpts0, size0))
        e1 = olg.positional_encoding(sd["posenc.Wr.weight"], olg.normalize_keypoints(kpts1, size1))
        full_e0, full_e1 = e0, e1
        early, prune = depth_confidence > 0, width_confidence > 0
        ind0, ind1 = torch.arange(m)[None], torch.arange(n)[None]
        prune0, prune1 = torch.ones_like(ind0), torch.ones_like(ind1)
        layers = []
        i = 0
        for i in range(n_layers):
            x0 = olg.self_block(sd, f"transformers.{i}.self_attn", x0, e0, heads)
            x1 = olg.self_block(sd, f"transformers.{i}.self_attn", x1, e1, heads)
            x0, x1 = olg.cross_block(sd, f"transformers.{i}.cross_attn", x0, x1, heads)
            rec = {"x0": x0[0].clone(), "x1": x1[0].clone(), "m": x0.shape[1], "n": x1.shape[1], "tok0": None,
                   "tok1": None, "sc0": None, "sc1": None, "ratio": None, "stop": False, "keep0": None, "keep1": None,
                   "ind0": ind0[0].clone(), "ind1": ind1[0].clone()}
            layers.append(rec)
            if i == n_layers - 1:
                break
            t0 = t1 = None
            if early:
                t0 = torch.sigmoid(olg._linear(sd, f"token_confidence.{i}.token.0", x0)).squeeze(-1)
                t1 = torch.sigmoid(olg._linear(sd, f"token_confidence.{i}.token.0", x1)).squeeze(-1)
                conf = torch.cat([t0, t1], -1)
                ratio = 1.0 - (conf < thr[i]).float().sum() / (m + n)
                rec.update(tok0=t0[0], tok1=t1[0], ratio=float(ratio))
                if ratio > depth_confidence:
                    rec["stop"] = True
                    break
            if prune:
                def mask(tok, x, tag):
                    sc = torch.sigmoid(olg._linear(sd, f"log_assignment.{i}.matchability", x)).squeeze(-1)
                    rec[tag] = sc[0]
                    keep = sc > (1 - width_confidence)
                    if tok is not None:
                        keep = keep | (tok <= thr[i])
                    return torch.where(keep)[1]

                k0, k1 = mask(t0, x0, "sc0"), mask(t1, x1, "sc1")
                rec.update(keep0=k0, keep1=k1)
                ind0, x0, e0 = ind0.index_select(1, k0), x0.index_select(1, k0), e0.index_select(-2, k0)
                ind1, x1, e1 = ind1.index_select(1, k1), x1.index_select(1, k1), e1.index_select(-2, k1)
                prune0[:, ind0] += 1
                prune1[:, ind1] += 1
        scores = olg.match_assignment(sd, f"log_assignment.{i}", x0, x1)
        m0, m1, s0, s1 = olg.filter_matches(scores, filter_threshold)
        final = {"pruned_matches0": m0, "pruned_matches1": m1, "pruned_scores0": s0, "pruned_scores1": s1,
                 "ind0": ind0[0], "ind1": ind1[0], "x0": x0[0], "x1": x1[0]}
        if prune:
            m0_ = torch.full((b, m), -1, dtype=m0.dtype)
            m1_ = torch.full((b, n), -1, dtype=m1.dtype)
            m0_[:, ind0] = torch.where(m0 == -1, -1, ind1.gather(1, m0.clamp(min=0)))
            m1_[:, ind1] = torch.where(m1 == -1, -1, ind0.gather(1, m1.clamp(min=0)))
            s0_, s1_ = torch.zeros((b, m)), torch.zeros((b, n))
            s0_[:, ind0], s1_[:, ind1] = s0, s1
            m0, m1, s0, s1 = m0_, m1_, s0_, s1_
        else:
            prune0 = torch.ones_like(s0) * n_layers
            prune1 = torch.ones_like(s1) * n_layers
    final.update({"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1,
                  "log_assignment": scores, "prune0": prune0, "prune1": prune1, "stop_layer": i + 1,
                  "ref_descriptors0": x0[:, None], "ref_descriptors1": x1[:, None]})
    return layers, final, full_e0, full_e1


def bands(layers, depth_confidence, width_confidence, n_layers=9, delta=DELTA):
    """Per decision layer, from the oracle's values alone: `unsure0/1` = boolean masks over the layer's rows whose keep
    decision is not compared (matchability within delta of 1 - width_confidence, or token confidence within delta of
    the layer's threshold), `n_unsure`, `rows`, and `ratio_margin` = |ratio - depth_confidence| in points (units of
    1 / (m + n) of the un-pruned sizes), None without early stopping."""
    thr = thresholds(n_layers)
    m_all, n_all = layers[0]["m"], layers[0]["n"]
    out = []
    for i, rec in enumerate(layers):
        if i == n_layers - 1 or rec["stop"] or rec["keep0"] is None:
            u0 = torch.zeros(rec["m"], dtype=torch.bool)
            u1 = torch.zeros(rec["n"], dtype=torch.bool)
        else:
            def unsure(sc, tok):
                u = (sc.double() - (1 - width_confidence)).abs() <= delta
                if tok is not None:
                    u = u | ((tok.double() - float(thr[i])).abs() <= delta)
                return u

            u0, u1 = unsure(rec["sc0"], rec["tok0"]), unsure(rec["sc1"], rec["tok1"])
        margin = None
        if rec["ratio"] is not None:
            margin = abs(rec["ratio"] - depth_confidence) * (m_all + n_all)
        out.append({"unsure0": u0, "unsure1": u1, "n_unsure": int(u0.sum() + u1.sum()), "rows": rec["m"] + rec["n"],
                    "ratio_margin": margin})
    return out


def near_tie_rows(scores, th=FILTER_THRESHOLD, tol=1e-4):
    """Rows of side 0 / columns of side 1 of a log assignment [1,M+1,N+1] whose match is not compared index by index:
    the oracle's matching score within tol of the filter threshold, or the two largest assignment scores of the row
    (column) within tol of each other while the larger one can pass the threshold (the rule tools/micro/fuzz_models.py applies, decided on the oracle alone)."""
    inner = scores[0, :-1, :-1].double()

    def close(t):  # a tie below the threshold changes nothing: the entry is -1 whichever index wins
        if t.shape[-1] < 2:
            return torch.zeros(t.shape[0], dtype=torch.bool)
        top = t.topk(2, dim=-1).values.exp()
        return ((top[:, 0] - top[:, 1]) < tol) & (top[:, 0] > th - tol)

    r, c = close(inner), close(inner.t())
    best0, best1 = inner.max(1), inner.max(0)
    at_th0 = (best0.values.exp() - th).abs() < tol
    at_th1 = (best1.values.exp() - th).abs() < tol
    # a row is also unsure when the column it points at is, and the other way round (the mutual check reads both)
    skip0 = r | at_th0 | c[best0.indices] | at_th1[best0.indices]
    skip1 = c | at_th1 | r[best1.indices] | at_th0[best1.indices]
    return skip0, skip1
