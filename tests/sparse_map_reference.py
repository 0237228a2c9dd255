"""Restatement of the sparse-map labels (gt_matches_from_pose_sparse_map and gt_matches_from_pose_sparse_dense_map,
gluefactory/geometry/gt_generation.py:441-591, 271-438) with torch operations in float64: the checker of
csrc/gt_sparse_map.hip, plus the inputs of its tests.

  sparse_map_labels   the matching part of ONE pair from projections that exist (what gfc_gt_matches_sparse_map receives):
                      matches0/1, the eight masks, positive0, assignment, reward, extra_positives in closed form (per row
                      |S_i u {p_i}| - 1) AND counted on the dense matrix, and which verdicts are UNDECIDED: resting on a
                      decision within DELTA (2e-3 px, tests/hpatches_reference.py) of going the other way, where a
                      float32 evaluation may differ.  The th_epi rule depends on who is `ignore`: a point is undecided
                      there too when its verdict changes with the undecided points counted in or out.
  entry_case          seeded inputs: key points and projections of hpatches_cases.metric_case, thinned visible / valid
                      masks, planted ids (true correspondences, duplicates, ids without valid_3D, contradicting ids) and
                      a fundamental matrix.

`rule=` selects a deliberately WRONG variant (WRONG_RULES); the host test shows the fixture rejects each.
"""
import torch

import hpatches_cases as hc
from hpatches_reference import DELTA

WRONG_RULES = ("negative_overrides_positive", "distance_before_seed", "last_index_ties")
MASK_KEYS = ("mask_pos_3d_map", "mask_pos_reproj", "mask_neg_reproj", "mask_neg_epi")
INF = float("inf")


def _argmin(D, dim, rule):
    if rule == "last_index_ties":
        return D.shape[dim] - 1 - D.flip(dim).min(dim).indices
    return D.min(dim).indices  # first index among equals; 0 for a row of +inf


def _first_true(P, dim, rule):
    """argmax of a 0/1 matrix: the lowest index that is set (0 for none)."""
    if rule == "last_index_ties":
        return P.shape[dim] - 1 - P.flip(dim).double().argmax(dim)
    return P.double().argmax(dim)


def _second(D, arg, pts, dim):
    """The smallest distance along `dim` to a candidate that is no bit-identical twin of the winner."""
    win = pts[arg]
    twin = (pts[None] == win[:, None]).all(-1)
    if dim == 0:
        twin = twin.T
    return torch.where(twin, torch.full_like(D, INF), D).min(dim).values


def epi_all(kp0, kp1, F):
    """sym_epipolar_distance_all (gluefactory/geometry/epipolar.py:59-72): [M,N]."""
    h0 = torch.cat([kp0, torch.ones_like(kp0[:, :1])], -1)
    h1 = torch.cat([kp1, torch.ones_like(kp1[:, :1])], -1)
    l0 = h0 @ F.T   # F p0: lines in image 1
    l1 = h1 @ F     # F^T p1: lines in image 0
    num = (h1[None] * l0[:, None]).sum(-1).abs()
    den0 = (l0[:, 0] ** 2 + l0[:, 1] ** 2 + 1e-15).sqrt()
    den1 = (l1[:, 0] ** 2 + l1[:, 1] ** 2 + 1e-15).sqrt()
    return (num / den0[:, None] + num / den1[None]) / 2


def sparse_map_labels(kp0, kp1, p01, p10, vis0, vis1, valid0, valid1, ids0=None, ids1=None, v3d0=None, v3d1=None,
                      F=None, pos_th=3.0, neg_th=5.0, epi_th=None, rule=None):
    """kp0, p01 [M,2], kp1, p10 [N,2] (M, N >= 1), masks [M] / [N]; ids None: no seeding.  All floats in one dtype."""
    M, N = kp0.shape[0], kp1.shape[0]
    vis0, vis1, valid0, valid1 = vis0.bool(), vis1.bool(), valid0.bool(), valid1.bool()
    m0 = torch.full((M,), -2, dtype=torch.long)
    m1 = torch.full((N,), -2, dtype=torch.long)
    zeros = lambda k: torch.zeros(k, dtype=torch.bool)  # noqa: E731
    masks = {k + s: zeros(M if s == "0" else N) for k in MASK_KEYS for s in "01"}
    positive_gt = torch.zeros((M, N), dtype=torch.bool)
    if ids0 is not None:
        a0 = torch.ones(M, dtype=torch.bool) if v3d0 is None else v3d0.bool()
        a1 = torch.ones(N, dtype=torch.bool) if v3d1 is None else v3d1.bool()
        positive_gt = (ids0[:, None] == ids1[None]) & a0[:, None] & a1[None]

    def seed(m0, m1):
        masks["mask_pos_3d_map0"], masks["mask_pos_3d_map1"] = positive_gt.any(1), positive_gt.any(0)
        return (torch.where(positive_gt.any(1), _first_true(positive_gt, 1, rule), m0),
                torch.where(positive_gt.any(0), _first_true(positive_gt, 0, rule), m1))

    if rule != "distance_before_seed":
        m0, m1 = seed(m0, m1)
    D0 = ((p01[:, None] - kp1[None]) ** 2).sum(-1)
    D1 = ((kp0[:, None] - p10[None]) ** 2).sum(-1)
    vis = vis0[:, None] & vis1[None]
    D = torch.where(vis, torch.maximum(D0, D1), torch.full_like(D0, INF))
    min0, min1 = _argmin(D, 1, rule), _argmin(D, 0, rule)
    positive_dist = torch.zeros_like(vis)
    if pos_th is not None:
        ismin0, ismin1 = torch.zeros_like(vis), torch.zeros_like(vis)
        ismin0[torch.arange(M), min0] = True
        ismin1[min1, torch.arange(N)] = True
        positive_dist = ismin0 & ismin1 & (D < pos_th**2)
        masks["mask_pos_reproj0"], masks["mask_pos_reproj1"] = positive_dist.any(1), positive_dist.any(0)
        m0 = torch.where((m0 == -2) & positive_dist.any(1), min0, m0)
        m1 = torch.where((m1 == -2) & positive_dist.any(0), min1, m1)
    if rule == "distance_before_seed":
        s0, s1 = seed(torch.full_like(m0, -2), torch.full_like(m1, -2))
        m0, m1 = torch.where(m0 == -2, s0, m0), torch.where(m1 == -2, s1, m1)
    own0, own1 = D0.min(1).values, D1.min(0).values
    if neg_th is not None:
        neg0, neg1 = (own0 > neg_th**2) & valid0, (own1 > neg_th**2) & valid1
        masks["mask_neg_reproj0"], masks["mask_neg_reproj1"] = neg0, neg1
        if rule == "negative_overrides_positive":
            m0, m1 = torch.where(neg0, -torch.ones_like(m0), m0), torch.where(neg1, -torch.ones_like(m1), m1)
        else:
            m0 = torch.where((m0 == -2) & neg0, -torch.ones_like(m0), m0)
            m1 = torch.where((m1 == -2) & neg1, -torch.ones_like(m1), m1)
    positive = positive_gt | positive_dist

    # margins of steps 3-5
    rb, cb = D.min(1).values, D.min(0).values
    rs, cs = _second(D, min0, kp1, 1), _second(D, min1, kp0, 0)
    pos_lim = INF if pos_th is None else pos_th

    def near(best, second):
        return (second.sqrt() - best.sqrt() < 2 * DELTA) & (best.sqrt() < pos_lim + DELTA) & (pos_th is not None)

    def at(d2, th):
        return zeros(d2.shape[0]) if th is None else (d2.sqrt() - th).abs() < DELTA

    rn, cn = near(rb, rs), near(cb, cs)
    und0 = at(rb, pos_th) | (at(own0, neg_th) & valid0) | rn | cn[min0]
    und1 = at(cb, pos_th) | (at(own1, neg_th) & valid1) | cn | rn[min1]
    und_dense = torch.zeros_like(vis)
    if pos_th is not None:
        und_dense = ((D.sqrt() - pos_th).abs() < DELTA) | ((rn[:, None] | cn[None]) & (D.sqrt() < pos_th + DELTA))

    ign0, ign1 = m0 == -2, m1 == -2  # the state BEFORE the epi_th rule
    E = None
    if epi_th is not None or neg_th is not None:
        assert F is not None
        E = epi_all(kp0, kp1, F)
    if epi_th is not None:
        def sweep(i0, i1):
            Em = torch.where(i0[:, None] & i1[None], E, torch.full_like(E, INF))
            return Em.min(1).values, Em.min(0).values

        e0, e1 = sweep(ign0, ign1)
        ex0, ex1 = e0 > epi_th, e1 > epi_th
        masks["mask_neg_epi0"], masks["mask_neg_epi1"] = ex0, ex1
        m0 = torch.where(ex0 & ~valid0 & ign0, -torch.ones_like(m0), m0)
        m1 = torch.where(ex1 & ~valid1 & ign1, -torch.ones_like(m1), m1)
        # with the undecided points counted as ignore, and with them counted out
        hi0, hi1 = sweep(ign0 | und0, ign1 | und1)
        lo0, lo1 = sweep(ign0 & ~und0, ign1 & ~und1)
        und_e0 = ((e0 - epi_th).abs() < DELTA) | ((hi0 > epi_th) != ex0) | ((lo0 > epi_th) != ex0)
        und_e1 = ((e1 - epi_th).abs() < DELTA) | ((hi1 > epi_th) != ex1) | ((lo1 > epi_th) != ex1)
        und0, und1 = und0 | und_e0, und1 | und_e1
        E = torch.where(ign0[:, None] & ign1[None], E, torch.full_like(E, INF))
        und_dense = und_dense | ((E - epi_th).abs() < DELTA) | (und0[:, None] | und1[None])
    gain = torch.maximum((D < pos_th**2).to(D.dtype) if pos_th is not None else torch.zeros_like(D),
                         positive.to(D.dtype))
    epi_val = epi_th if epi_th is not None else neg_th
    penalty = (E > epi_val).to(D.dtype) if epi_val is not None else torch.zeros_like(D)
    if epi_th is None and epi_val is not None:
        und_dense = und_dense | ((E - epi_val).abs() < DELTA)
    positive0 = torch.where(positive_dist.any(1), min0, -torch.ones_like(min0))
    # extra_positives in closed form: S_i = the id-equal valid columns, p_i = the distance positive
    count = positive_gt.sum(1)
    p_in_s = positive_gt[torch.arange(M), min0] & positive_dist.any(1)
    size = count + (positive_dist.any(1) & ~p_in_s).long()
    extra_closed = int((size - 1).clamp(min=0).sum())
    extra_dense = int((positive & (torch.arange(N)[None] != m0[:, None])).sum())
    return {"matches0": m0, "matches1": m1, **masks, "positive0": positive0, "assignment": positive,
            "reward": gain - penalty, "extra_positives": extra_closed, "extra_positives_dense": extra_dense,
            "undecided0": und0, "undecided1": und1, "undecided_dense": und_dense}


def fundamental(seed):
    """A fundamental matrix of a 640 x 480 pinhole pair with a small motion, float32 [3,3]."""
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]], dtype=torch.float64)
    w = 0.05 * torch.randn(3, generator=g, dtype=torch.float64)
    skew = lambda v: torch.tensor([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=torch.float64)  # noqa: E731
    R = torch.linalg.matrix_exp(skew(w))
    t = torch.randn(3, generator=g, dtype=torch.float64)
    Kinv = torch.linalg.inv(K)
    return (Kinv.T @ skew(t) @ R @ Kinv).float()


def entry_case(seed, b, m, n, twins=False):
    """Inputs of gfc_gt_matches_sparse_map for b pairs of m x n key points (float32 / bool / int64 CPU tensors)."""
    case = hc.metric_case(seed, b, m, n)
    g = torch.Generator().manual_seed(seed * 31 + 5)
    kp0, kp1, H = case["kp0"].clone(), case["kp1"].clone(), case["H"]
    if twins and m > 40 and n > 40:  # bit-identical twins on both sides: the first index must win at every split
        kp0[:, m - 3] = kp0[:, 2]
        kp0[:, m // 2] = kp0[:, 2]
        kp1[:, n - 1] = kp1[:, 5]
        kp1[:, n // 3] = kp1[:, 5]
    p01, p10 = hc.warp32(kp0, H), hc.warp32(kp1, torch.linalg.inv(H.double()).float())
    valid0, valid1 = torch.rand((b, m), generator=g) > 0.25, torch.rand((b, n), generator=g) > 0.25
    vis0, vis1 = valid0 & (torch.rand((b, m), generator=g) > 0.1), valid1 & (torch.rand((b, n), generator=g) > 0.1)
    # ids: unique and unrelated by default; true correspondences share one; then the special plants
    ids0 = torch.arange(m)[None].repeat(b, 1) + 1_000_000
    ids1 = torch.arange(n)[None].repeat(b, 1) + 2_000_000
    m0 = case["m0"]
    for i in range(b):
        rows = torch.nonzero(m0[i] > -1).flatten()
        rows = rows[torch.rand(rows.shape[0], generator=g) > 0.4]
        ids1[i, m0[i, rows]] = ids0[i, rows]
    if m >= 8 and n >= 8:
        ids0[:, [1, m // 2, m - 1]] = 77     # a triple in image 0 ...
        ids1[:, [n - 2, 3]] = 77             # ... and a pair in image 1: six positives
        ids0[:, 4] = ids1[:, (5 * n) // 7]   # an id pair wherever the distance says
    v3d0, v3d1 = torch.rand((b, m), generator=g) > 0.15, torch.rand((b, n), generator=g) > 0.15
    if m >= 8 and n >= 8:
        v3d0[:, [1, m // 2, m - 1, 4]] = True
        v3d1[:, [n - 2, 3, (5 * n) // 7]] = True
    if twins and m > 40 and n > 40:
        ids0[:, [2, m - 3]] = 99
        ids1[:, [5, n - 1, n // 3]] = 99
        v3d0[:, [2, m - 3]] = True
        v3d1[:, [5, n - 1, n // 3]] = True
    F = torch.stack([fundamental(seed * 7 + i) for i in range(b)])
    return {"kp0": kp0, "kp1": kp1, "p01": p01, "p10": p10, "vis0": vis0, "vis1": vis1, "valid0": valid0,
            "valid1": valid1, "ids0": ids0, "ids1": ids1, "v3d0": v3d0, "v3d1": v3d1, "F": F}


def labels_of(case, i, pos_th, neg_th, epi_th, use_ids=True, rule=None):
    """sparse_map_labels of pair i of an entry_case, in float64."""
    d = lambda k: case[k][i].double()  # noqa: E731
    ids = (case["ids0"][i], case["ids1"][i], case["v3d0"][i], case["v3d1"][i]) if use_ids else (None,) * 4
    return sparse_map_labels(d("kp0"), d("kp1"), d("p01"), d("p10"), case["vis0"][i], case["vis1"][i],
                             case["valid0"][i], case["valid1"][i], *ids, F=d("F"), pos_th=pos_th, neg_th=neg_th,
                             epi_th=epi_th, rule=rule)
