"""Checker of csrc/eval_metrics.hip: the HPatches match metrics and the weighted DLT written out with torch operations.

This is this project's own statement of the arithmetic, organised like tests/pose_reference.py: one pair at a time, in
the dtype of its inputs (float64 for the GPU comparison, float32 to show the rules do not depend on the precision).
The M x N distance matrix is walked in row chunks, so a 4736 x 4400 pair stays within a few hundred MB.
tests/test_hpatches_reference_host.py pins the match metrics to vectors that the reference project produced
(tests/golden/hpatches_metrics.npz).  The DLT has no such vectors: the reference delegates it to kornia's
find_homography_dlt, which is not available where the fixture is made, so parity with kornia's solver (and with OpenCV)
stays unpinned; the DLT is pinned by what defines it (exact correspondences recover H, the weights matter).

Beside every verdict the checker says whether it is UNDECIDED: whether a decision it rests on is within DELTA of going
the other way, so that a float32 evaluation of the same rule may legitimately differ.  DELTA = 2e-3 px is this
project's bound on a float32 projection of coordinates below 4096 (tests/test_gpu_ransac.py): keep coordinates below
4096.  Candidates with bit-identical coordinates ("twins") are never undecided against each other: their distances are
equal in any arithmetic, and the lower index is the answer.

`rule=` selects a deliberately WRONG variant of one rule (WRONG_RULES); the host test shows the fixture rejects each.
"""
import torch

DELTA = 2e-3
WRONG_RULES = ("last_index_ties", "dist_negatives", "pos_le")
RESULT_KEYS = ("prec@1px", "prec@3px", "num_matches", "num_keypoints", "gt_match_recall@3px", "gt_match_precision@3px")
INF = float("inf")


def warp(kp, H, eps=0.0):
    """[K,2] points through H [3,3]: x H[r,0] + y H[r,1] + H[r,2], divided by (w + eps)."""
    x, y = kp[:, 0], kp[:, 1]
    wx = x * H[0, 0] + y * H[0, 1] + H[0, 2]
    wy = x * H[1, 0] + y * H[1, 1] + H[1, 2]
    ww = x * H[2, 0] + y * H[2, 1] + H[2, 2]
    return torch.stack([wx / (ww + eps), wy / (ww + eps)], -1)


def _chunks(kp0, kp1, k01, k10, chunk):
    """Row chunks of the squared-distance matrices: (row range, D0 = |warp(kp0_i) - kp1_j|^2, D1 = |kp0_i - warp^-1(kp1_j)|^2,
    D = max(D0, D1))."""
    for lo in range(0, kp0.shape[0], chunk):
        r = slice(lo, min(lo + chunk, kp0.shape[0]))
        D0 = ((k01[r, None] - kp1[None]) ** 2).sum(-1)
        D1 = ((kp0[r, None] - k10[None]) ** 2).sum(-1)
        yield r, D0, D1, torch.maximum(D0, D1)


def _argmin(D, dim, rule):
    if rule == "last_index_ties":
        idx = D.shape[dim] - 1 - D.flip(dim).min(dim).indices
        return D.gather(dim, idx.unsqueeze(dim)).squeeze(dim), idx
    m = D.min(dim)  # first index among equals
    return m.values, m.indices


def gt_matches(kp0, kp1, H, pos_th=3.0, neg_th=3.0, rule=None, chunk=256, Hinv=None):
    """Ground-truth matches of ONE pair from a homography: kp0 [M,2], kp1 [N,2], H [3,3] (0 -> 1).  Both key-point sets
    are warped into the other image with divisor w + 1e-5; dist = max(d0, d1); i <-> j match when each is the other's
    argmin of dist (first index among equals) and dist < pos_th^2; a point whose nearest neighbour in d0 (d1 for
    image 1) is farther than neg_th is unmatched (-1); every other point is ignored (-2); N == 0 or M == 0: all -1.
    -> {"matches0" [M], "matches1" [N], "undecided0" [M] bool, "undecided1" [N] bool}"""
    M, N, dev = kp0.shape[0], kp1.shape[0], kp0.device
    if M == 0 or N == 0:
        return {"matches0": torch.full((M,), -1, dtype=torch.long, device=dev),
                "matches1": torch.full((N,), -1, dtype=torch.long, device=dev),
                "undecided0": torch.zeros(M, dtype=torch.bool, device=dev),
                "undecided1": torch.zeros(N, dtype=torch.bool, device=dev)}
    if Hinv is None:
        Hinv = torch.linalg.inv(H)
    k01, k10 = warp(kp0, H, 1e-5), warp(kp1, Hinv, 1e-5)
    last = rule == "last_index_ties"
    # pass 1: per row (best, argmin, runner-up that is no twin of the winner, min d0); per column (best, argmin, min d1)
    row_best, row_arg, row_second, row_d0 = (torch.empty(M, dtype=kp0.dtype, device=dev) for _ in range(4))
    row_arg = row_arg.long()
    col_best = torch.full((N,), INF, dtype=kp0.dtype, device=dev)
    col_arg = torch.zeros(N, dtype=torch.long, device=dev)
    col_d1 = torch.full((N,), INF, dtype=kp0.dtype, device=dev)
    for r, D0, D1, D in _chunks(kp0, kp1, k01, k10, chunk):
        best, arg = _argmin(D, 1, rule)
        row_best[r], row_arg[r] = best, arg
        row_d0[r] = (D if rule == "dist_negatives" else D0).min(1).values
        twin = (kp1[None] == kp1[arg][:, None]).all(-1)
        row_second[r] = torch.where(twin, torch.full_like(D, INF), D).min(1).values
        cbest, carg = _argmin(D, 0, rule)
        take = (cbest <= col_best) if last else (cbest < col_best)
        col_best = torch.where(take, cbest, col_best)
        col_arg = torch.where(take, carg + r.start, col_arg)
        col_d1 = torch.minimum(col_d1, (D if rule == "dist_negatives" else D1).min(0).values)
    # pass 2: per column the runner-up that is no twin of the winner
    col_second = torch.full((N,), INF, dtype=kp0.dtype, device=dev)
    for r, _, _, D in _chunks(kp0, kp1, k01, k10, chunk):
        twin = (kp0[r][:, None] == kp0[col_arg][None]).all(-1)
        col_second = torch.minimum(col_second, torch.where(twin, torch.full_like(D, INF), D).min(0).values)
    pos2, neg2 = pos_th**2, neg_th**2
    below = (lambda d: d <= pos2) if rule == "pos_le" else (lambda d: d < pos2)
    rows, cols = torch.arange(M, device=dev), torch.arange(N, device=dev)
    hit0 = (col_arg[row_arg] == rows) & below(row_best)
    hit1 = (row_arg[col_arg] == cols) & below(col_best)
    m0 = torch.where(hit0, row_arg, torch.full_like(row_arg, -2))
    m1 = torch.where(hit1, col_arg, torch.full_like(col_arg, -2))
    m0 = torch.where(row_d0 > neg2, torch.full_like(m0, -1), m0)
    m1 = torch.where(col_d1 > neg2, torch.full_like(m1, -1), m1)

    def near(best, second):  # the argmin could go to another candidate, and the winner is close enough to matter
        return (second.sqrt() - best.sqrt() < 2 * DELTA) & (best.sqrt() < pos_th + DELTA)

    row_near, col_near = near(row_best, row_second), near(col_best, col_second)
    und0 = ((row_best.sqrt() - pos_th).abs() < DELTA) | ((row_d0.sqrt() - neg_th).abs() < DELTA) | row_near | col_near[row_arg]
    und1 = ((col_best.sqrt() - pos_th).abs() < DELTA) | ((col_d1.sqrt() - neg_th).abs() < DELTA) | col_near | row_near[col_arg]
    return {"matches0": m0, "matches1": m1, "undecided0": und0, "undecided1": und1}


def match_errors(kp0, kp1, m0, H, Hinv=None):
    """Symmetric transfer error of the predicted matches of ONE pair, plain division: [M] values, +inf where the match
    index is >= N (it names no key point), NaN where there is no match; and whether an error is within DELTA of the
    1 px or the 3 px threshold.  -> (err [M], undecided [M] bool)"""
    N = kp1.shape[0]
    if Hinv is None:
        Hinv = torch.linalg.inv(H)
    has = (m0 > -1) & (m0 < N)
    j = torch.where(has, m0, torch.zeros_like(m0)) if N > 0 else torch.zeros_like(m0)
    err = torch.full((kp0.shape[0],), float("nan"), dtype=kp0.dtype, device=kp0.device)
    err = torch.where(m0 >= N, torch.full_like(err, INF), err)
    if N > 0 and kp0.shape[0] > 0:
        b = kp1[j]
        e01 = ((warp(kp0, H) - b) ** 2).sum(-1).sqrt()
        e10 = ((warp(b, Hinv) - kp0) ** 2).sum(-1).sqrt()
        err = torch.where(has, (e01 + e10) / 2.0, err)
    und = has & (((err - 1.0).abs() < DELTA) | ((err - 3.0).abs() < DELTA))
    return err, und


def _ratio(num, den):
    return float(num) / (1e-8 + float(den))


def match_ratios(m0, gt0):
    """(recall, precision) of predicted matches m0 [M] against ground-truth matches gt0 [M]: agreement over the points
    with a ground-truth match, and over the matched points whose ground truth is not `ignore`; x / (1e-8 + count)."""
    agree = m0 == gt0
    rec, prec = gt0 > -1, (m0 > -1) & (gt0 >= -1)
    return _ratio((agree & rec).sum(), rec.sum()), _ratio((agree & prec).sum(), prec.sum())


def metrics(kp0, kp1, m0, H, pos_th=3.0, neg_th=3.0, rule=None, Hinv=None):
    """ONE pair -> the six values in RESULT_KEYS order (python floats)."""
    err, _ = match_errors(kp0, kp1, m0, H, Hinv)
    e = err[m0 > -1]
    n = e.numel()
    gt0 = gt_matches(kp0, kp1, H, pos_th, neg_th, rule, Hinv=Hinv)["matches0"]
    rec, prec = match_ratios(m0, gt0)
    return [float((e < 1).sum()) / n if n else 0.0, float((e < 3).sum()) / n if n else 0.0, float(n),
            (kp0.shape[0] + kp1.shape[0]) / 2.0, rec, prec]


# ---- weighted DLT ----------------------------------------------------------------------------------------------------
def _hartley(p):
    """Translate to the centroid, scale the mean distance to sqrt(2) (+1e-8 in the divisor) -> (points, T [3,3])."""
    mean = p.mean(0)
    s = 2.0**0.5 / ((p - mean).norm(dim=-1).mean() + 1e-8)
    T = torch.tensor([[s, 0.0, -s * mean[0]], [0.0, s, -s * mean[1]], [0.0, 0.0, 1.0]], dtype=p.dtype)
    return (p - mean) * s, T


def corner_error(H, H_gt, size):
    """Mean distance of the four image corners (0,0) (W,0) (W,H) (0,H) warped by H and by H_gt, plain division."""
    w, h = float(size[0]), float(size[1])
    c = torch.tensor([[0.0, 0.0], [w, 0.0], [w, h], [0.0, h]], dtype=H.dtype)
    return float(((warp(c, H) - warp(c, H_gt)) ** 2).sum(-1).sqrt().mean())


def dlt(kp0, kp1, m0, scores, H_gt, size, use_weights=True):
    """Weighted DLT homography of ONE pair in float64 from the matches with an index in [0, N): Hartley normalisation,
    two design rows per match, A^T diag(w) A, eigenvector of the smallest eigenvalue (torch.linalg.eigh), de-normalise,
    divide by H[2,2] + 1e-8.  The sign of an eigenvector is not defined and the +1e-8 makes the two results differ by
    about 2e-8 / |f8|: `H` holds both, [2,3,3].  `err` is the corner error of H[0] against H_gt; `kappa` =
    lambda_max / (lambda_2 - lambda_1), how much an error of the normal matrix is amplified in the eigenvector.
    Fewer than four such matches: everything +inf."""
    N = kp1.shape[0]
    sel = (m0 > -1) & (m0 < N)
    if int(sel.sum()) < 4:
        return {"H": torch.full((2, 3, 3), INF, dtype=torch.float64), "err": INF, "kappa": INF}
    p0, p1 = kp0[sel].double(), kp1[m0[sel]].double()
    w = scores[sel].double() if use_weights else torch.ones(int(sel.sum()), dtype=torch.float64)
    q0, T0 = _hartley(p0)
    q1, T1 = _hartley(p1)
    x1, y1, x2, y2 = q0[:, 0], q0[:, 1], q1[:, 0], q1[:, 1]
    o, z = torch.ones_like(x1), torch.zeros_like(x1)
    ax = torch.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], -1)
    ay = torch.stack([x1, y1, o, z, z, z, -x2 * x1, -x2 * y1, -x2], -1)
    A = (ax.T * w) @ ax + (ay.T * w) @ ay
    evals, evecs = torch.linalg.eigh(A)
    Hs = []
    for sign in (1.0, -1.0):
        f = torch.linalg.inv(T1) @ (sign * evecs[:, 0]).reshape(3, 3) @ T0
        Hs.append(f / (f[2, 2] + 1e-8))
    Hs = torch.stack(Hs)
    return {"H": Hs, "err": corner_error(Hs[0], H_gt.double(), size),
            "kappa": float(evals[-1] / (evals[1] - evals[0]))}
