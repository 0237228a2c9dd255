"""Float64 restatement of the GPU RANSAC homography estimator (csrc/ransac.hip; DESIGN.md "Robust homography") and
the seeded inputs its tests share.  Test infrastructure only: numpy float64 on the CPU, step by step the algorithm the
kernel runs -- ordered compaction of the matches, the counter-based sampler (`eval_utils.ransac_sample_indices`, pure
integer numpy), the closed-form 4-point solve on Hartley-normalised points, MSAC scores summed in correspondence
order for every threshold, argmin by (score, h), local optimisation by the unweighted normalised DLT.  The package
never imports this file."""
import numpy as np

from glue_factory_colon_amd.eval_utils import ransac_sample_indices

DET_EPS = 1e-10
SWEEP = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
# (n key points = M = N, outlier share, noise sigma in pixels, hypotheses): the regimes the tests run
TABLE = [(12, 0.0, 0.0, 256), (60, 0.3, 0.0, 512), (300, 0.6, 0.5, 1024), (1000, 0.5, 0.5, 1024), (1000, 0.7, 0.5, 2048)]
IMAGE_WH = (640.0, 480.0)

# Largest corner errors (px) the float64 restatement itself gives on rr.table_cases() with thresholds [0.5, 1, 3] and
# the six-threshold sweep, seed 0 (measured: printed by test_ransac_host.py::test_restatement_on_the_table).  The bounds are 1.5 x these.
MEASURED_MAX_NOISE_FREE = 3.69e-5  # rows sigma = 0
MEASURED_MAX_NOISY_T05 = 1.20      # rows sigma = 0.5 at t = 0.5 (= sigma)
MEASURED_MAX_NOISY = 0.638         # rows sigma = 0.5 at t >= 1
BOUND_NOISE_FREE, BOUND_NOISY_T05, BOUND_NOISY = 1.5 * 3.69e-5, 1.5 * 1.20, 1.5 * 0.638


def error_bound(sigma, t):
    return BOUND_NOISE_FREE if sigma == 0 else (BOUND_NOISY_T05 if t < 1.0 else BOUND_NOISY)


# ---- inputs ------------------------------------------------------------------------------------------------
def _area2(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def make_case(n, outlier_share, sigma, seed, unmatched_share=0.1):
    """A 640 x 480 scene: H_gt from four corners each moved by up to +-25 % of the image size, M = N = n key points
    (uniform), matches0 a random permutation with `unmatched_share` of the rows set to -1; `outlier_share` of the
    matched rows point at a uniform random position, the others at H_gt(kp0) + N(0, sigma).  float32 like the cache."""
    w, h = IMAGE_WH
    for attempt in range(100):
        rng = np.random.default_rng([seed, attempt])
        src = np.array([[0, 0], [w, 0], [w, h], [0, h]], dtype=np.float64)
        dst = src + rng.uniform(-0.25, 0.25, (4, 2)) * np.array([w, h])
        H_gt, ok = homography_4pt(src[None, :, 0], src[None, :, 1], dst[None, :, 0], dst[None, :, 1])
        H_gt = H_gt[0].reshape(3, 3)
        kp0 = rng.uniform(0, 1, (n, 2)) * np.array([w, h])
        den = kp0 @ H_gt[2, :2] + H_gt[2, 2]
        if ok[0] and (n == 0 or den.min() > 0.2):
            break
    else:
        raise RuntimeError("no usable scene")
    proj = (kp0 @ H_gt[:2, :2].T + H_gt[:2, 2]) / den[:, None] if n else np.zeros((0, 2))
    perm = rng.permutation(n)
    m0 = perm.astype(np.int64)
    unmatched = rng.permutation(n)[: int(unmatched_share * n)]
    matched = np.setdiff1d(np.arange(n), unmatched)
    outl = rng.permutation(matched)[: int(round(outlier_share * len(matched)))]
    tgt = proj + rng.normal(0, 1, (n, 2)) * sigma
    tgt[outl] = rng.uniform(0, 1, (len(outl), 2)) * np.array([w, h])
    kp1 = np.zeros((n, 2))
    kp1[perm] = tgt
    kp1[perm[unmatched]] = rng.uniform(0, 1, (len(unmatched), 2)) * np.array([w, h])
    m0[unmatched] = -1
    is_outlier = np.zeros(n, bool)
    is_outlier[outl] = True
    return {"kp0": kp0.astype(np.float32), "kp1": kp1.astype(np.float32), "m0": m0, "H_gt": H_gt.astype(np.float32),
            "size": np.array(IMAGE_WH, np.float32), "clean": ~is_outlier & (m0 >= 0)}


# ---- the algorithm -----------------------------------------------------------------------------------------
def correspondences(kp0, kp1, m0):
    """Matches (i, m0[i]) with 0 <= m0[i] < N in ascending i -> ([n,4] float64 rows x0 y0 x1 y1, their indices i)."""
    kp0, kp1, m0 = np.asarray(kp0), np.asarray(kp1), np.asarray(m0)
    idx = np.nonzero((m0 > -1) & (m0 < len(kp1)))[0]
    return np.concatenate([kp0[idx], kp1[m0[idx]]], axis=1).astype(np.float64).reshape(-1, 4), idx


def _normalise4(x, y):
    mx = (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) * 0.25
    my = (((y[:, 0] + y[:, 1]) + y[:, 2]) + y[:, 3]) * 0.25
    d = 0.0
    for k in range(4):
        ax, ay = x[:, k] - mx, y[:, k] - my
        d = d + np.sqrt(ax * ax + ay * ay)
    s = 1.4142135623730951 / (d * 0.25 + 1e-8)
    return s[:, None] * (x - mx[:, None]), s[:, None] * (y - my[:, None]), mx, my, s


def _basis(u, v):
    d = _area2(u[:, 0], v[:, 0], u[:, 1], v[:, 1], u[:, 2], v[:, 2])
    l0 = _area2(u[:, 3], v[:, 3], u[:, 1], v[:, 1], u[:, 2], v[:, 2])
    l1 = _area2(u[:, 0], v[:, 0], u[:, 3], v[:, 3], u[:, 2], v[:, 2])
    l2 = _area2(u[:, 0], v[:, 0], u[:, 1], v[:, 1], u[:, 3], v[:, 3])
    B = np.stack([l0 * u[:, 0], l1 * u[:, 1], l2 * u[:, 2], l0 * v[:, 0], l1 * v[:, 1], l2 * v[:, 2], l0, l1, l2], 1)
    return B, np.minimum(np.minimum(np.abs(d), np.abs(l0)), np.minimum(np.abs(l1), np.abs(l2)))


def homography_4pt(x0, y0, x1, y1):
    """[K,4] coordinate arrays -> (H [K,9] divided by H[2][2], ok [K]).  Closed form on Hartley-normalised points:
    Hn = B1 adj(B0) with B the map from the projective basis to the four points; not ok: three points collinear in
    either image (twice the normalised triangle area <= 1e-10) or a non-finite entry."""
    x0, y0, x1, y1 = (np.asarray(a, dtype=np.float64) for a in (x0, y0, x1, y1))
    with np.errstate(all="ignore"):
        u0, v0, mx0, my0, s0 = _normalise4(x0, y0)
        u1, v1, mx1, my1, s1 = _normalise4(x1, y1)
        A, e0 = _basis(u0, v0)
        B, e1 = _basis(u1, v1)
        a = A.T
        C = [a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
             a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
             a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]
        b = B.T
        h = [[(b[r * 3] * C[c] + b[r * 3 + 1] * C[3 + c]) + b[r * 3 + 2] * C[6 + c] for c in range(3)] for r in range(3)]
        g = []
        for r in range(3):
            g0, g1 = h[r][0] * s0, h[r][1] * s0
            g.append([g0, g1, (h[r][2] - g0 * mx0) - g1 * my0])
        f = [[g[0][c] / s1 + mx1 * g[2][c] for c in range(3)], [g[1][c] / s1 + my1 * g[2][c] for c in range(3)],
             [g[2][c] for c in range(3)]]
        inv = 1.0 / f[2][2]
        H = np.stack([f[r][c] * inv for r in range(3) for c in range(3)], axis=1)
        ok = (e0 > DET_EPS) & (e1 > DET_EPS) & np.isfinite(H).all(axis=1)
    return H, ok


def residual2(H, corr):
    """Squared forward transfer error of models H [K,9] on correspondences [n,4] -> [K,n]; +inf where the projective
    denominator is <= 0 or not finite."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    x0, y0, x1, y1 = (corr[None, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        X = (H[:, 0:1] * x0 + H[:, 1:2] * y0) + H[:, 2:3]
        Y = (H[:, 3:4] * x0 + H[:, 4:5] * y0) + H[:, 5:6]
        W = (H[:, 6:7] * x0 + H[:, 7:8] * y0) + H[:, 8:9]
        iw = 1.0 / W
        dx, dy = X * iw - x1, Y * iw - y1
        r2 = dx * dx + dy * dy
    return np.where((W > 0) & (W < np.inf), r2, np.inf)


def msac(r2, t2):
    """sum of min(r2, t2) over the correspondences, in correspondence order (a running sum, not a pairwise one)."""
    r2 = np.atleast_2d(r2)
    if r2.shape[1] == 0:
        return np.zeros(r2.shape[0])
    return np.cumsum(np.where(r2 < t2, r2, t2), axis=1)[:, -1]


def dlt(corr):
    """Unweighted Hartley-normalised DLT over correspondences [k,4] (k >= 4): eigenvector of the smallest eigenvalue
    of the 9x9 normal matrix, de-normalised, divided by H[2][2] -> [9] (may be non-finite)."""
    x0, y0, x1, y1 = corr.T
    k = len(corr)
    mx0, my0, mx1, my1 = x0.sum() / k, y0.sum() / k, x1.sum() / k, y1.sum() / k
    sa = 1.4142135623730951 / (np.sqrt((x0 - mx0) ** 2 + (y0 - my0) ** 2).sum() / k + 1e-8)
    sb = 1.4142135623730951 / (np.sqrt((x1 - mx1) ** 2 + (y1 - my1) ** 2).sum() / k + 1e-8)
    a, b, c, d = sa * (x0 - mx0), sa * (y0 - my0), sb * (x1 - mx1), sb * (y1 - my1)
    z, o = np.zeros(k), np.ones(k)
    rx = np.stack([z, z, z, -a, -b, -o, d * a, d * b, d], 1)
    ry = np.stack([a, b, o, z, z, z, -c * a, -c * b, -c], 1)
    N = rx.T @ rx + ry.T @ ry
    _, vec = np.linalg.eigh(N)
    hn = vec[:, 0].reshape(3, 3)
    T0 = np.array([[sa, 0, -sa * mx0], [0, sa, -sa * my0], [0, 0, 1]])
    T1i = np.array([[1 / sb, 0, mx1], [0, 1 / sb, my1], [0, 0, 1]])
    with np.errstate(all="ignore"):
        H = T1i @ hn @ T0
        return (H / H[2, 2]).reshape(9)


def corner_error(H, H_gt, size):
    """Mean distance of the four warped image corners (float64)."""
    w, h = float(size[0]), float(size[1])
    c = np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]], dtype=np.float64)
    with np.errstate(all="ignore"):
        a, b = c @ np.asarray(H, np.float64).reshape(3, 3).T, c @ np.asarray(H_gt, np.float64).reshape(3, 3).T
        e = np.sqrt((((a[:, :2] / a[:, 2:]) - (b[:, :2] / b[:, 2:])) ** 2).sum(1)).mean()
    return float(e) if np.isfinite(e) else float("inf")


def corners(H, size):
    w, h = float(size[0]), float(size[1])
    c = np.array([[0, 0, 1], [w, 0, 1], [w, h, 1], [0, h, 1]], dtype=np.float64) @ np.asarray(H, np.float64).reshape(3, 3).T
    return c[:, :2] / c[:, 2:]


def hypotheses(corr, seed, stream_id, num_hypotheses):
    """All minimal models of a pair: (H [K,9], ok [K], samples [K,4])."""
    s = ransac_sample_indices(seed, stream_id, len(corr), num_hypotheses)
    p = corr[s]  # [K,4,4]
    H, ok = homography_4pt(p[:, :, 0], p[:, :, 1], p[:, :, 2], p[:, :, 3])
    return H, ok, s


def ransac(kp0, kp1, m0, thresholds, num_hypotheses=2048, lo_iters=3, seed=0, stream_id=0, H_gt=None, size=None):
    """The whole estimator for one pair -> a list with one dict per threshold: success, H [9], H_minimal [9],
    best_hypothesis, inliers [M] bool, num_inliers, error (when H_gt is given), scores [K] (every hypothesis's MSAC
    score, +inf for skipped samples), lo_scores (the accepted scores, first = the minimal model's)."""
    corr, idx = correspondences(kp0, kp1, m0)
    M, n = len(kp0), len(corr)
    fail = {"success": False, "H": np.eye(3).reshape(9), "H_minimal": np.eye(3).reshape(9), "best_hypothesis": -1,
            "inliers": np.zeros(M, bool), "num_inliers": 0, "error": float("inf"), "scores": None, "lo_scores": []}
    if n < 4:
        return [dict(fail) for _ in thresholds]
    H, ok, _ = hypotheses(corr, seed, stream_id, num_hypotheses)
    r2 = residual2(H, corr)
    out = []
    for t in thresholds:
        t2 = float(np.float32(t)) ** 2
        scores = np.where(ok, msac(r2, t2), np.inf)
        best = int(np.argmin(scores))  # first minimum: ties to the lower h
        if not np.isfinite(scores[best]):
            out.append({**fail, "scores": scores})
            continue
        cur = H[best].copy()
        cur_score = float(msac(residual2(cur, corr), t2)[0])
        trace = [cur_score]
        for _ in range(lo_iters):
            inl = residual2(cur, corr)[0] < t2
            if inl.sum() < 4:
                break
            cand = dlt(corr[inl])
            if not np.isfinite(cand).all():
                break
            cand_score = float(msac(residual2(cand, corr), t2)[0])
            if not cand_score < cur_score:
                break
            cur, cur_score = cand, cand_score
            trace.append(cur_score)
        inl = residual2(cur, corr)[0] < t2
        inliers = np.zeros(M, bool)
        inliers[idx] = inl
        res = {"success": True, "H": cur, "H_minimal": H[best], "best_hypothesis": best, "inliers": inliers,
               "num_inliers": int(inl.sum()), "scores": scores, "lo_scores": trace}
        if H_gt is not None:
            res["error"] = corner_error(cur, H_gt, size)
        out.append(res)
    return out


SCENES_PER_ROW = 2


def table_cases():
    """The seeded scenes of TABLE: a list of (row, scene, case dict, hypotheses); stream_id = 100 * row + scene."""
    out = []
    for r, (n, share, sigma, hyp) in enumerate(TABLE):
        for k in range(SCENES_PER_ROW):
            out.append((r, k, make_case(n, share, sigma, seed=1000 * r + k), hyp))
    return out
