"""Checker of csrc/eval_pose.hip: the pose / depth match metrics written out with torch tensor operations.

This is this project's own statement of the arithmetic, written from the definitions (camera models, bilinear sampling,
mutual nearest neighbours, symmetric epipolar distance) and organised by coordinate (x and y as separate tensors, one
pair at a time), like the kernel.  tests/test_pose_reference_host.py pins it to vectors that the reference project
produced (tests/golden/pose_depth.npz); the GPU tests use it where the fixture has no case (edge shapes), and
tools/pose_eval_bench.py times it against the kernels: it forms the M x N matrices that the kernels avoid.

Conventions: a camera is a [10] tensor `w, h, fx, fy, cx, cy, d0, d1, d2, d3` plus a model name (PINHOLE uses no
coefficient, RADIAL d0 d1, OPENCV d0..d3 = k1 k2 p1 p2, OPENCV_FISHEYE d0..d3 = k1..k4 of the Kannala-Brandt model);
a pose a [12] tensor, R row-major then t, x_dst = R x_src + t.  Pixel centres are at +0.5.  Everything runs in the
dtype and on the device of its inputs.

`rule=` selects a deliberately WRONG variant of one rule (WRONG_RULES); the host test shows the fixture rejects each.
"""
import torch

MODELS = ("PINHOLE", "RADIAL", "OPENCV", "OPENCV_FISHEYE")
WRONG_RULES = ("last_index_ties", "masked_d0_negatives", "in_image_lt_size")
Z_MIN = 1e-4  # depth below which a point counts as behind the camera; also the floor of the divisor
NEWTON_ROUNDS, NEWTON_TOL, R_TINY = 10, 1e-12, 1e-12


def rot(T):
    return T[:9].reshape(3, 3)


def invert_pose(T):
    """(R, t) -> (R^T, -R^T t)."""
    Rt = rot(T).t()
    return torch.cat([Rt.reshape(9), -(Rt @ T[9:, None])[:, 0]])


# ---- camera models ---------------------------------------------------------------------------------------------------
def kb4_unproject_radius(rd, k):
    """Solve theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = rd by Newton from theta = rd, a fixed
    number of rounds; a point is frozen after the first round in which its own step is below the tolerance.  -> tan(theta)"""
    th = rd.clone()
    live = rd > R_TINY
    for _ in range(NEWTON_ROUNDS):
        t2 = th * th
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t4 * t4
        val = th * (1.0 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8) - rd
        slope = 1.0 + 3.0 * k[0] * t2 + 5.0 * k[1] * t4 + 7.0 * k[2] * t6 + 9.0 * k[3] * t8
        step = val / slope
        th = torch.where(live, th - step, th)
        live = live & (step.abs() >= NEWTON_TOL)
    return torch.tan(th)


def pixel_to_ray(cam, model, x, y):
    """Pixel -> point on the z = 1 plane.  Only the fisheye model removes its distortion here."""
    nx, ny = (x - cam[4]) / cam[2], (y - cam[5]) / cam[3]
    if model == "OPENCV_FISHEYE":
        rd = torch.sqrt(nx * nx + ny * ny)
        s = torch.where(rd > R_TINY, kb4_unproject_radius(rd, cam[6:10]) / rd, torch.ones_like(rd))
        nx, ny = nx * s, ny * s
    return nx, ny


def ray_to_pixel(cam, model, X, Y, Z, rule=None):
    """3-D point in the camera frame -> (px, py, ok): in front, inside the model's range, inside the image."""
    ok = Z > Z_MIN
    Zc = torch.where(Z < Z_MIN, torch.full_like(Z, Z_MIN), Z)
    u, v = X / Zc, Y / Zc
    if model == "OPENCV_FISHEYE":
        k = cam[6:10]
        r = torch.sqrt(u * u + v * v)
        th = torch.atan(r)
        t2 = th * th
        t3 = th * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        rd = th + k[0] * t3 + k[1] * t5 + k[2] * t7 + k[3] * t9
        s = torch.where(r > R_TINY, rd / r, torch.ones_like(r))
        u, v = u * s, v * s
        ok = ok & torch.isfinite(u) & torch.isfinite(v)
    elif model in ("RADIAL", "OPENCV"):
        k1, k2 = cam[6], cam[7]
        r2 = u * u + v * v
        g = k1 * r2 + k2 * r2**2
        du, dv = u + u * g, v + v * g
        # beyond the turning point of r (1 + k1 r^2 + k2 r^4) the model folds back into the image: not valid there
        disc = 9 * k1**2 - 20 * k2
        bounded = bool(((k2 > 0) & (disc > 0)) | ((k2 <= 0) & (k1 > 0)))
        if bounded:
            r2_max = torch.abs((torch.sqrt(disc) - 3 * k1) / (10 * k2) if k2 > 0 else 1 / (3 * k1))
            ok = ok & (r2 < r2_max)
        if model == "OPENCV":
            p1, p2 = cam[8], cam[9]
            uv = u * v
            du = du + 2 * p1 * uv + p2 * (r2 + 2 * u**2)
            dv = dv + 2 * p2 * uv + p1 * (r2 + 2 * v**2)
        u, v = du, dv
    px, py = u * cam[2] + cam[4], v * cam[3] + cam[5]
    if rule == "in_image_lt_size":
        inside = (px >= 0) & (px < cam[0]) & (py >= 0) & (py < cam[1])
    else:
        inside = (px >= 0) & (px <= cam[0] - 1) & (py >= 0) & (py <= cam[1] - 1)
    return px, py, ok & inside


# ---- depth sampling --------------------------------------------------------------------------------------------------
def sample_depth(x, y, depth):
    """Depth [H,W] at pixel coordinates: holes (<= 0) are NaN; bilinear over the four neighbours with zero padding
    (a neighbour outside the map adds nothing, a hole inside it makes the sum NaN whatever its weight); where that is
    NaN, the nearest pixel instead (round half to even, 0 outside).  -> (d, valid = finite and > 0)."""
    h, w = depth.shape
    nan = torch.full((), float("nan"), dtype=depth.dtype, device=depth.device)
    flat = torch.where(depth > 0, depth, nan).reshape(-1)
    gx, gy = x / w * 2 - 1, y / h * 2 - 1
    fx, fy = ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2

    def tap(ix, iy):
        inside = (ix >= 0) & (ix <= w - 1) & (iy >= 0) & (iy <= h - 1)
        idx = (iy.clamp(0, h - 1) * w + ix.clamp(0, w - 1)).long()
        return flat[idx], inside

    x0, y0 = torch.floor(fx), torch.floor(fy)
    x1, y1 = x0 + 1, y0 + 1
    lin = torch.zeros_like(fx)
    for ix, iy, wgt in ((x0, y0, (x1 - fx) * (y1 - fy)), (x1, y0, (fx - x0) * (y1 - fy)),
                        (x0, y1, (x1 - fx) * (fy - y0)), (x1, y1, (fx - x0) * (fy - y0))):
        val, inside = tap(ix, iy)
        lin = torch.where(inside, lin + val * wgt, lin)
    val, inside = tap(torch.round(fx), torch.round(fy))
    near = torch.where(inside, val, torch.zeros_like(val))
    d = torch.where(torch.isnan(lin), near, lin)
    return d, (~torch.isnan(d)) & (d > 0)


def pose_project(kp, depth_i, cam_i, model_i, cam_j, model_j, T_itoj, rule=None):
    """Key points [K,2] of view i: sampled depth, its validity, their projection into view j and whether they are
    visible there (valid depth and a valid projection).  What gfc_eval_pose_project computes."""
    x, y = kp[:, 0], kp[:, 1]
    d, valid = sample_depth(x, y, depth_i)
    nx, ny = pixel_to_ray(cam_i, model_i, x, y)
    P = torch.stack([nx * d, ny * d, d], -1) @ rot(T_itoj).t() + T_itoj[9:]
    px, py, ok = ray_to_pixel(cam_j, model_j, P[:, 0], P[:, 1], P[:, 2], rule)
    return d, valid, torch.stack([px, py], -1), valid & ok


# ---- ground-truth matches --------------------------------------------------------------------------------------------
def _argmin(D, dim, rule):
    if rule == "last_index_ties":
        return D.shape[dim] - 1 - D.flip(dim).min(dim).indices
    return D.min(dim).indices  # first index among equals


def gt_matches(kp0, kp1, depth0, depth1, cam0, model0, cam1, model1, T_0to1, T_1to0=None, pos_th=3.0, neg_th=5.0,
               rule=None):
    """Ground-truth matches of ONE pair from pose and depth.  D0[i,j] = |proj(kp0_i) - kp1_j|^2, D1[i,j] =
    |kp0_i - proj(kp1_j)|^2, D = max(D0, D1), +inf unless both points are visible in the other view.  i <-> j match when
    each is the other's argmin of D and D < pos_th^2.  A point with valid depth whose nearest neighbour in D0 (D1 for
    view 1), WITHOUT the visibility mask, is farther than neg_th is unmatched (-1); every other point is ignored (-2)."""
    if T_1to0 is None:
        T_1to0 = invert_pose(T_0to1)
    d0, valid0, p01, vis0 = pose_project(kp0, depth0, cam0, model0, cam1, model1, T_0to1, rule)
    d1, valid1, p10, vis1 = pose_project(kp1, depth1, cam1, model1, cam0, model0, T_1to0, rule)
    out = {"depth_keypoints0": d0, "depth_keypoints1": d1, "proj_0to1": p01, "proj_1to0": p10, "visible0": vis0,
           "visible1": vis1, "valid0": valid0, "valid1": valid1}
    M, N = kp0.shape[0], kp1.shape[0]
    if M == 0 or N == 0:
        out["matches0"] = torch.full((M,), -1, dtype=torch.long, device=kp0.device)
        out["matches1"] = torch.full((N,), -1, dtype=torch.long, device=kp0.device)
        out["visible0"], out["visible1"] = torch.zeros_like(vis0), torch.zeros_like(vis1)
        return out
    D0 = ((p01[:, None] - kp1[None]) ** 2).sum(-1)
    D1 = ((kp0[:, None] - p10[None]) ** 2).sum(-1)
    both = vis0[:, None] & vis1[None]
    D = torch.where(both, torch.maximum(D0, D1), torch.full_like(D0, float("inf")))
    j_of_i, i_of_j = _argmin(D, 1, rule), _argmin(D, 0, rule)
    rows, cols = torch.arange(M, device=D.device), torch.arange(N, device=D.device)
    hit0 = (i_of_j[j_of_i] == rows) & (D[rows, j_of_i] < pos_th**2)
    hit1 = (j_of_i[i_of_j] == cols) & (D[i_of_j, cols] < pos_th**2)
    if rule == "masked_d0_negatives":
        D0 = torch.where(both, D0, torch.full_like(D0, float("inf")))
        D1 = torch.where(both, D1, torch.full_like(D1, float("inf")))
    far0 = (D0.min(1).values > neg_th**2) & valid0
    far1 = (D1.min(0).values > neg_th**2) & valid1
    m0 = torch.where(hit0, j_of_i, torch.full_like(j_of_i, -2))
    m1 = torch.where(hit1, i_of_j, torch.full_like(i_of_j, -2))
    out["matches0"] = torch.where(far0, torch.full_like(m0, -1), m0)
    out["matches1"] = torch.where(far1, torch.full_like(m1, -1), m1)
    return out


# ---- metrics ---------------------------------------------------------------------------------------------------------
def _mean(flags):
    return float(flags.float().mean()) if flags.numel() else 0.0


def reprojection_errors(kp0, kp1, matches0, depth0, depth1, cam0, model0, cam1, model1, T_0to1, T_1to0=None):
    """Per predicted match of ONE pair: half the sum of the two pixel distances between a point and its partner's
    projection, and whether both end points have valid depth.  -> (err [n], valid [n])"""
    if T_1to0 is None:
        T_1to0 = invert_pose(T_0to1)
    sel = matches0 > -1
    a, b = kp0[sel], kp1[matches0[sel]]
    _, va, pa, _ = pose_project(a, depth0, cam0, model0, cam1, model1, T_0to1)
    _, vb, pb, _ = pose_project(b, depth1, cam1, model1, cam0, model0, T_1to0)
    err = 0.5 * (torch.sqrt(((pa - b) ** 2).sum(-1)) + torch.sqrt(((pb - a) ** 2).sum(-1)))
    return err, va & vb


def depth_metrics(kp0, kp1, matches0, depth0, depth1, cam0, model0, cam1, model1, T_0to1, T_1to0=None, pos_th=3.0,
                  neg_th=5.0, rule=None):
    """Batched inputs ([B,...]) -> ([B,7] float64 on the CPU: reproj_prec@1/3/5px, covisible, covisible_percent,
    gt_match_recall, gt_match_precision; gt matches0 [B,M]; gt matches1 [B,N])."""
    table, g0, g1 = [], [], []
    for b in range(kp0.shape[0]):
        Tinv = invert_pose(T_0to1[b]) if T_1to0 is None else T_1to0[b]
        err, valid = reprojection_errors(kp0[b], kp1[b], matches0[b], depth0[b], depth1[b], cam0[b], model0, cam1[b],
                                         model1, T_0to1[b], Tinv)
        e = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)[valid]
        gt = gt_matches(kp0[b], kp1[b], depth0[b], depth1[b], cam0[b], model0, cam1[b], model1, T_0to1[b], Tinv, pos_th,
                        neg_th, rule)
        m, g = matches0[b], gt["matches0"]
        agree = m == g
        rec_set, prec_set = g > -1, (m > -1) & (g >= -1)
        table.append([_mean(e < 1), _mean(e < 3), _mean(e < 5), float(valid.sum()), _mean(valid) * 100.0,
                      float((agree & rec_set).sum()) / (1e-8 + float(rec_set.sum())),
                      float((agree & prec_set).sum()) / (1e-8 + float(prec_set.sum()))])
        g0.append(g)
        g1.append(gt["matches1"])
    return torch.tensor(table, dtype=torch.float64).reshape(-1, 7), torch.stack(g0), torch.stack(g1)


def essential(T):
    """[t]x R"""
    t = T[9:]
    z = torch.zeros_like(t[0])
    return torch.stack([z, -t[2], t[1], t[2], z, -t[0], -t[1], t[0], z]).reshape(3, 3) @ rot(T)


def epipolar_errors(a, b, cam0, model0, cam1, model1, T_0to1):
    """Symmetric epipolar distance (not squared) of matched pixels a [n,2] <-> b [n,2] on their z = 1 rays:
    |b^T E a| (1 / |E a|_xy + 1 / |E^T b|_xy) / 2 with both squared norms floored at 1e-6."""
    E = essential(T_0to1)
    ax, ay = pixel_to_ray(cam0, model0, a[:, 0], a[:, 1])
    bx, by = pixel_to_ray(cam1, model1, b[:, 0], b[:, 1])
    A = torch.stack([ax, ay, torch.ones_like(ax)], -1)
    Bp = torch.stack([bx, by, torch.ones_like(bx)], -1)
    Ea, Etb = A @ E.t(), Bp @ E
    s = (Bp * Ea).sum(-1).abs()
    na = (Ea[:, 0] ** 2 + Ea[:, 1] ** 2).clamp(min=1e-6)
    nb = (Etb[:, 0] ** 2 + Etb[:, 1] ** 2).clamp(min=1e-6)
    return s * (1 / na.sqrt() + 1 / nb.sqrt()) / 2


def epipolar_metrics(kp0, kp1, matches0, cam0, model0, cam1, model1, T_0to1):
    """Batched inputs -> [B,5] float64 on the CPU: epi_prec@1e-4/5e-4/1e-3, num_matches, num_keypoints."""
    table = []
    for b in range(kp0.shape[0]):
        sel = matches0[b] > -1
        err = epipolar_errors(kp0[b][sel], kp1[b][matches0[b][sel]], cam0[b], model0, cam1[b], model1, T_0to1[b])
        table.append([_mean(err < 1e-4), _mean(err < 5e-4), _mean(err < 1e-3), float(sel.sum()),
                      (kp0.shape[1] + kp1.shape[1]) / 2.0])
    return torch.tensor(table, dtype=torch.float64).reshape(-1, 5)


def relative_pose_error(T_gt, R, t, ignore_gt_t_thr=0.0):
    """Angles in degrees between the translation directions (sign-free: an essential matrix fixes t up to sign) and
    between the rotations, of an estimate (R, t) and the true pose [12]: acos of the cosines, in float64.
    -> (t_err, r_err)"""
    T_gt, R, t = T_gt.double(), R.double(), t.double()
    t_gt = T_gt[9:]
    c = (t * t_gt).sum() / torch.clamp(t.norm() * t_gt.norm(), min=1e-10)
    t_err = torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0)))
    t_err = torch.minimum(t_err, 180 - t_err)
    if t_gt.norm() < ignore_gt_t_thr:
        t_err = torch.zeros_like(t_err)
    c = ((R.t() @ rot(T_gt)).trace() - 1) / 2
    return t_err, torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0)).abs())


# ---- the fixture: what it covers and whether every decision in it is clear of rounding ------------------------------
BAND = 1e-3


def _case_matrices(fx, c):
    import numpy as np

    kp0, kp1 = fx["kp0"][c].astype(np.float64), fx["kp1"][c].astype(np.float64)
    p01, p10 = fx["proj_0to1_f64"][c], fx["proj_1to0_f64"][c]
    with np.errstate(invalid="ignore"):
        D0 = ((p01[:, None] - kp1[None]) ** 2).sum(-1)
        D1 = ((kp0[:, None] - p10[None]) ** 2).sum(-1)
    both = fx["visible0"][c][:, None] & fx["visible1"][c][None]
    return D0, D1, np.where(both, np.maximum(D0, D1), np.inf)


def _two_smallest(D, axis, twins=None):
    """(smallest, second smallest) along `axis`; with `twins` (two indices holding the same key point) also whether
    the two are exactly equal AND sit at the twins: the planted exact ties."""
    import numpy as np

    D = D if axis == 1 else D.T
    order = np.argsort(D, axis=1, kind="stable")[:, :2]
    best, second = np.take_along_axis(D, order[:, :1], 1)[:, 0], np.take_along_axis(D, order[:, 1:2], 1)[:, 0]
    if twins is None:
        return best, second
    planted = (best == second) & (np.sort(order, 1) == np.sort(np.asarray(twins))[None]).all(1)
    return best, second, planted


def _cell_status(depth, iy, ix):
    """0 valid, 1 hole, 2 outside"""
    h, w = depth.shape
    if not (0 <= iy < h and 0 <= ix < w):
        return 2
    return 0 if depth[iy, ix] > 0 else 1


def _sampling_undecided(kp, depth):
    return int(_sampling_undecided_mask(kp, depth).sum())


def _sampling_undecided_mask(kp, depth):
    """Per key point: whether the cells its depth sample reads depend on rounding AND one of them is a hole or outside."""
    import numpy as np

    mask = np.zeros(len(kp), dtype=bool)
    for q, (x, y) in enumerate(kp.astype(np.float64)):
        fx_, fy_ = x - 0.5, y - 0.5  # source index of the sample
        near_lin = [abs(v - round(v)) < BAND for v in (fx_, fy_)]      # pixel coordinate at k + 0.5
        near_nn = [abs(v - 0.5 - round(v - 0.5)) < BAND for v in (fx_, fy_)]  # pixel coordinate at k
        if not (any(near_lin) or any(near_nn)):
            continue
        cols = range(int(round(fx_)) - 1, int(round(fx_)) + 2) if near_lin[0] else range(int(np.floor(fx_)), int(np.floor(fx_)) + 2)
        rows = range(int(round(fy_)) - 1, int(round(fy_)) + 2) if near_lin[1] else range(int(np.floor(fy_)), int(np.floor(fy_)) + 2)
        status = [_cell_status(depth, r, c) for r in rows for c in cols]
        if any(near_lin) and any(status):
            mask[q] = True  # the bilinear footprint itself depends on rounding and touches a hole or the outside
        elif any(near_nn) and 1 in status:
            mask[q] = True  # bilinear is NaN for certain, so the nearest pixel decides, and which one depends on rounding
    return mask


def undecidable_counts(fx):
    """Fixture arrays (numpy, stacked over the cases) -> how many reference values lie within a rounding error of a
    decision, per rule.  The float64 evaluation of the reference is the measure.  All must be 0."""
    import numpy as np

    n = {"reproj_threshold": 0, "epipolar_threshold": 0, "match_threshold": 0, "argmin_margin": 0, "image_bound": 0,
         "depth_sign": 0, "sampling_cell": 0}
    for c in range(len(fx["kp0"])):
        nm = int((fx["matches0"][c] > -1).sum())
        err = fx["reproj_err_f64"][c][:nm][fx["reproj_valid"][c][:nm]]
        err = err[np.isfinite(err)]
        n["reproj_threshold"] += int(sum((np.abs(err - th) < BAND).sum() for th in (1, 3, 5)))
        epi = fx["epi_err_f64"][c][:nm]
        n["epipolar_threshold"] += int(sum((np.abs(epi - th) < BAND * th).sum() for th in (1e-4, 5e-4, 1e-3)))
        D0, D1, D = _case_matrices(fx, c)
        for axis, Dn, twins in ((1, D0, fx["dup_kp1"][c]), (0, D1, fx["dup_kp0"][c])):
            best, second, planted = _two_smallest(D, axis, twins)
            ok = np.isfinite(best)
            n["match_threshold"] += int((np.abs(np.sqrt(best[ok]) - 3.0) < BAND).sum())
            with np.errstate(invalid="ignore"):
                dmin = Dn.min(axis)
            dmin = dmin[np.isfinite(dmin)]
            n["match_threshold"] += int((np.abs(np.sqrt(dmin) - 5.0) < BAND).sum())
            close = ok & (second - np.where(ok, best, 0) < BAND * (1 + np.where(ok, best, 0)))
            close &= ~planted  # exact ties between the two copies of a duplicated key point: decided by the index rule
            n["argmin_margin"] += int(close.sum())
        for proj, cam in ((fx["proj_0to1_f64"][c], fx["cam1"][c]), (fx["proj_1to0_f64"][c], fx["cam0"][c])):
            for a in (0, 1):
                v = proj[:, a][np.isfinite(proj[:, a])]
                n["image_bound"] += int(((np.abs(v) < BAND) | (np.abs(v - (cam[a] - 1)) < BAND)).sum())
        for z in (fx["p3d_1_f64"][c][:, 2], fx["p3d_0_f64"][c][:, 2]):
            n["depth_sign"] += int((np.abs(z - Z_MIN) < 1e-5).sum())
        n["sampling_cell"] += _sampling_undecided(fx["kp0"][c], fx["depth0"][c]) + _sampling_undecided(fx["kp1"][c], fx["depth1"][c])
    return n


def coverage(fx):
    """How many fixture elements exercise each special case the fixture is there for.  All must be > 0."""
    import numpy as np

    n = {"err<1": 0, "err1-3": 0, "err3-5": 0, "err>5": 0, "in_hole": 0, "nearest_used": 0, "border_x0": 0,
         "border_xmax": 0, "outside_view1": 0, "behind_camera1": 0, "beyond_limit": 0, "last_pixel": 0, "tie_row": 0,
         "tie_col": 0, "gt_match": 0, "gt_unmatched": 0, "gt_ignore": 0, "valid_not_visible_near": 0}
    for c in range(len(fx["kp0"])):
        nm = int((fx["matches0"][c] > -1).sum())
        err = fx["reproj_err_f64"][c][:nm][fx["reproj_valid"][c][:nm]]
        for key, lo, hi in (("err<1", 0, 1), ("err1-3", 1, 3), ("err3-5", 3, 5), ("err>5", 5, np.inf)):
            n[key] += int(((err >= lo) & (err < hi)).sum())
        kp0, depth0, w = fx["kp0"][c], fx["depth0"][c], fx["cam0"][c][0]
        n["in_hole"] += int((~fx["valid0"][c]).sum())
        for (x, y), valid in zip(kp0, fx["valid0"][c]):  # valid although the bilinear footprint holds a hole
            x0, y0 = int(np.floor(x - 0.5)), int(np.floor(y - 0.5))
            cells = [_cell_status(depth0, r, q) for r in (y0, y0 + 1) for q in (x0, x0 + 1)]
            n["nearest_used"] += int(bool(valid) and 1 in cells)
        n["border_x0"] += int((kp0[:, 0] == 0).sum() + (fx["kp1"][c][:, 0] == 0).sum())
        n["border_xmax"] += int((kp0[:, 0] == w - 1).sum() + (fx["kp1"][c][:, 0] == w - 1).sum())
        z, px = fx["p3d_1_f64"][c][:, 2], fx["proj_0to1_f64"][c]
        cam1 = fx["cam1"][c]
        inside = (px[:, 0] >= 0) & (px[:, 0] <= cam1[0] - 1) & (px[:, 1] >= 0) & (px[:, 1] <= cam1[1] - 1)
        n["outside_view1"] += int((fx["valid0"][c] & (z > Z_MIN) & ~inside).sum())
        n["behind_camera1"] += int((fx["valid0"][c] & (z <= Z_MIN)).sum())
        n["beyond_limit"] += int((fx["valid0"][c] & (z > Z_MIN) & inside & ~fx["visible0"][c]).sum())
        last = ((px[:, 0] > cam1[0] - 1) & (px[:, 0] < cam1[0]) & (px[:, 1] >= 0) & (px[:, 1] <= cam1[1] - 1)) | \
               ((px[:, 1] > cam1[1] - 1) & (px[:, 1] < cam1[1]) & (px[:, 0] >= 0) & (px[:, 0] <= cam1[0] - 1))
        n["last_pixel"] += int((fx["valid0"][c] & (z > Z_MIN) & last).sum())
        D0, D1, D = _case_matrices(fx, c)
        best, second = _two_smallest(D, 1)
        n["tie_row"] += int(np.isfinite(best[fx["dup_row"][c]]) and best[fx["dup_row"][c]] == second[fx["dup_row"][c]]
                            and fx["gt_matches0"][c][fx["dup_row"][c]] > -1)
        best, second = _two_smallest(D, 0)
        n["tie_col"] += int(np.isfinite(best[fx["dup_col"][c]]) and best[fx["dup_col"][c]] == second[fx["dup_col"][c]]
                            and fx["gt_matches1"][c][fx["dup_col"][c]] > -1)
        g = fx["gt_matches0"][c]
        n["gt_match"] += int((g > -1).sum())
        n["gt_unmatched"] += int((g == -1).sum())
        n["gt_ignore"] += int((g == -2).sum())
        with np.errstate(invalid="ignore"):
            near = D0.min(1) < 25.0  # a neighbour within neg_th without the visibility mask ...
        n["valid_not_visible_near"] += int((fx["valid0"][c] & near & ~(np.isfinite(D).any(1)) & (g == -2)).sum())  # ... only
    return n


# ---- the same rules for ARBITRARY inputs: which key points and matches a float32 evaluation may decide differently ----
NEAR_PX = 1.0  # a partner whose own projection is unsure counts as a possible match within pos_th + NEAR_PX


def _unsure_points(kp, depth_i, cam_i, model_i, cam_j, model_j, T_itoj):
    """Per key point of view i (float64 evaluation): its depth sample, its visibility or its projection depends on
    rounding -- the sampling-cell, depth-sign and image-bound rules of `undecidable_counts`."""
    kp, depth_i, cam_i, cam_j, T = kp.double(), depth_i.double(), cam_i.double(), cam_j.double(), T_itoj.double()
    d, valid, proj, _ = pose_project(kp, depth_i, cam_i, model_i, cam_j, model_j, T)
    nx, ny = pixel_to_ray(cam_i, model_i, kp[:, 0], kp[:, 1])
    Z = (torch.stack([nx * d, ny * d, d], -1) @ rot(T).t() + T[9:])[:, 2]
    unsure = torch.from_numpy(_sampling_undecided_mask(kp.numpy(), depth_i.numpy()))
    unsure = unsure | (valid & ((Z - Z_MIN).abs() < 1e-5))
    for a in (0, 1):
        v = proj[:, a]
        unsure = unsure | (valid & torch.isfinite(v) & ((v.abs() < BAND) | ((v - (cam_j[a] - 1)).abs() < BAND)))
    return unsure


def undecided(kp0, kp1, matches0, depth0, depth1, cam0, model0, cam1, model1, T_0to1, T_1to0=None, pos_th=3.0,
              neg_th=5.0):
    """ONE pair, evaluated in float64: which verdicts of `gt_matches` / `reprojection_errors` rest on a decision within a
    rounding error of going the other way (the rules of `undecidable_counts`, per key point instead of per fixture).
    A key point is undecided when its own sample / visibility is unsure (`_unsure_points`); when its best distance is
    within BAND of pos_th or its nearest unmasked neighbour within BAND of neg_th; when the runner-up of its argmin -- or
    of the argmin of its partner's line -- is within BAND (1 + best) of the winner (squared distances) while the winner
    is below pos_th + BAND; or when a point of the other view that is itself unsure lies within pos_th + NEAR_PX of it.
    Candidates with bit-identical coordinates are exempt from the runner-up rule: their distances are equal in any
    arithmetic and the lower index is the answer.  A match is undecided when its error is within BAND of 1, 3 or 5 px
    or one of its end points is unsure.  -> {"undecided0" [M], "undecided1" [N], "undecided_match" [M]} bool"""
    kp0, kp1, depth0, depth1 = kp0.double(), kp1.double(), depth0.double(), depth1.double()
    cam0, cam1, T_0to1 = cam0.double(), cam1.double(), T_0to1.double()
    T_1to0 = invert_pose(T_0to1) if T_1to0 is None else T_1to0.double()
    M, N = kp0.shape[0], kp1.shape[0]
    uns0 = _unsure_points(kp0, depth0, cam0, model0, cam1, model1, T_0to1)
    uns1 = _unsure_points(kp1, depth1, cam1, model1, cam0, model0, T_1to0)
    if M == 0 or N == 0:
        return {"undecided0": torch.zeros(M, dtype=torch.bool), "undecided1": torch.zeros(N, dtype=torch.bool),
                "undecided_match": torch.zeros(M, dtype=torch.bool)}
    _, valid0, p01, vis0 = pose_project(kp0, depth0, cam0, model0, cam1, model1, T_0to1)
    _, valid1, p10, vis1 = pose_project(kp1, depth1, cam1, model1, cam0, model0, T_1to0)
    inf = float("inf")
    D0 = ((p01[:, None] - kp1[None]) ** 2).sum(-1)
    D1 = ((kp0[:, None] - p10[None]) ** 2).sum(-1)
    D = torch.where(vis0[:, None] & vis1[None], torch.maximum(D0, D1), torch.full_like(D0, inf))
    near2 = (pos_th + NEAR_PX) ** 2
    close = torch.minimum(torch.nan_to_num(D0, nan=inf), torch.nan_to_num(D1, nan=inf)) < near2
    by_other0 = (close & uns1[None]).any(1)
    by_other1 = (close & uns0[:, None]).any(0)
    del close
    und, near, arg = [], [], []
    for dim, Dn, kp_other, valid in ((1, D0, kp1, valid0), (0, D1, kp0, valid1)):
        best, idx = D.min(dim)
        twin = (kp_other[None] == kp_other[idx][:, None]).all(-1)  # [this side, other side]
        second = torch.where(twin if dim == 1 else twin.t(), torch.full_like(D, inf), D).min(dim).values
        ok = torch.isfinite(best)
        b = torch.where(ok, best, torch.zeros_like(best))
        near.append(ok & (second - b < BAND * (1 + b)) & (b.sqrt() < pos_th + BAND))
        arg.append(idx)
        dmin = Dn.min(dim).values  # NaN where the point's own projection is
        u = ok & ((b.sqrt() - pos_th).abs() < BAND)
        u = u | (valid & torch.isfinite(dmin) & ((torch.nan_to_num(dmin, nan=0.0).sqrt() - neg_th).abs() < BAND))
        und.append(u)
    und0 = uns0 | by_other0 | und[0] | near[0] | near[1][arg[0]]
    und1 = uns1 | by_other1 | und[1] | near[1] | near[0][arg[1]]
    has = (matches0 > -1) & (matches0 < N)
    j = torch.where(has, matches0, torch.zeros_like(matches0))
    err = 0.5 * (((p01 - kp1[j]) ** 2).sum(-1).sqrt() + ((p10[j] - kp0) ** 2).sum(-1).sqrt())
    at_th = torch.zeros(M, dtype=torch.bool)
    for th in (1.0, 3.0, 5.0):
        at_th = at_th | ((torch.nan_to_num(err, nan=inf) - th).abs() < BAND)
    und_match = has & ((valid0 & valid1[j] & at_th) | uns0 | uns1[j])
    return {"undecided0": und0, "undecided1": und1, "undecided_match": und_match}
