"""Float64 restatement of the GPU five-point RANSAC relative-pose estimator (csrc/relpose.hip, relpose_solver.h;
DESIGN.md "Robust relative pose") and the seeded scenes its tests share.  Test infrastructure only: numpy on the CPU,
step by step the algorithm the kernels run -- ordered compaction of the matches, fp32 bearings through the camera,
the counter-based sampler (`eval_utils.ransac_sample_indices(sample_size=5)`), the five-point solve (null space by
fully pivoted Gauss-Jordan, ten cubic constraints, 10x20 elimination, degree-10 polynomial, Sturm bisection + Newton),
MSAC sums of the squared Sampson distance in correspondence order, argmin by (score, h, k), decomposition with the
cheirality vote, Gauss-Newton local optimisation.  Vectorised over the hypotheses.  The package never imports this."""
import numpy as np

from glue_factory_colon_amd.eval_utils import ransac_sample_indices

SWEEP = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]  # pixels
FOCAL = 500.0
IMAGE_WH = (640.0, 480.0)
# (n key points = M = N, outlier share, noise sigma in pixels, hypotheses): the regimes the tests run, each with
# general depth ("general") and with 70 % of the points on a plane ("plane"), SCENES_PER_ROW scenes of either
REGIMES = [(5, 0.0, 0.0, 256), (6, 0.0, 0.0, 256), (12, 0.0, 0.0, 256), (60, 0.3, 0.0, 512), (257, 0.5, 0.5, 1024),
           (300, 0.6, 0.5, 1024)]
STRUCTURES = ("general", "plane")
SCENES_PER_ROW = 2
# rows with real intrinsics and pixel thresholds: (camera model, regime index)
CAMERA_ROWS = [("PINHOLE", 3), ("OPENCV_FISHEYE", 4)]
FISHEYE_COEFFS = (-0.02, 0.005, -0.001, 0.0002)

PIVOT_EPS, ELIM_EPS = 1e-12, 1e-14
BISECT_ITERS, NEWTON_ITERS, JACOBI_SWEEPS = 52, 4, 12

# ---- measured constants (printed by test_relpose_reference_host.py::test_restatement_on_the_table; seed 0, SWEEP) ----
# Largest pose error (degrees, max of the rotation and translation angles) of the restatement per regime, over both
# structures, all scenes and thresholds.  A minimal n = 5 scene has up to ten exact models: its winner need not be the
# true pose.  The host test bounds the restatement by 1.01 x, the GPU test the kernels by 2 x.
MEASURED_MAX_POSE_ERROR = {0: 101.7, 1: 49.71, 2: 5.30e-05, 3: 5.162, 4: 1.564, 5: 2.678}
MEASURED_MAX_POSE_ERROR_CAMERA = {"PINHOLE": 1.009, "OPENCV_FISHEYE": 0.7727}
# Largest angle (radians) between the models of the two root-finding routes (Sturm + Newton here, companion-matrix
# eigenvalues) on the winning samples of the outlier-free rows, matched root by root.
MEASURED_ROUTE_SPREAD = 2.51e-08
# Largest |difference| of an entry of (R, t) between the two reduction orders of the local optimisation's sums
# (the kernel's strided block order, plain serial order) over every scene and threshold of the table.
MEASURED_REDUCTION_SPREAD = 2.73e-13


# ---- cameras ---------------------------------------------------------------------------------------------------------
def identity_camera():
    return np.array([0, 0, 1, 1, 0, 0, 0, 0, 0, 0], np.float32)


def image2cam_f32(cam, model, xy):
    """ep_image2cam (csrc/eval_common.h) in float32 numpy, operation for operation: [n,2] pixels -> [n,2] float32."""
    cam = np.asarray(cam, np.float32)
    xy = np.asarray(xy, np.float32)
    nx = (xy[:, 0] - cam[4]) / cam[2]
    ny = (xy[:, 1] - cam[5]) / cam[3]
    if model != "OPENCV_FISHEYE":
        return np.stack([nx, ny], 1)
    d0, d1, d2, d3 = cam[6:10]
    one, tiny = np.float32(1), np.float32(1e-12)
    theta_d = np.sqrt(nx * nx + ny * ny)
    theta = theta_d.copy()
    active = theta_d > tiny
    with np.errstate(all="ignore"):
        for _ in range(10):
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            f = theta * (one + d0 * t2 + d1 * t4 + d2 * t6 + d3 * t8) - theta_d
            fp = one + np.float32(3) * d0 * t2 + np.float32(5) * d1 * t4 + np.float32(7) * d2 * t6 + np.float32(9) * d3 * t8
            step = f / fp
            theta = np.where(active, theta - step, theta)
            active = active & (np.abs(step) >= tiny)
        scale = np.where(theta_d > tiny, np.tan(theta) / theta_d, one).astype(np.float32)
    return np.stack([nx * scale, ny * scale], 1)


def distort_kb4(cam, ray):
    """float64 [n,3] camera points -> pixels through the KB4 fisheye model."""
    u = ray[:, :2] / ray[:, 2:]
    r = np.linalg.norm(u, axis=1, keepdims=True)
    th = np.arctan(r)
    t2 = th * th
    k = cam[6:10].astype(np.float64)
    rd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    u = u * np.where(r > 1e-12, rd / np.maximum(r, 1e-300), 1.0)
    return u * cam[2:4] + cam[4:6]


# ---- scenes ----------------------------------------------------------------------------------------------------------
def _rotation(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def make_case(n, outlier_share, sigma, seed, structure="general", model=None, unmatched_share=0.1):
    """A 640 x 480, f = 500 scene: rotation 5-15 degrees, baseline 0.3-0.6, depths 2-6 (structure "plane": 70 % of the
    points on a tilted plane at depth ~4).  M = N = n key points, matches0 a random permutation with `unmatched_share`
    of the rows set to -1; `outlier_share` of the matched rows point at a uniform random position, the others at the
    projection + N(0, sigma px).  model None: key points are stored as float32 BEARINGS with identity cameras (both
    the kernel and the restatement then see identical inputs and thresholds are pixels / FOCAL); "PINHOLE" /
    "OPENCV_FISHEYE": float32 pixels with real intrinsics."""
    w, h = IMAGE_WH
    rng = np.random.default_rng([seed, 77])
    R = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(5, 15)))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * rng.uniform(0.3, 0.6)
    K = np.array([w, h, FOCAL, FOCAL * 1.01, w / 2 + 3.0, h / 2 - 2.0])
    normal = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
    dist = rng.uniform(3.5, 4.5)
    pts0, pts1 = [], []
    while len(pts0) < n:
        px = rng.uniform(0, 1, 2) * np.array([w, h])
        ray = np.array([(px[0] - K[4]) / K[2], (px[1] - K[5]) / K[3], 1.0])
        on_plane = structure == "plane" and (len(pts0) % 10) < 7
        depth = dist / (ray @ normal) if on_plane else rng.uniform(2, 6)
        X1 = R @ (ray * depth) + t
        if not (2.0 <= depth <= 6.0) or X1[2] < 0.5:
            continue
        q = X1[:2] / X1[2]
        p1 = q * K[2:4] + K[4:6]
        if 0 <= p1[0] <= w and 0 <= p1[1] <= h:
            pts0.append(ray[:2])
            pts1.append(q)
    b0, b1 = np.array(pts0).reshape(n, 2), np.array(pts1).reshape(n, 2)  # exact bearings
    perm = rng.permutation(n)
    m0 = perm.astype(np.int64)
    unmatched = rng.permutation(n)[: int(unmatched_share * n)]
    matched = np.setdiff1d(np.arange(n), unmatched)
    outl = rng.permutation(matched)[: int(round(outlier_share * len(matched)))]
    tgt = b1 + rng.normal(0, 1, (n, 2)) * sigma / K[2:4]
    tgt[outl] = (rng.uniform(0, 1, (len(outl), 2)) * np.array([w, h]) - K[4:6]) / K[2:4]
    k1 = np.zeros((n, 2))
    k1[perm] = tgt
    k1[perm[unmatched]] = (rng.uniform(0, 1, (len(unmatched), 2)) * np.array([w, h]) - K[4:6]) / K[2:4]
    m0[unmatched] = -1
    clean = np.ones(n, bool)
    clean[outl] = False
    clean &= m0 >= 0
    if model is None:
        cam = identity_camera()
        kp0, kp1 = b0, k1
    else:
        coeffs = FISHEYE_COEFFS if model == "OPENCV_FISHEYE" else ()
        cam = np.array(list(K) + list(coeffs) + [0.0] * (4 - len(coeffs)), np.float32)
        if model == "OPENCV_FISHEYE":
            hom = lambda b: np.concatenate([b, np.ones((len(b), 1))], 1)
            kp0, kp1 = distort_kb4(cam.astype(np.float64), hom(b0)), distort_kb4(cam.astype(np.float64), hom(k1))
        else:
            kp0, kp1 = b0 * K[2:4] + K[4:6], k1 * K[2:4] + K[4:6]
    return {"kp0": kp0.astype(np.float32), "kp1": kp1.astype(np.float32), "m0": m0, "cam0": cam, "cam1": cam.copy(),
            "model": model or "PINHOLE", "identity": model is None, "R_gt": R, "t_gt": t,
            "T_gt": np.concatenate([R.reshape(9), t]).astype(np.float32), "clean": clean}


def table_cases():
    """The seeded scenes: a list of dicts {row, regime, structure, scene, case, hypotheses, stream_id, camera}."""
    out = []
    row = 0
    for g, (n, share, sigma, hyp) in enumerate(REGIMES):
        for structure in STRUCTURES:
            for k in range(SCENES_PER_ROW):
                out.append({"row": row, "regime": g, "structure": structure, "scene": k, "hypotheses": hyp,
                            "sigma": sigma, "stream_id": 100 * row + k, "camera": None,
                            "case": make_case(n, share, sigma, seed=1000 * row + k, structure=structure)})
            row += 1
    for model, g in CAMERA_ROWS:
        n, share, sigma, hyp = REGIMES[g]
        for k in range(SCENES_PER_ROW):
            out.append({"row": row, "regime": g, "structure": "general", "scene": k, "hypotheses": hyp, "sigma": sigma,
                        "stream_id": 100 * row + k, "camera": model,
                        "case": make_case(n, share, sigma, seed=1000 * row + k, model=model)})
        row += 1
    return out


def thresholds_for(entry, px=SWEEP):
    """What is passed as `ransac_th`: identity-camera rows take normalised units (pixels / FOCAL), camera rows pixels."""
    return [float(np.float32(t / FOCAL)) for t in px] if entry["camera"] is None else [float(t) for t in px]


def delta_for(entry):
    """Width of the band in which the kernel and the restatement may classify a correspondence differently
    (normalised units): identical fp64 inputs for identity cameras; a handful of fp32 roundings in ep_image2cam
    (2e-3 px) for real cameras."""
    return 1e-9 if entry["camera"] is None else 2e-3 / FOCAL


# ---- records ---------------------------------------------------------------------------------------------------------
def records(case):
    """Matches (i, m0[i]) with 0 <= m0[i] < N in ascending i -> ([n,4] float64 rows u0 v0 u1 v1 from fp32 bearings,
    their indices i)."""
    kp0, kp1, m0 = case["kp0"], case["kp1"], case["m0"]
    idx = np.nonzero((m0 > -1) & (m0 < len(kp1)))[0]
    if "bearings" in case:  # fp32 bearings computed elsewhere (the kernel's own image2cam) instead of the mirror below
        a, b = case["bearings"][0][idx], case["bearings"][1][m0[idx]]
        return np.concatenate([a, b], 1).astype(np.float64).reshape(-1, 4), idx
    a = image2cam_f32(case["cam0"], case["model"], kp0[idx].reshape(-1, 2))
    b = image2cam_f32(case["cam1"], case["model"], kp1[m0[idx]].reshape(-1, 2))
    return np.concatenate([a, b], 1).astype(np.float64).reshape(-1, 4), idx


def threshold2(case, th):
    f = lambda c: float(c)
    fm = ((f(case["cam0"][2]) + f(case["cam0"][3])) + (f(case["cam1"][2]) + f(case["cam1"][3]))) * 0.25
    t = float(np.float32(th)) / fm
    return t * t


# ---- five-point solve, vectorised over K samples ------------------------------------------------------------------------
MUL11 = [0, 1, 2, 3, 1, 4, 5, 6, 2, 5, 7, 8, 3, 6, 8, 9]
MUL21 = [0, 1, 2, 3, 1, 4, 5, 6, 2, 5, 7, 8, 3, 6, 8, 9, 4, 10, 11, 12, 5, 11, 13, 14, 6, 12, 14, 15, 7, 13, 16, 17, 8, 14,
         17, 18, 9, 15, 18, 19]
PERM = [0, 10, 1, 4, 2, 3, 11, 12, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 19]


def nullspace(rec):
    """rec [K,5,4] -> (basis [K,4,9] = X, Y, Z, W, ok [K]): Gauss-Jordan with full pivoting, as rp_nullspace."""
    K = len(rec)
    u0, v0, u1, v1 = (rec[:, :, k] for k in range(4))
    A = np.stack([u1 * u0, u1 * v0, u1, v1 * u0, v1 * v0, v1, u0, v0, np.ones_like(u0)], 2)
    perm = np.tile(np.arange(9), (K, 1))
    ok = np.ones(K, bool)
    ar = np.arange(K)
    for r in range(5):
        sub = np.abs(A[:, r:, r:]).reshape(K, -1)
        flat = np.argmax(np.where(np.isnan(sub), -1.0, sub), axis=1)  # first maximum in row-major order
        best = sub[ar, flat]
        pr, pc = r + flat // (9 - r), r + flat % (9 - r)
        ok &= (best > PIVOT_EPS) & np.isfinite(best)
        tmp = A[ar, r].copy(); A[ar, r] = A[ar, pr]; A[ar, pr] = tmp
        tmp = A[ar, :, r].copy(); A[ar, :, r] = A[ar, :, pc]; A[ar, :, pc] = tmp
        tmp = perm[ar, r].copy(); perm[ar, r] = perm[ar, pc]; perm[ar, pc] = tmp
        A[:, r] = A[:, r] * (1.0 / A[:, r, r])[:, None]
        for i in range(5):
            if i != r:
                A[:, i] = A[:, i] - A[:, i, r][:, None] * A[:, r]
    basis = np.zeros((K, 4, 9))
    for k in range(4):
        basis[ar, k, perm[:, 5 + k]] = 1.0
        for i in range(5):
            basis[ar, k, perm[:, i]] = -A[:, i, 5 + k]
    return basis, ok


def _mul11(a, b, s, out):
    for i in range(4):
        for j in range(4):
            out[:, MUL11[i * 4 + j]] += s * (a[:, i] * b[:, j])


def _mul21(q, l, out):
    for a in range(10):
        for b in range(4):
            out[:, MUL21[a * 4 + b]] += q[:, a] * l[:, b]


def constraints(basis):
    """basis [K,4,9] -> the 10x20 constraint matrices [K,10,20], columns in Nister's order (rp_constraints)."""
    K = len(basis)
    E = [basis[:, :, e] for e in range(9)]  # linear polynomials [K,4]
    L = []
    for i in range(3):
        for j in range(i, 3):
            acc = np.zeros((K, 10))
            for k in range(3):
                _mul11(E[i * 3 + k], E[j * 3 + k], 1.0, acc)
            L.append(acc)
    half_tr = 0.5 * ((L[0] + L[3]) + L[5])
    L[0], L[3], L[5] = L[0] - half_tr, L[3] - half_tr, L[5] - half_tr
    LI = [0, 1, 2, 1, 3, 4, 2, 4, 5]
    Mx = np.zeros((K, 10, 20))
    for i in range(3):
        for j in range(3):
            row = np.zeros((K, 20))
            for k in range(3):
                _mul21(L[LI[i * 3 + k]], E[k * 3 + j], row)
            Mx[:, i * 3 + j] = row[:, PERM]
    row = np.zeros((K, 20))
    for a, b, c, d, e in ((1, 5, 2, 4, 6), (2, 3, 0, 5, 7), (0, 4, 1, 3, 8)):
        m2 = np.zeros((K, 10))
        _mul11(E[a], E[b], 1.0, m2)
        _mul11(E[c], E[d], -1.0, m2)
        _mul21(m2, E[e], row)
    Mx[:, 9] = row[:, PERM]
    return Mx


def eliminate(Mx):
    """rp_eliminate: forward elimination with partial pivoting, back substitution into rows 4..9 -> (Mx, ok)."""
    K = len(Mx)
    ar = np.arange(K)
    ok = np.ones(K, bool)
    with np.errstate(all="ignore"):
        for c in range(10):
            col = np.abs(Mx[:, c:, c])
            pr = c + np.argmax(np.where(np.isnan(col), -1.0, col), axis=1)
            best = np.abs(Mx[ar, pr, c])
            ok &= (best > ELIM_EPS) & np.isfinite(best)
            tmp = Mx[ar, c].copy(); Mx[ar, c] = Mx[ar, pr]; Mx[ar, pr] = tmp
            Mx[:, c, c:] = Mx[:, c, c:] * (1.0 / Mx[:, c, c])[:, None]
            for r in range(c + 1, 10):
                Mx[:, r, c:] = Mx[:, r, c:] - Mx[:, r, c][:, None] * Mx[:, c, c:]
        for c in range(9, 4, -1):
            for r in range(4, c):
                Mx[:, r, 10:] = Mx[:, r, 10:] - Mx[:, r, c][:, None] * Mx[:, c, 10:]
    return Mx, ok


def hidden_variable(Mx):
    """-> Bz [K,3,13]: per row the x (4), y (4) and constant (5) polynomials in z, ascending powers."""
    Bz = np.zeros((len(Mx), 3, 13))
    for r in range(3):
        e, f = Mx[:, 4 + 2 * r, 10:], Mx[:, 5 + 2 * r, 10:]
        Bz[:, r] = np.stack([e[:, 2], e[:, 1] - f[:, 2], e[:, 0] - f[:, 1], -f[:, 0],
                             e[:, 5], e[:, 4] - f[:, 5], e[:, 3] - f[:, 4], -f[:, 3],
                             e[:, 9], e[:, 8] - f[:, 9], e[:, 7] - f[:, 8], e[:, 6] - f[:, 7], -f[:, 6]], 1)
    return Bz


def det_poly(Bz):
    K = len(Bz)
    c = np.zeros((K, 11))
    for r, (ra, rb) in enumerate(((1, 2), (2, 0), (0, 1))):
        a, b = Bz[:, ra], Bz[:, rb]
        cof = np.zeros((K, 7))
        for i in range(4):
            for j in range(4):
                cof[:, i + j] += a[:, i] * b[:, 4 + j] - a[:, 4 + i] * b[:, j]
        w = Bz[:, r, 8:]
        for i in range(5):
            for j in range(7):
                c[:, i + j] += w[:, i] * cof[:, j]
    with np.errstate(all="ignore"):
        mx = np.abs(c).max(1)
        ok = (mx > 0) & np.isfinite(mx)
        c = c * (1.0 / mx)[:, None]
    return c, ok


def _horner(c, deg, x):
    """c [K, >deg] ascending, x [K, R] -> [K, R]"""
    v = np.broadcast_to(c[:, deg][:, None], x.shape).copy()
    for k in range(deg - 1, -1, -1):
        v = v * x + c[:, k][:, None]
    return v


def sturm_chain(c):
    K = len(c)
    s = np.zeros((K, 11, 11))
    s[:, 0] = c
    s[:, 1, :10] = c[:, 1:] * np.arange(1, 11)
    with np.errstate(all="ignore"):
        for i in range(2, 11):
            a, b = s[:, i - 2], s[:, i - 1]
            da, db = 12 - i, 11 - i
            r = a.copy()
            q1 = r[:, da] / b[:, db]
            r[:, 1:db + 2] = r[:, 1:db + 2] - q1[:, None] * b[:, :db + 1]
            q0 = r[:, da - 1] / b[:, db]
            r[:, :db + 1] = r[:, :db + 1] - q0[:, None] * b[:, :db + 1]
            mx = np.nanmax(np.abs(np.where(np.isnan(r[:, :db]), 0.0, r[:, :db])), axis=1) if db > 0 else np.zeros(K)
            # the kernel's running maximum passes NaNs over
            sc = np.where((mx > 0) & np.isfinite(mx), 1.0 / np.where(mx > 0, mx, 1.0), 1.0)
            s[:, i, :db] = -(r[:, :db] * sc[:, None])
    return s


def sturm_count(s, x):
    """sign changes of the chain at x [K,R] (zeros and NaNs passed over) -> int [K,R]"""
    changes = np.zeros(x.shape, np.int64)
    last = np.zeros(x.shape, np.int64)
    with np.errstate(all="ignore"):
        for i in range(11):
            v = _horner(s[:, i], 10 - i, x)
            sg = np.where(v > 0, 1, np.where(v < 0, -1, 0))
            changes += (sg != 0) & (last != 0) & (sg != last)
            last = np.where(sg != 0, sg, last)
    return changes


def _unit_to_line(s):
    return s / (1.0 - np.abs(s))


def real_roots(c):
    """-> (roots [K,10] ascending, count [K]): rp_real_roots (bisection of s in x = s / (1 - |s|), no root bound)."""
    S = 1.0 - 2.0 ** -40
    with np.errstate(all="ignore"):
        s = sturm_chain(c)
        ends = np.full((len(c), 1), _unit_to_line(S))
        v_lo = sturm_count(s, -ends)
        nr = np.clip(v_lo[:, 0] - sturm_count(s, ends)[:, 0], 0, 10)
        k1 = np.arange(1, 11)[None, :]
        lo = np.full((len(c), 10), -S)
        hi = np.full((len(c), 10), S)
        for _ in range(BISECT_ITERS):
            mid = 0.5 * (lo + hi)
            up = (v_lo - sturm_count(s, _unit_to_line(mid))) >= k1
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        xlo, xhi = _unit_to_line(lo), _unit_to_line(hi)
        z = _unit_to_line(0.5 * (lo + hi))
        live = np.ones(z.shape, bool)
        for _ in range(NEWTON_ITERS):
            zn = z - _horner(s[:, 0], 10, z) / _horner(s[:, 1], 9, z)
            live &= (zn >= xlo) & (zn <= xhi)
            z = np.where(live, zn, z)
    return z, nr


def real_roots_companion(c):
    """The other route: eigenvalues of the companion matrix, real ones (|imag| <= 1e-9 (1 + |real|)) ascending."""
    out = []
    for row in c:
        if not np.isfinite(row).all() or row[10] == 0:
            out.append(np.zeros(0))
            continue
        ev = np.roots(row[::-1])
        out.append(np.sort(ev.real[np.abs(ev.imag) <= 1e-9 * (1 + np.abs(ev.real))]))
    return out


def models_at_roots(Bz, basis, z):
    """z [K,R] -> (E [K,R,9] unit Frobenius norm, ok [K,R]): rp_model_at_root."""
    with np.errstate(all="ignore"):
        b = np.zeros(z.shape + (3, 3))
        for r in range(3):
            b[..., r, 0] = _horner(Bz[:, r, 0:4], 3, z)
            b[..., r, 1] = _horner(Bz[:, r, 4:8], 3, z)
            b[..., r, 2] = _horner(Bz[:, r, 8:13], 4, z)
        best = None
        for p, (pa, pb) in enumerate(((0, 1), (0, 2), (1, 2))):
            u, v = b[..., pa, :], b[..., pb, :]
            cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
            cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
            cw = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
            if p == 0:
                best = [cx, cy, cw]
            else:
                take = np.abs(cw) > np.abs(best[2])
                best = [np.where(take, n, o) for n, o in zip((cx, cy, cw), best)]
        x, y = best[0] / best[2], best[1] / best[2]
        E = ((x[..., None] * basis[:, None, 0] + y[..., None] * basis[:, None, 1]) + z[..., None] * basis[:, None, 2]) \
            + basis[:, None, 3]
        n2 = np.zeros(z.shape)
        for e in range(9):
            n2 = n2 + E[..., e] * E[..., e]
        E = E * (1.0 / np.sqrt(n2))[..., None]
    return E, np.isfinite(E).all(-1)


def five_point(rec, route="sturm"):
    """rec [K,5,4] -> (E [K,10,9], ok [K,10]): slot k = the k-th real root."""
    rec = np.asarray(rec, np.float64)
    K = len(rec)
    fin = np.isfinite(rec).all((1, 2))
    safe = np.where(fin[:, None, None], rec, 0.0)
    with np.errstate(all="ignore"):
        basis, ok = nullspace(safe)
        Mx, ok2 = eliminate(constraints(basis))
        Bz = hidden_variable(Mx)
        c, ok3 = det_poly(Bz)
        good = fin & ok & ok2 & ok3
        if route == "sturm":
            z, nr = real_roots(c)
        else:
            z, nr = np.zeros((K, 10)), np.zeros(K, np.int64)
            for i, r in enumerate(real_roots_companion(c)):
                nr[i] = min(len(r), 10)
                z[i, :nr[i]] = r[:nr[i]]
        E, eok = models_at_roots(Bz, basis, z)
    eok &= good[:, None] & (np.arange(10)[None, :] < nr[:, None])
    return np.where(eok[..., None], E, 0.0), eok


# ---- residual, scores --------------------------------------------------------------------------------------------------
def sampson2(E, rec):
    """models E [...,9], records [n,4] -> [...,n] squared Sampson distance (rp_sampson2; inf / NaN on a zero denominator)."""
    E = np.asarray(E, np.float64)[..., None, :]
    u0, v0, u1, v1 = (rec[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        a0 = (E[..., 0] * u0 + E[..., 1] * v0) + E[..., 2]
        a1 = (E[..., 3] * u0 + E[..., 4] * v0) + E[..., 5]
        a2 = (E[..., 6] * u0 + E[..., 7] * v0) + E[..., 8]
        b0 = (E[..., 0] * u1 + E[..., 3] * v1) + E[..., 6]
        b1 = (E[..., 1] * u1 + E[..., 4] * v1) + E[..., 7]
        r = (u1 * a0 + v1 * a1) + a2
        den = (a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1)
        return (r * r) / den


def msac_serial(r2, t2):
    """sum of min(r2, t2) in correspondence order (a running sum); NaN counts as t2."""
    with np.errstate(all="ignore"):
        v = np.where(r2 < t2, r2, t2)
    if v.shape[-1] == 0:
        return np.zeros(v.shape[:-1])
    return np.cumsum(v, axis=-1)[..., -1]


def block_sum(v, order="block"):
    """Sum of v [n, ...] over n: "block" = the kernel's order (256 thread-strided serial partial sums, xor butterfly
    32..1 inside each wave of 64, then ((w0 + w1) + w2) + w3); "serial" = one running sum."""
    v = np.asarray(v, np.float64)
    if order == "serial":
        return np.cumsum(v, axis=0)[-1] if len(v) else np.zeros(v.shape[1:])
    part = np.zeros((256,) + v.shape[1:])
    for start in range(0, len(v), 256):
        chunk = v[start:start + 256]
        part[:len(chunk)] += chunk
    w = part.reshape((4, 64) + v.shape[1:])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def msac_block(E, rec, t2, order="block"):
    r2 = sampson2(E, rec)
    with np.errstate(all="ignore"):
        return float(block_sum(np.where(r2 < t2, r2, t2), order))


# ---- decomposition, cheirality, local optimisation -------------------------------------------------------------------------
def _normalise(a):
    return a * (1.0 / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def essential(R, t):
    R = R.reshape(3, 3)
    return np.stack([t[1] * R[2] - t[2] * R[1], t[2] * R[0] - t[0] * R[2], t[0] * R[1] - t[1] * R[0]]).reshape(9)


def decompose(E):
    """rp_decompose: the four (R, t) candidates in the kernel's order."""
    E = E.reshape(3, 3)
    A = np.array([[(E[0, i] * E[0, j] + E[1, i] * E[1, j]) + E[2, i] * E[2, j] for j in range(3)] for i in range(3)])
    V = np.eye(3)
    old = np.seterr(all="ignore")  # a tiny off-diagonal entry overflows theta^2, as in the kernel: the rotation is then 0
    for _ in range(JACOBI_SWEEPS):
        for p in range(2):
            for r in range(p + 1, 3):
                apq = A[p, r]
                if not abs(apq) > 1e-300:
                    continue
                theta = (A[r, r] - A[p, p]) / (2.0 * apq)
                tt = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(tt * tt + 1.0)
                s = tt * c
                for M_ in (A, None, V):
                    if M_ is None:
                        apk, ark = A[p].copy(), A[r].copy()
                        A[p], A[r] = c * apk - s * ark, s * apk + c * ark
                    else:
                        kp, kr = M_[:, p].copy(), M_[:, r].copy()
                        M_[:, p], M_[:, r] = c * kp - s * kr, s * kp + c * kr
    np.seterr(**old)
    d = np.diag(A)
    i1 = 0
    for k in (1, 2):
        if d[k] > d[i1]:
            i1 = k
    i2 = -1
    for k in range(3):
        if k != i1 and (i2 < 0 or d[k] > d[i2]):
            i2 = k
    v1 = _normalise(V[:, i1].copy())
    v2 = V[:, i2].copy()
    v2 = _normalise(v2 - _dot(v1, v2) * v1)
    v3 = np.cross(v1, v2)
    u1 = np.array([_dot(E[k], v1) for k in range(3)])
    u2 = np.array([_dot(E[k], v2) for k in range(3)])
    u1 = _normalise(u1)
    u2 = _normalise(u2 - _dot(u1, u2) * u1)
    u3 = np.cross(u1, u2)
    out = []
    for cnd in range(4):
        sw, st = (1.0 if cnd < 2 else -1.0), (-1.0 if cnd & 1 else 1.0)
        R = sw * (np.outer(u2, v1) - np.outer(u1, v2)) + np.outer(u3, v3)
        out.append((R, st * u3))
    return out


def cheiral(R, t, rec):
    """rp_cheiral for records [n,4] -> bool [n]"""
    q0 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    q1 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    p = np.stack([(R[k, 0] * q0[:, 0] + R[k, 1] * q0[:, 1]) + R[k, 2] for k in range(3)], 1)
    pxq = np.cross(p, q1)
    n0 = -_dot(np.cross(t[None], q1).T, pxq.T)
    n1 = -_dot(np.cross(t[None], p).T, pxq.T)
    return (n0 > 0) & (n1 > 0)


def tangent(t):
    j = 0
    for k in (1, 2):
        if abs(t[k]) < abs(t[j]):
            j = k
    e = np.zeros(3)
    e[j] = 1.0
    b3 = _normalise(np.cross(t, e))
    return b3, np.cross(t, b3)


def gn_terms(R, t, E, b3, b4, rec):
    """Per record the 20 terms of rp_gn_accumulate -> [n,20]."""
    u0, v0, u1, v1 = rec.T
    a0 = (E[0] * u0 + E[1] * v0) + E[2]
    a1 = (E[3] * u0 + E[4] * v0) + E[5]
    a2 = (E[6] * u0 + E[7] * v0) + E[8]
    e0 = (E[0] * u1 + E[3] * v1) + E[6]
    e1 = (E[1] * u1 + E[4] * v1) + E[7]
    r = (u1 * a0 + v1 * a1) + a2
    w = 1.0 / np.sqrt((a0 * a0 + a1 * a1) + (e0 * e0 + e1 * e1))
    p = np.stack([(R[k, 0] * u0 + R[k, 1] * v0) + R[k, 2] for k in range(3)], 1)
    q1 = np.stack([u1, v1, np.ones_like(u1)], 1)
    c = np.cross(q1, t[None])
    jw = np.cross(p, c)
    J = np.stack([w * jw[:, 0], w * jw[:, 1], w * jw[:, 2], w * _dot(q1.T, np.cross(b3[None], p).T),
                  w * _dot(q1.T, np.cross(b4[None], p).T)], 1)
    rho = w * r
    cols = [J[:, i] * J[:, j] for i in range(5) for j in range(i, 5)] + [J[:, i] * rho for i in range(5)]
    return np.stack(cols, 1) if len(rec) else np.zeros((0, 20))


def gn_update(acc, b3, b4, R, t):
    """rp_gn_update -> (R, t) or None."""
    L = np.zeros((5, 5))
    q = 0
    for i in range(5):
        for j in range(i, 5):
            L[j, i] = acc[q]
            q += 1
    with np.errstate(all="ignore"):
        for j in range(5):
            s = L[j, j]
            for k in range(j):
                s -= L[j, k] * L[j, k]
            if not (s > 0.0) or not np.isfinite(s):
                return None
            dj = np.sqrt(s)
            L[j, j] = dj
            for i in range(j + 1, 5):
                v = L[i, j]
                for k in range(j):
                    v -= L[i, k] * L[j, k]
                L[i, j] = v / dj
        d = np.zeros(5)
        for i in range(5):
            v = -acc[15 + i]
            for k in range(i):
                v -= L[i, k] * d[k]
            d[i] = v / L[i, i]
        for i in range(4, -1, -1):
            v = d[i]
            for k in range(i + 1, 5):
                v -= L[k, i] * d[k]
            d[i] = v / L[i, i]
        th2 = _dot(d, d)
        th = np.sqrt(th2)
        A = 1.0 - th2 / 6.0 if th < 1e-4 else np.sin(th) / th
        B = 0.5 - th2 / 24.0 if th < 1e-4 else (1.0 - np.cos(th)) / th2
        Kx = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
        X = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                k2 = (Kx[i, 0] * Kx[0, j] + Kx[i, 1] * Kx[1, j]) + Kx[i, 2] * Kx[2, j]
                X[i, j] = ((1.0 if i == j else 0.0) + A * Kx[i, j]) + B * k2
        Rn = np.array([[(X[i, 0] * R[0, j] + X[i, 1] * R[1, j]) + X[i, 2] * R[2, j] for j in range(3)] for i in range(3)])
        tn = _normalise((t + d[3] * b3) + d[4] * b4)
    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
        return None
    return Rn, tn


def pose_error(R, t, R_gt, t_gt, ignore_gt_t_thr=0.0):
    """(r_err, t_err) in degrees, the fp64 atan2 expressions of eval_utils.relative_pose_error."""
    cx = np.cross(t, t_gt)
    te = np.degrees(np.arctan2(np.sqrt(_dot(cx, cx)), _dot(t, t_gt)))
    te = min(te, 180.0 - te)
    if np.sqrt(_dot(t_gt, t_gt)) < ignore_gt_t_thr:
        te = 0.0
    D = R.T @ R_gt
    ax = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(np.sqrt(_dot(ax, ax)) / 2.0, (np.trace(D) - 1.0) / 2.0))), float(te)


def refine(E_min, rec, t2, lo_iters=3, order="block"):
    """Decomposition, cheirality vote and local optimisation of one winner -> (R, t, E, accepted scores)."""
    cands = decompose(E_min)
    with np.errstate(all="ignore"):
        inl = sampson2(E_min, rec) < t2
    votes = [float(block_sum(np.where(inl, cheiral(R, t, rec), False).astype(np.float64), order)) for R, t in cands]
    win = 0
    for k in range(1, 4):
        if votes[k] > votes[win]:
            win = k
    R, t = cands[win]
    cur = essential(R, t)
    cur_score = msac_block(cur, rec, t2, order)
    trace = [cur_score]
    for _ in range(lo_iters):
        b3, b4 = tangent(t)
        with np.errstate(all="ignore"):
            inl = sampson2(cur, rec) < t2
            acc = block_sum(np.where(inl[:, None], gn_terms(R, t, cur, b3, b4, rec), 0.0), order)
        upd = gn_update(acc, b3, b4, R, t)
        if upd is None:
            break
        cand = essential(*upd)
        cand_score = msac_block(cand, rec, t2, order)
        if not cand_score < cur_score:
            break
        (R, t), cur, cur_score = upd, cand, cand_score
        trace.append(cur_score)
    return R, t, cur, trace


def sign_fix(E):
    big = int(np.argmax(np.abs(E)))  # the first largest
    return -E if E[big] < 0 else E


# ---- the estimator ---------------------------------------------------------------------------------------------------
def hypotheses(rec, seed, stream_id, num_hypotheses, route="sturm"):
    """All minimal models of a pair: (E [K,10,9], ok [K,10], samples [K,5])."""
    s = ransac_sample_indices(seed, stream_id, len(rec), num_hypotheses, sample_size=5)
    E, ok = five_point(rec[s], route)
    return E, ok, s


def ransac(case, thresholds, num_hypotheses=2048, lo_iters=3, seed=0, stream_id=0, order="block"):
    """The whole estimator for one pair -> a list with one dict per threshold: success, R, t, E, E_minimal,
    best_hypothesis, best_solution, inliers [M] bool, num_inliers, r_err, t_err, scores [K,10] (every model's MSAC
    score, +inf for skipped ones), t2."""
    rec, idx = records(case)
    M, n = len(case["kp0"]), len(rec)
    fail = {"success": False, "R": np.eye(3), "t": np.zeros(3), "E": np.zeros(9), "E_minimal": np.zeros(9),
            "best_hypothesis": -1, "best_solution": -1, "inliers": np.zeros(M, bool), "num_inliers": 0,
            "r_err": float("inf"), "t_err": float("inf"), "scores": None}
    if n < 5:
        return [dict(fail) for _ in thresholds]
    E, ok, samples = hypotheses(rec, seed, stream_id, num_hypotheses)
    r2 = sampson2(E, rec)  # [K,10,n]
    out = []
    for th in thresholds:
        t2 = threshold2(case, th)
        scores = np.where(ok, msac_serial(r2, t2), np.inf)
        flat = int(np.argmin(scores.reshape(-1)))  # first minimum: ties to the lower h, then the lower k
        h, k = divmod(flat, 10)
        if not np.isfinite(scores[h, k]):
            out.append({**fail, "scores": scores, "t2": t2})
            continue
        R, t, cur, trace = refine(E[h, k], rec, t2, lo_iters, order)
        with np.errstate(all="ignore"):
            inl = sampson2(cur, rec) < t2
        inliers = np.zeros(M, bool)
        inliers[idx] = inl
        r_err, t_err = pose_error(R, t, case["T_gt"][:9].astype(np.float64).reshape(3, 3), case["T_gt"][9:].astype(np.float64))
        out.append({"success": True, "R": R, "t": t, "E": cur, "E_minimal": sign_fix(E[h, k]), "best_hypothesis": h,
                    "best_solution": k, "inliers": inliers, "num_inliers": int(inl.sum()), "r_err": r_err,
                    "t_err": t_err, "scores": scores, "t2": t2, "lo_scores": trace, "sample": samples[h]})
    return out
