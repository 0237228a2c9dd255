"""Normative restatement of the package's SIFT (csrc/sift.hip), numpy, float64 unless a dtype is asked for.

Lowe's detector and descriptor with the meaning pycolmap gives the reference's conf keys (reference
gluefactory/models/extractors/sift.py:139-144).  UNPINNED against OpenCV, pycolmap and CudaSift (all absent): what is
held by the tests is that the kernels compute THIS algorithm, not that its key points are those of any library.

Input: one grey plane, clipped to [0, 1].  Scale space: first_octave -1 (2x bilinear up-sample, align-corners false, edge clamp)
or 0; an octave exists while its shorter side is >= 16; S = 3 layers, S + 3 Gaussian levels, sigma0 = 1.6, assumed input
blur 0.5 (x 2 after the up-sample); level s is level s - 1 blurred by sqrt(sigma_s^2 - sigma_{s-1}^2); the next octave is
every second pixel (0, 2, 4, ...; floor(n / 2) of them) of level S.  Taps: radius ceil(4 sigma), float64, normalised,
rounded to fp32; replicate border; rows then columns.

Every decision records its MARGIN (relative distance to the point where it would flip); `detect` returns per key point
the smallest one, and `near_misses` holds the margins of the rejections that were close.
"""
import math

import numpy as np

S = 3
SIGMA0 = 1.6
NOMINAL_BLUR = 0.5
MIN_SIDE = 16
MAX_MOVES = 5
MOVE_AT = 0.6
N_OBINS = 36
PEAK_RATIO = 0.8
MAX_ORI = 4
U24 = 2.0 ** -24
UPSAMPLE_ROUNDINGS = 6  # two lerps of (two products, one sum) each


# ------------------------------------------------------------------------------------------------------ scale space
def level_sigmas():
    return [SIGMA0 * 2.0 ** (s / S) for s in range(S + 3)]


def step_sigmas(first_octave):
    """Incremental blur of level 0 of the first octave, then of levels 1 .. S + 2 of every octave."""
    sig = level_sigmas()
    nominal = NOMINAL_BLUR * (2.0 if first_octave < 0 else 1.0)
    return [math.sqrt(SIGMA0 * SIGMA0 - nominal * nominal)] + [
        math.sqrt(sig[s] * sig[s] - sig[s - 1] * sig[s - 1]) for s in range(1, S + 3)]


def gaussian_taps(sigma):
    r = int(math.ceil(4.0 * sigma))
    x = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def blur(a, taps):
    t = taps.astype(np.float64)
    r = len(t) // 2
    h, w = a.shape
    p = np.pad(a, ((0, 0), (r, r)), mode="edge")
    rows = sum(t[k] * p[:, k: k + w] for k in range(2 * r + 1))
    p = np.pad(rows, ((r, r), (0, 0)), mode="edge")
    return sum(t[k] * p[k: k + h, :] for k in range(2 * r + 1))


def upsample2(a):
    def up(a, axis):
        n = a.shape[axis]
        src = (np.arange(2 * n) + 0.5) / 2.0 - 0.5
        i0 = np.floor(src).astype(int)
        f = src - i0
        lo, hi = np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1)
        shape = [1, 1]
        shape[axis] = -1
        f = f.reshape(shape)
        return np.take(a, lo, axis) * (1.0 - f) + np.take(a, hi, axis) * f

    return up(up(a, 1), 0)


def octave_sizes(h, w, first_octave, num_octaves):
    if first_octave < 0:
        h, w = 2 * h, 2 * w
    out = []
    while len(out) < num_octaves and min(h, w) >= MIN_SIDE:
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def pyramid(image, first_octave=-1, num_octaves=4):
    """-> dict(gauss=[(S+3,h,w) per octave], dog=[(S+2,h,w)], gauss_bound=[(S+3,)], dog_bound=[(S+2,h,w)]).
    The bounds are those of an fp32 evaluation against this one: one level 2 (T + 2) 2^-24 max|x| (T taps, x its input),
    a chain the sum of its steps, a DoG level its two levels' bounds plus 2^-24 |v|."""
    a = np.clip(np.asarray(image, np.float64), 0.0, 1.0)  # the reference's np.clip (sift.py:208)
    sizes = octave_sizes(a.shape[0], a.shape[1], first_octave, num_octaves)
    steps = step_sigmas(first_octave)
    err = 0.0
    if first_octave < 0:
        err = UPSAMPLE_ROUNDINGS * U24 * np.abs(a).max()
        a = upsample2(a)
    gauss, dog, gb, db = [], [], [], []
    base, base_err = a, err
    for o, (h, w) in enumerate(sizes):
        levels, errs = [], []
        if o == 0:
            t = gaussian_taps(steps[0])
            errs.append(base_err + 2 * (len(t) + 2) * U24 * np.abs(base).max())
            levels.append(blur(base, t))
        else:
            levels.append(base)
            errs.append(base_err)
        for s in range(1, S + 3):
            t = gaussian_taps(steps[s])
            errs.append(errs[-1] + 2 * (len(t) + 2) * U24 * np.abs(levels[-1]).max())
            levels.append(blur(levels[-1], t))
        g = np.stack(levels)
        d = g[1:] - g[:-1]
        gauss.append(g)
        dog.append(d)
        gb.append(np.array(errs))
        db.append(np.stack([errs[s] + errs[s + 1] + U24 * np.abs(d[s]) for s in range(S + 2)]))
        base, base_err = g[S][0: 2 * (h // 2): 2, 0: 2 * (w // 2): 2], errs[S]
    return dict(gauss=gauss, dog=dog, gauss_bound=gb, dog_bound=db)


# -------------------------------------------------------------------------------------------------------- detection
def _solve3(A, b):
    """Gaussian elimination with partial pivoting, in the order the kernel uses.  None when singular."""
    A = [list(r) for r in A]
    b = list(b)
    for j in range(3):
        piv, big = j, abs(A[j][j])
        for i in range(j + 1, 3):
            if abs(A[i][j]) > big:
                big, piv = abs(A[i][j]), i
        if big < 1e-30:
            return None
        if piv != j:
            A[j], A[piv] = A[piv], A[j]
            b[j], b[piv] = b[piv], b[j]
        for i in range(j + 1, 3):
            f = A[i][j] / A[j][j]
            for k in range(j, 3):
                A[i][k] -= f * A[j][k]
            b[i] -= f * b[j]
    x = [0.0, 0.0, 0.0]
    for i in (2, 1, 0):
        s = b[i]
        for k in range(i + 1, 3):
            s -= A[i][k] * x[k]
        x[i] = s / A[i][i]
    return x


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def detect(dog, first_octave=-1, detection_threshold=0.0066667, edge_threshold=10.0, near=1e-3, band=None):
    """dog: list of (S+2, h, w) arrays per octave (any float dtype; computed on in float64).
    -> dict(raw=[N,7] (x, y, sigma, score, x_oct, y_oct, sigma_oct), idx=[N,4] (octave, layer, y, x of the integer
    extremum), pos=[N,3] (layer, y, x after the moves), margin=[N], moves=[N], n_candidates, near_misses=[...],
    fates={what became of the candidates}).  Order: idx ascending.
    band: per octave an array like the DoG levels, the absolute error band of each sample (e.g. twice the pyramid chain
    bound).  With it every decision is judged against the band relative to the sample that decides, band / |v|: `risky`
    flags the key points with a margin inside it, and near_misses holds the rejections inside it (not inside `near`)."""
    thr = float(detection_threshold)
    r = float(edge_threshold)
    edge_limit = (r + 1.0) * (r + 1.0) / r
    s0 = 0.5 if first_octave < 0 else 1.0
    raw, idx, pos, margins, near_misses, n_moves, bands = [], [], [], [], [], [], []
    fates = dict(accepted=0, moved=0, singular=0, left_margin=0, not_converged=0, low_contrast=0, edge=0)
    n_cand = 0
    for o, d in enumerate(dog):
        d = np.asarray(d, np.float64)
        L, h, w = d.shape
        if h < 3 or w < 3:
            continue
        c = d[1:-1, 1:-1, 1:-1]
        nb = [d[1 + ds: L - 1 + ds, 1 + dy: h - 1 + dy, 1 + dx: w - 1 + dx]
              for ds in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (ds, dy, dx) != (0, 0, 0)]
        hi, lo = np.maximum.reduce(nb), np.minimum.reduce(nb)
        strong = np.abs(c) > 0.8 * thr
        is_ext = ((c > hi) | (c < lo))
        gap = np.maximum(c - hi, lo - c) / np.maximum(np.abs(c), 1e-300)  # > 0: an extremum, = 0: a tie
        # rejections that were close: a strong sample a hair from being an extremum, an extremum a hair under 0.8 thr
        # (an exact tie, gap = 0, is no near miss: equal fp32 samples are equal on every side)
        rel_band = None if band is None else np.asarray(band[o])[1:-1, 1:-1, 1:-1] / np.maximum(np.abs(c), 1e-300)
        close = strong & ~is_ext & (np.abs(gap) < (near if band is None else rel_band)) & (gap != 0)
        near_misses += list(np.abs(gap[close]))
        weak = is_ext & ~strong & (np.abs(np.abs(c) - 0.8 * thr) < (near * 0.8 * thr if band is None else rel_band * np.abs(c)))
        near_misses += list(np.abs(np.abs(c[weak]) - 0.8 * thr) / (0.8 * thr))
        ls, ys, xs = np.nonzero(is_ext & strong)
        n_cand += len(ls)
        for l0, y0, x0 in zip(ls + 1, ys + 1, xs + 1):
            v0 = d[l0, y0, x0]
            m = min(abs(gap[l0 - 1, y0 - 1, x0 - 1]), _rel(abs(v0), 0.8 * thr))
            near = near if band is None else float(rel_band[l0 - 1, y0 - 1, x0 - 1])
            l, y, x = int(l0), int(y0), int(x0)
            moves, off, ok = 0, None, False
            while True:
                v = d[l, y, x]
                gx = 0.5 * (d[l, y, x + 1] - d[l, y, x - 1])
                gy = 0.5 * (d[l, y + 1, x] - d[l, y - 1, x])
                gs = 0.5 * (d[l + 1, y, x] - d[l - 1, y, x])
                hxx = d[l, y, x + 1] + d[l, y, x - 1] - 2.0 * v
                hyy = d[l, y + 1, x] + d[l, y - 1, x] - 2.0 * v
                hss = d[l + 1, y, x] + d[l - 1, y, x] - 2.0 * v
                hxy = 0.25 * (d[l, y + 1, x + 1] + d[l, y - 1, x - 1] - d[l, y - 1, x + 1] - d[l, y + 1, x - 1])
                hxs = 0.25 * (d[l + 1, y, x + 1] + d[l - 1, y, x - 1] - d[l - 1, y, x + 1] - d[l + 1, y, x - 1])
                hys = 0.25 * (d[l + 1, y + 1, x] + d[l - 1, y - 1, x] - d[l - 1, y + 1, x] - d[l + 1, y - 1, x])
                off = _solve3([[hxx, hxy, hxs], [hxy, hyy, hys], [hxs, hys, hss]], [-gx, -gy, -gs])
                if off is None:
                    fates["singular"] += 1
                    break
                m = min(m, min(_rel(abs(t), MOVE_AT) for t in off))
                mx = (1 if off[0] > MOVE_AT else -1 if off[0] < -MOVE_AT else 0)
                my = (1 if off[1] > MOVE_AT else -1 if off[1] < -MOVE_AT else 0)
                ml = (1 if off[2] > MOVE_AT else -1 if off[2] < -MOVE_AT else 0)
                if mx == 0 and my == 0 and ml == 0:
                    ok = True
                    break
                if moves == MAX_MOVES:
                    fates["not_converged"] += 1
                    break
                moves += 1
                x, y, l = x + mx, y + my, l + ml
                if x < 1 or x > w - 2 or y < 1 or y > h - 2 or l < 1 or l > S:
                    fates["left_margin"] += 1
                    break
            if not ok:
                continue
            val = v + 0.5 * (gx * off[0] + gy * off[1] + gs * off[2])
            score = abs(val)
            tr, det = hxx + hyy, hxx * hyy - hxy * hxy
            m_thr = _rel(score, thr)
            if score < thr:
                fates["low_contrast"] += 1
                if m_thr < near:
                    near_misses.append(m_thr)
                continue
            if not (det > 0.0 and tr * tr / det < edge_limit):
                fates["edge"] += 1
            if not det > 0.0:
                if abs(det) < near * max(abs(hxx * hyy), 1e-300):
                    near_misses.append(abs(det) / max(abs(hxx * hyy), 1e-300))
                continue
            m_edge = _rel(tr * tr / det, edge_limit)
            if not tr * tr / det < edge_limit:
                if m_edge < near:
                    near_misses.append(m_edge)
                continue
            m = min(m, m_thr, m_edge)
            fates["accepted"] += 1
            fates["moved"] += moves > 0
            n_moves.append(moves)
            bands.append(near)
            step = 2.0 ** o
            xo, yo = x + off[0], y + off[1]
            so = SIGMA0 * 2.0 ** ((l + off[2]) / S)
            raw.append([(xo * step + 0.5) * s0, (yo * step + 0.5) * s0, so * step * s0, score, xo, yo, so])
            idx.append([o, int(l0), int(y0), int(x0)])
            pos.append([l, y, x])
            margins.append(m)
    if raw:
        order = sorted(range(len(idx)), key=lambda i: tuple(idx[i]))
        raw, idx = np.array(raw)[order], np.array(idx, np.int64)[order]
        pos, margins = np.array(pos, np.int64)[order], np.array(margins)[order]
        n_moves, bands = np.array(n_moves)[order], np.array(bands)[order]
    else:
        raw, idx, pos, margins = np.zeros((0, 7)), np.zeros((0, 4), np.int64), np.zeros((0, 3), np.int64), np.zeros(0)
    return dict(raw=raw, idx=idx, pos=pos, margin=margins, n_candidates=n_cand, near_misses=np.array(near_misses),
                fates=fates, moves=np.array(n_moves, np.int64), risky=np.array(margins) < np.array(bands, np.float64))


# ------------------------------------------------------------------------------------------------------ orientation
def orientations(level, xo, yo, so, dtype=np.float64):
    """36-bin histogram on one Gaussian level.  -> (angles in (-pi, pi] by ascending bin, at most 4; peak margin)."""
    f = dtype
    g = np.asarray(level, f)
    h, w = g.shape
    xo, yo, so = f(xo), f(yo), f(so)
    sw = f(1.5) * so
    W = int(math.floor(3.0 * 1.5 * float(so) + 0.5))
    xi, yi = int(math.floor(float(xo) + 0.5)), int(math.floor(float(yo) + 0.5))
    ys, xs = np.mgrid[yi - W: yi + W + 1, xi - W: xi + W + 1]
    ok = (xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2)
    ys, xs = ys[ok], xs[ok]
    dx, dy = xs.astype(f) - xo, ys.astype(f) - yo
    r2 = dx * dx + dy * dy
    inside = r2 < f(W * W) + f(0.6)
    ys, xs, r2 = ys[inside], xs[inside], r2[inside]
    gx = f(0.5) * (g[ys, xs + 1] - g[ys, xs - 1])
    gy = f(0.5) * (g[ys + 1, xs] - g[ys - 1, xs])
    mag = np.sqrt(gx * gx + gy * gy)
    ang = np.arctan2(gy, gx)
    ang = np.where(ang < 0, ang + f(2 * math.pi), ang)
    wgt = mag * np.exp(-r2 / (f(2.0) * sw * sw))
    fbin = ang * f(N_OBINS / (2 * math.pi)) - f(0.5)
    b0 = np.floor(fbin)
    rb = fbin - b0
    hist = np.zeros(N_OBINS, np.float64 if f is np.float64 else np.float32)
    b0 = b0.astype(int)
    np.add.at(hist, b0 % N_OBINS, wgt * (f(1.0) - rb))
    np.add.at(hist, (b0 + 1) % N_OBINS, wgt * rb)
    third = f(1.0) / f(3.0)
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) * third
    top = hist.max()
    angles, margin = [], np.inf
    if not top > 0:
        return angles, margin
    for i in range(N_OBINS):
        h0, hm, hp = hist[i], hist[i - 1], hist[(i + 1) % N_OBINS]
        is_max = h0 > hm and h0 > hp
        if is_max or h0 >= PEAK_RATIO * top:
            # margins of the two tests, of the ones that decide
            gap = min(abs(float(h0 - hm)), abs(float(h0 - hp))) / float(top)
            lvl = abs(float(h0) - PEAK_RATIO * float(top)) / float(top)
            if is_max and h0 >= PEAK_RATIO * top:
                margin = min(margin, gap, lvl if h0 != top else np.inf)
            elif is_max:
                margin = min(margin, lvl)
            else:
                margin = min(margin, gap)
        if is_max and h0 >= PEAK_RATIO * top and len(angles) < MAX_ORI:
            di = -f(0.5) * (hp - hm) / (hp + hm - f(2.0) * h0)
            th = f(2 * math.pi) * (f(i) + di + f(0.5)) / f(N_OBINS)
            if th > f(math.pi):
                th -= f(2 * math.pi)
            angles.append(float(th))
    return angles, margin


# ------------------------------------------------------------------------------------------------------- descriptor
def descriptor(level, xo, yo, so, theta, dtype=np.float64):
    """4 x 4 cells x 8 bins, index (cell_y * 4 + cell_x) * 8 + bin; L2, clamp 0.2, L2."""
    f = dtype
    g = np.asarray(level, f)
    h, w = g.shape
    xo, yo, so, theta = f(xo), f(yo), f(so), f(theta)
    sbp = f(3.0) * so
    W = int(math.floor(math.sqrt(2.0) * float(sbp) * 2.5 + 0.5))
    xi, yi = int(math.floor(float(xo) + 0.5)), int(math.floor(float(yo) + 0.5))
    ct, st = np.cos(theta), np.sin(theta)
    ys, xs = np.mgrid[yi - W: yi + W + 1, xi - W: xi + W + 1]
    ok = (xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2)
    ys, xs = ys[ok], xs[ok]
    dx, dy = xs.astype(f) - xo, ys.astype(f) - yo
    gx = f(0.5) * (g[ys, xs + 1] - g[ys, xs - 1])
    gy = f(0.5) * (g[ys + 1, xs] - g[ys - 1, xs])
    mag = np.sqrt(gx * gx + gy * gy)
    ang = np.arctan2(gy, gx) - theta
    two_pi = f(2 * math.pi)
    ang = np.where(ang < 0, ang + two_pi, ang)
    ang = np.where(ang < 0, ang + two_pi, ang)
    ang = np.where(ang >= two_pi, ang - two_pi, ang)
    nx = (ct * dx + st * dy) / sbp
    ny = (-st * dx + ct * dy) / sbp
    nt = ang * f(8.0 / (2 * math.pi))
    wgt = mag * np.exp(-(nx * nx + ny * ny) / f(8.0))  # sigma = 2 cells
    bx, by, bt = np.floor(nx - f(0.5)), np.floor(ny - f(0.5)), np.floor(nt)
    rx, ry, rt = nx - (bx + f(0.5)), ny - (by + f(0.5)), nt - bt
    bx, by, bt = bx.astype(int), by.astype(int), bt.astype(int)
    hist = np.zeros(128, np.float64 if f is np.float64 else np.float32)
    one = f(1.0)
    for ddy in (0, 1):
        for ddx in (0, 1):
            cx, cy = bx + ddx + 2, by + ddy + 2
            keep = (cx >= 0) & (cx < 4) & (cy >= 0) & (cy < 4)
            wxy = wgt * (rx if ddx else one - rx) * (ry if ddy else one - ry)
            for ddt in (0, 1):
                v = wxy * (rt if ddt else one - rt)
                np.add.at(hist, ((cy * 4 + cx) * 8 + (bt + ddt) % 8)[keep], v[keep])
    n = np.sqrt((hist * hist).sum())
    if n > 0:
        hist = hist / n
    hist = np.minimum(hist, f(0.2))
    n = np.sqrt((hist * hist).sum())
    if n > 0:
        hist = hist / n
    return hist


def extract(image, first_octave=-1, num_octaves=4, detection_threshold=0.0066667, edge_threshold=10.0, fp32_levels=True):
    """Whole raw extractor.  With fp32_levels the pyramid is rounded to fp32 between the stages, as on the device.
    -> dict(keypoints [N,2], scales, oris, scores, descriptors [N,128], src (index into the raw list), det, pyr)."""
    pyr = pyramid(image, first_octave, num_octaves)
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if fp32_levels else (lambda a: a)
    det = detect([rnd(d) for d in pyr["dog"]], first_octave, detection_threshold, edge_threshold,
                 band=[2.0 * b for b in pyr["dog_bound"]])
    kp, sc, ori, score, desc, src, omargin = [], [], [], [], [], [], []
    for i, (r, ix, ps) in enumerate(zip(det["raw"], det["idx"], det["pos"])):
        level = rnd(pyr["gauss"][ix[0]][ps[0]])
        angles, m = orientations(level, r[4], r[5], r[6])
        for th in angles:
            kp.append(r[:2]); sc.append(r[2]); score.append(r[3]); ori.append(th); src.append(i); omargin.append(m)
            desc.append(descriptor(level, r[4], r[5], r[6], th))
    return dict(keypoints=np.array(kp).reshape(-1, 2), scales=np.array(sc), oris=np.array(ori), scores=np.array(score),
                descriptors=np.array(desc).reshape(-1, 128), src=np.array(src, np.int64), ori_margin=np.array(omargin),
                det=det, pyr=pyr)


# -------------------------------------------------------------------------------------------------- post-processing
def filter_dog_point(points, scales, angles, image_shape, nms_radius, scores=None):
    """The reference's rule (sift.py:29-62) without torch: -> kept indices, ascending."""
    h, w = image_shape
    ij = np.round(points - 0.5).astype(int).T[::-1]
    s = scales if scores is None else scores
    buf = np.zeros((h, w))
    np.maximum.at(buf, tuple(ij), s)
    keep = np.where(buf[tuple(ij)] == s)[0]
    ij = ij[:, keep]
    buf[:] = np.inf
    o_abs = np.abs(angles[keep])
    np.minimum.at(buf, tuple(ij), o_abs)
    mask = buf[tuple(ij)] == o_abs
    ij, keep = ij[:, mask], keep[mask]
    if nms_radius > 0:
        buf[:] = 0
        buf[tuple(ij)] = s[keep]
        r = nms_radius
        p = np.pad(buf, r, mode="constant", constant_values=-np.inf)
        local = np.maximum.reduce([p[dy: dy + h, dx: dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)])
        keep = keep[(buf == local)[tuple(ij)]]
    return keep


def sift_to_rootsift(x, eps=1e-6):
    x = np.asarray(x, np.float64)
    x = x / np.maximum(np.abs(x).sum(-1, keepdims=True), eps)
    x = np.sqrt(np.maximum(x, eps))
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), eps)


def specular_keep(keypoints, mask, offset=0.5):
    """extractors/utils.py:4-42: all four pixels around the point are True and inside."""
    m = np.asarray(mask).astype(bool)
    m = m.reshape(m.shape[-2:])
    h, w = m.shape
    xy = np.asarray(keypoints) - offset
    x0, x1 = np.floor(xy[:, 0]).astype(int), np.ceil(xy[:, 0]).astype(int)
    y0, y1 = np.floor(xy[:, 1]).astype(int), np.ceil(xy[:, 1]).astype(int)
    inside = (x0 >= 0) & (x1 < w) & (y0 >= 0) & (y1 < h)
    keep = np.zeros(len(xy), bool)
    i = inside
    keep[i] = m[y0[i], x0[i]] & m[y0[i], x1[i]] & m[y1[i], x0[i]] & m[y1[i], x1[i]]
    return keep


def topk_indices(scores, k, scales=None):
    """Indices of the k largest ranking values (score, or score x scale), as a sorted set."""
    rank = np.asarray(scores) if scales is None else np.asarray(scores) * np.asarray(scales)
    if len(rank) <= k:
        return np.arange(len(rank))
    return np.sort(np.argsort(-rank, kind="stable")[:k])


# ---------------------------------------------------------------------------------------------------------- fixtures
def blob_image(h, w, blobs, background=0.5):
    """Gaussians centred on pixel centres: blobs = [(y, x, sigma, amplitude)]."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), background)
    for y, x, s, a in blobs:
        img += a * np.exp(-((ys - y) ** 2 + (xs - x) ** 2) / (2.0 * s * s))
    return img


def textured_image(h, w, seed, n=40, vignette=True):
    """Seeded blobs of mixed size and sign on a smooth ramp inside a black vignette (exactly 0 outside)."""
    g = np.random.RandomState(seed)
    m = min(8, h // 4, w // 4)
    blobs = [(g.randint(m, h - m), g.randint(m, w - m), g.uniform(1.5, 6.0), g.uniform(0.1, 0.35) * g.choice([-1, 1]))
             for _ in range(n)]
    img = blob_image(h, w, blobs, 0.5)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    img += 0.1 * xs / w - 0.05 * ys / h
    img = np.clip(img, 0.0, 1.0)
    if vignette:
        rr = ((ys - (h - 1) / 2) / (h * 0.62)) ** 2 + ((xs - (w - 1) / 2) / (w * 0.62)) ** 2
        img[rr > 1.0] = 0.0
    return img.astype(np.float32)


def e2e_fixture():
    """The end-to-end image and its (first_octave, num_octaves): searched over seeds 1..59 so that at most 2 % of its key
    points have a margin inside twice the pyramid chain bound (1 of 75)."""
    return textured_image(120, 160, 53, n=120), 0, 3


DETECT_SHAPE = (40, 56)  # one octave, first_octave 0
DETECT_THR = 0.0066667


def detect_fixture():
    """A DoG octave (5, 40, 56) fp32 for the stage-isolated detection test: seeded smooth noise, whose candidates meet
    every fate of the refinement (seed 7: one accepted after a move, three leave the margin, two do not converge, fifteen
    fall under the threshold after refinement, one fails the edge test), plus planted cases on cleared ground.
    -> (volume, planted): planted[name] = (layer, y, x)."""
    h, w = DETECT_SHAPE
    g = np.random.RandomState(7)
    v = g.randn(5, h, w)
    for _ in range(2):
        v = (v + np.roll(v, 1, 1) + np.roll(v, -1, 1) + np.roll(v, 1, 2) + np.roll(v, -1, 2)) / 5
    v[1:] = 0.6 * v[1:] + 0.4 * v[:-1]
    v = (v * 0.02).astype(np.float32)
    planted = {}

    def bump(name, y, x, value, l=2):
        v[l - 1: l + 2, y - 3: y + 4, x - 3: x + 4] = 0.0
        v[l - 1: l + 2, y - 1: y + 2, x - 1: x + 2] = 0.5 * value
        v[l, y, x] = value
        planted[name] = (l, y, x)

    thr = DETECT_THR
    bump("under_0.8_thr", 5, 5, 0.79 * thr)       # never a candidate
    bump("over_0.8_thr", 5, 13, 0.81 * thr)       # a candidate, refined |D| = v < thr
    bump("under_thr", 5, 21, 0.99 * thr)          # rejected on contrast
    bump("over_thr", 5, 29, 1.01 * thr)           # accepted, offsets 0
    bump("negative", 5, 37, -1.5 * thr)           # a minimum, accepted
    bump("tie", 13, 5, 0.05)                      # a plateau of two equal samples: neither is strictly greater
    v[2, 13, 6] = v[2, 13, 5]
    planted["tie_twin"] = (2, 13, 6)
    # an elongated ridge with a shallow summit: tr^2 / det far above (r + 1)^2 / r
    v[1:4, 31:38, 14:33] = 0.0
    for x in range(16, 31):
        top = 0.03 * (1.0 - 0.0005 * (x - 23) ** 2)
        v[2, 34, x] = top
        v[2, 33, x] = v[2, 35, x] = v[1, 34, x] = v[3, 34, x] = 0.3 * top
    planted["ridge"] = (2, 34, 23)
    bump("on_margin", 1, 48, 2.0 * thr)           # y = 1: the last row that may hold a key point
    return v.astype(np.float32), planted


STAGE_SHAPE = (64, 80)  # the image behind the orientation and descriptor fixtures, first_octave 0, 2 octaves


def stage_fixture():
    """Gaussian levels (fp32-rounded, as the device holds them) and key-point records for the stage-isolated
    orientation and descriptor tests.  -> (levels: list per octave of (6, h, w) fp32, records [N, 5] float32-rounded
    (x_oct, y_oct, sigma_oct, octave, level)).  The records are the restatement's own detections plus planted ones:
    windows clipped by the level border (orientation and descriptor), the largest sigma of an octave (1.6 * 2^(3.6/3),
    the largest window), and a count that is no multiple of 4 (the waves of a workgroup)."""
    img = textured_image(*STAGE_SHAPE, seed=11, n=30, vignette=False)
    pyr = pyramid(img, 0, 2)
    levels = [g.astype(np.float32) for g in pyr["gauss"]]
    det = detect([d.astype(np.float32) for d in pyr["dog"]], 0)
    rec = [[r[4], r[5], r[6], ix[0], ps[0]] for r, ix, ps in zip(det["raw"], det["idx"], det["pos"])]
    big = SIGMA0 * 2.0 ** (3.6 / S)
    rec += [[2.3, 3.1, 2.0, 0, 1], [77.6, 61.2, 2.4, 0, 2], [20.25, 30.5, big, 0, 3], [12.0, 9.0, big, 1, 3],
            [37.4, 1.2, 1.7, 1, 1]]
    if len(rec) % 4 == 0:
        rec.append([40.0, 32.0, 2.0, 0, 2])
    return levels, np.array(rec, np.float32).astype(np.float64)
