"""Ill-conditioned cases for the fp32 LayerNorm and soft-max kernels: gfc_layernorm_gelu, gfc_linear_layernorm_gelu, the
statistics of gfc_ffn_fused (csrc/lg_misc.hip, csrc/gemm.hip), gfc_attention (csrc/attention.hip) and the 65-way soft-max
of gfc_sp_detector_head (csrc/sp_heads.hip).

Plain torch on the CPU, no GPU import.  Every case carries its inputs, a float64 reference, a per-element bound, an fp32
emulation of the algorithm the kernel implements, and the wrong variants of that algorithm the case is aimed at.
tests/test_conditioning_cases_host.py proves without a GPU that the correct emulation meets every bound and that every
variant misses one by a factor of 100 or more; tests/test_gpu_conditioning.py holds the kernels to the same bounds.

Exactness is the design rule.  Inputs are small integers and powers of two, so the quantity whose conditioning is under
test -- the pre-activation row of a LayerNorm, the logits of a soft-max -- is exactly representable in fp32 whatever the
order of accumulation: every partial sum is an integer (or a multiple of one power of two) far below 2^24.  Each builder
asserts this: the fp32 and the float64 evaluation of that quantity are torch.equal.  The float64 reference therefore
sees the very pre-activations the kernel computes, and the only error left is the arithmetic being pinned.

u = 2^-24 is the unit round-off of fp32 throughout.
"""
import math
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
HEADS = 4
SCALE = 0.125
NAN = float("nan")
INF = float("inf")


def _gen(*key):
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % 2147483647
    return torch.Generator().manual_seed(seed)


def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def worst_ratio(y, ref, tol):
    """max over elements of |y - ref| / tol; NaN or inf in y counts as an infinite error; 0 / 0 (an exact element with a
    zero bound) as 0."""
    err = (y.double() - ref).abs()
    r = torch.where((err == 0) & (tol == 0), torch.zeros_like(err), err / tol)
    return float(r.nan_to_num(nan=INF, posinf=INF).max())


# ============================================================================================== LayerNorm + GELU
# Two launches of M = 133 rows (one full 128-row tile of the fused kernels and a tail of 5), width 512:
#   "offset"  pre-activation = [A0 | A1] W0^T + 4096 with integer A in [-3, 3] and 16 entries of +-1 per row of W0: row
#             mean about 4096, sigma about 8.  sum x^2 is then about 2^33 with an fp32 spacing of 2^10 while the variance
#             it hides is about 64: E[x^2] - mean^2 loses it (0.1 in the output), the two-pass form keeps it.
#             Some rows of the same launch and the same 128-row tile are special:
#     const   A = 0: every column equals 4096, the variance is exactly 0, the output is gelu(beta) -- NaN without eps;
#     spike   every input of the row is +3 or -3 (two rows: +-1), and W0[LN_SPIKE_COL] is all ones over A0: that column
#             sits at +-768 while the others stay within +-48, more than 20 sigma of the row: the statistics under one
#             dominant element and both tails of the GELU (gamma * x_hat near +21 in the rows of +3, -21 in those of -3).
#   "tiny"    bias 0 and A scaled by 2^-10: variance about 6e-5, the order of eps = 1e-5, so that dropping eps, using
#             1e-6 or adding it outside the square root each move the output by more than 0.3.
# The bounds are the suite's own for these kernels -- 2e-5 on the LayerNorm + GELU output (O(1) values of exact
# pre-activations: |x_hat| <= 23, gamma <= 1.5, so one fp32 rounding of the largest output is 2e-6, the statistics add a
# few u relative), 3e-5 on the FFN output -- under the condition the host test asserts: at most 1/100 of the error of
# every variant aimed at the case.  One pair cannot meet it: `spike` at the FFN output.  The one-pass variance is off by at
# most 2 of 1295 there, which moves the spike column of the hidden activation by 0.007 (364 x the 2e-5 bound), and W3's
# entries of about 0.04 pass 1e-3 of that on: 34 x the 3e-5 bound.  The FFN is held to `spike` through the hidden activation:
# the GPU test demands that gfc_ffn_fused equals gfc_linear_layernorm_gelu + gfc_linear bit for bit.
LN_FFN_CONDITION_CASES = ("offset", "const", "tiny")
LN_M, LN_W = 133, 512
LN_TOL, FFN_TOL = 2e-5, 3e-5
LN_CONST_ROWS = (7, 64, 130)
LN_SPIKE_ROWS = {20: 3, 21: -3, 99: 1, 100: -1, 131: 3}  # row -> the value of every input of that row
LN_SPIKE_COL = 77
LN_VARIANTS = ("one_pass_var", "no_eps", "eps_1e-6", "eps_outside_sqrt")
# case -> (launch, the variants aimed at it)
LN_CASES = {"offset": ("offset", ("one_pass_var",)), "const": ("offset", ("no_eps",)), "spike": ("offset", ("one_pass_var",)),
            "tiny": ("tiny", ("no_eps", "eps_1e-6", "eps_outside_sqrt"))}
_LN = {}


def ln_rows(case):
    special = sorted(LN_CONST_ROWS + tuple(LN_SPIKE_ROWS))
    return {"offset": [r for r in range(LN_M) if r not in special], "const": list(LN_CONST_ROWS),
            "spike": sorted(LN_SPIKE_ROWS), "tiny": list(range(LN_M))}[case]


def ln_launch(name):
    """The inputs of one launch (built once per process, never modified): a [M, 512] = A0 | A1, w0 [512, 512], b0, gamma,
    beta, w3 [256, 512], b3, the exact pre-activation `pre` and the float64 references `h_ref` (LayerNorm + GELU) and
    `y_ref` (the FFN with its residual A0)."""
    if name in _LN:
        return _LN[name]
    g = _gen("layernorm", name)
    c = types.SimpleNamespace(name=name, M=LN_M)
    a = _randint(g, -3, 3, LN_M, LN_W)
    w0 = torch.zeros(LN_W, LN_W)
    idx = torch.rand(LN_W, LN_W, generator=g).argsort(1)[:, :16]
    w0.scatter_(1, idx, _randint(g, 0, 1, LN_W, 16) * 2 - 1)
    c.gamma, c.beta = torch.rand(LN_W, generator=g) + 0.5, torch.randn(LN_W, generator=g) * 0.2
    c.w3, c.b3 = torch.randn(256, LN_W, generator=g) / LN_W ** 0.5, torch.randn(256, generator=g)
    if name == "offset":
        c.b0 = torch.full((LN_W,), 4096.0)
        w0[LN_SPIKE_COL] = 0
        w0[LN_SPIKE_COL, :256] = 1
        a[list(LN_CONST_ROWS)] = 0
        for r, val in LN_SPIKE_ROWS.items():
            a[r] = val
    else:
        c.b0 = torch.zeros(LN_W)
        a = a * 2.0 ** -10
    c.a, c.w0 = a, w0
    # exact whatever the order: every partial sum is a multiple of 2^-10 (tiny) or an integer bounded by sum|a||w| + |b|
    assert float((a.abs() @ w0.abs().T).max() * (1024 if name == "tiny" else 1) + c.b0.abs().max()) < 2 ** 24
    c.pre = a @ w0.T + c.b0
    pre64 = a.double() @ w0.double().T + c.b0.double()
    assert torch.equal(c.pre.double(), pre64)
    c.h_ref = F.gelu(F.layer_norm(pre64, (LN_W,), c.gamma.double(), c.beta.double(), 1e-5))
    c.y_ref = a[:, :256].double() + c.h_ref @ c.w3.double().T + c.b3.double()
    if name == "offset":
        sd = pre64.std(1, unbiased=False)
        assert (pre64.mean(1) - 4096).abs().max() < 4 and 6 < float(sd[ln_rows("offset")].min()) and float(sd[ln_rows("offset")].max()) < 10
        assert (pre64[list(LN_CONST_ROWS)] == 4096).all()
        sp = pre64[ln_rows("spike")]
        rest = torch.cat([sp[:, :LN_SPIKE_COL], sp[:, LN_SPIKE_COL + 1:]], 1)
        amp = torch.tensor([abs(LN_SPIKE_ROWS[r]) for r in ln_rows("spike")], dtype=torch.float64)
        assert ((sp[:, LN_SPIKE_COL] - 4096).abs() == 256 * amp).all() and ((rest - 4096).abs() <= 16 * amp[:, None]).all()
        assert (((sp[:, LN_SPIKE_COL] - sp.mean(1)).abs() / sd[ln_rows("spike")]) > 20).all()  # of the row's own sigma
    else:
        var = pre64.var(1, unbiased=False)
        assert 3e-5 < float(var.min()) and float(var.max()) < 1.2e-4  # the order of eps
    _LN[name] = c
    return c


def emulate_layernorm(c, variant=None):
    """fp32 restatement of LayerNorm(512, eps 1e-5) + GELU(erf) on the exact pre-activation: two passes (mean, then the
    mean of squared deviations), 1 / sqrt(var + eps).  The mean is exact here (an integer sum below 2^24 times 2^-9) and so
    is every deviation, so the order of the two sums moves the result by a few u only: torch's order stands for the
    kernels' (which differ among themselves).  `variant` names one wrong algorithm (LN_VARIANTS)."""
    x = c.pre
    mean = x.sum(1, keepdim=True) * (1.0 / LN_W)
    if variant == "one_pass_var":
        var = (x * x).sum(1, keepdim=True) * (1.0 / LN_W) - mean * mean
    else:
        d = x - mean
        var = (d * d).sum(1, keepdim=True) * (1.0 / LN_W)
    eps = {"no_eps": 0.0, "eps_1e-6": 1e-6}.get(variant, 1e-5)
    rstd = 1.0 / (torch.sqrt(var) + eps) if variant == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    return F.gelu((x - mean) * rstd * c.gamma + c.beta)


def emulate_ffn(c, variant=None):
    """The second GEMM with its bias and the residual A0 on the emulated hidden activation."""
    return emulate_layernorm(c, variant) @ c.w3.T + c.b3 + c.a[:, :256]


def ln_ratio(case, out, which="h"):
    """Worst |out - reference| / bound over the rows of `case`; out is the whole launch's [M, 512] (which = "h") or
    [M, 256] FFN output (which = "y")."""
    c = ln_launch(LN_CASES[case][0])
    rows = ln_rows(case)
    ref, tol = (c.h_ref, LN_TOL) if which == "h" else (c.y_ref, FFN_TOL)
    return worst_ratio(out[rows], ref[rows], torch.full_like(ref[rows], tol))


# ============================================================================================== fp32 attention
# 4 heads x 64, scale 0.125, integer q and k: the logits are exact multiples of 1/8.  v holds integers / 8 in [-1, 1].
# Dimension 0 of a head carries the structure of a case, the other 63 hold integers in [-2, 2] (a logit noise of sigma 2):
#   wide          q, k uniform in [-10, 10] in every dimension: logits to about +-145, a bare exp overflows and underflows
#                 in one row
#   ascending     q0 = 8, k0 = 16 (j div 32): the logits rise by 16 per 32 keys, so the running maximum of every query
#                 moves in every half tile and every tile: the rescale of O and of l is live at each step.  With a key
#                 split the early shares' merge weights underflow to exactly 0
#   descending    the same keys (and values) reversed: the first half tile sets the maximum for good -- the skip-rescale
#                 branch, taken by every lane of a wave
#   mixed         ascending keys; queries 3, 17 and 30 of every 32 have q0 = 8, the others q0 = -8 (descending logits): the
#                 wave-uniform skip test must fail because of a few lanes only
#   all_negative  q0 = 8, k0 = -190: every logit about -190; the weights exist only after the subtraction
#   all_positive  k0 = +190
#   equal         all keys identical (entries in [-10, 10], q too): every weight is exactly 1 and O is the mean of v
#
# The bound.  The kernel folds c = fl(scale * log2 e) into the query and accumulates s_j = sum_d k_d fl(q_d c) on the fp32
# matrix pipe.  With B = the case's largest sum_d |q_d k_d| * scale * log2(e):
#   |s_j - exact| <= (64 + 1 + 1) u B   (64 accumulation steps whose partial sums are bounded by B in ANY order, the rounding
#                                        of q_d c, the rounding of c)
#   fl(s_j - m) adds u |s_j - m| <= 2 u B; the maximum m itself and every rescale factor are common to O and l of a query
#   and cancel, as do the merge weights of a key split.
# So the weight of key j carries a relative error eps_j <= ln 2 * 68 u B (70 with the second-order terms), and
#   O' - O = sum_j p_j eps_j (v_j - O) / (1 + sum p eps),   |O' - O| <= ln 2 * 70 u B * (sum_j p_j |v_j| + |O|).
# The remaining arithmetic is relative to sum_j p_j |v_j|: the sums l and P V (nk terms each, worst case nk u each), two
# multiplies per half tile in the rescale, v_exp_f32 (1 ulp = 2 u), the normalisation:
#   A = (2 nk + 4 ceil(nk / 32) + 16) u.
#   tol = ln 2 * 70 u B (sum_j p_j |v_j| + |O|) + A sum_j p_j |v_j|        per element
# It is a worst-case bound (a correct kernel sits one to two orders below it); the host test shows that every wrong
# variant aimed at a case still misses it by a factor of 100 or more.
# `equal` needs none of this: identical keys give bit-identical scores in any deterministic kernel, every weight and every
# merge weight is exactly 1, sum_j v_j (multiples of 1/8 below 2^11) and l = nk are exact, and what is left is the
# normalisation: O = S * fl(1 / nk) or S / nk: tol = 4 u |O|  (reciprocal 2 u when approximate, multiply u, one spare).
ATT_CASES = ("wide", "ascending", "descending", "mixed", "all_negative", "all_positive", "equal")
ATT_VARIANTS = ("no_max", "no_rescale_o", "no_rescale_l", "skip_by_lane0", "merge_no_max", "merge_w1", "merge_no_empty_guard")
# run -> (problem shapes (nq, nk), key split).  300: a query-tile tail; 600: 10 key tiles of 64 (shares 2+2+2+2+2+0+0+0 of
# a split by 8, 4+4+2 by 3); 200 and 100: masked key tails; 100 at split 3: shares 1+1+0, one empty (m = -inf).
ATT_RUNS = {"single": ([(300, 600)], 1), "pair": ([(96, 600), (300, 200)], 1), "split8": ([(96, 600), (300, 100)], 8),
            "split3": ([(96, 600), (300, 100)], 3), "nosplit": ([(96, 600), (300, 100)], 1)}
# case -> {variant aimed at it: the runs in which it must be rejected}
_SPLITS = ("split8", "split3")
_ALL = tuple(ATT_RUNS)
ATT_AIMED = {
    "wide": {"no_max": _ALL},
    "ascending": {"no_rescale_o": _ALL, "no_rescale_l": _ALL, "merge_w1": _SPLITS},
    "descending": {"no_max": _ALL},
    "mixed": {"no_rescale_o": _ALL, "no_rescale_l": _ALL, "skip_by_lane0": _ALL},
    "all_negative": {"no_max": _ALL, "merge_no_max": _SPLITS},
    "all_positive": {"no_max": _ALL, "merge_no_max": _SPLITS},
    "equal": {"no_max": _ALL, "merge_no_empty_guard": _SPLITS},
}
MIXED_ASCENDING_LANES = (3, 17, 30)
_ATT = {}


def _att_head(case, nq, nk, g):
    """(q [nq, 64], k [nk, 64], v [nk, 64]) of one head."""
    if case in ("wide", "equal"):
        q, k = _randint(g, -10, 10, nq, 64), _randint(g, -10, 10, nk, 64)
        if case == "equal":  # one key, entries +-10: logits of sigma 60 over the queries
            k = (k[:1].sign() * 10 + (k[:1] == 0) * 10).expand(nk, 64).contiguous()
    else:
        q, k = _randint(g, -2, 2, nq, 64), _randint(g, -2, 2, nk, 64)
        q[:, 0] = 8
        if case == "mixed":
            q[:, 0] = -8
            for lane in MIXED_ASCENDING_LANES:
                q[lane::32, 0] = 8
        k[:, 0] = {"all_negative": -190.0, "all_positive": 190.0}.get(case, 0.0)
        if case in ("ascending", "descending", "mixed"):
            k[:, 0] = 16.0 * (torch.arange(nk) // 32)
    v = _randint(g, -8, 8, nk, 64) / 8
    if case == "descending":
        k, v = k.flip(0).contiguous(), v.flip(0).contiguous()
    return q, k, v


def _check_design(case, s):
    """s: exact logits [nq, nk] (float64) of one head: the property the case exists for."""
    nq, nk = s.shape
    nb = (nk + 31) // 32
    pad = torch.full((nq, nb * 32 - nk), -INF, dtype=s.dtype)
    bm = torch.cat([s, pad], 1).reshape(nq, nb, 32).max(-1).values       # maximum of every 32-key half tile
    run = bm.cummax(1).values
    moves = run[:, 1:] > run[:, :-1]                                       # the running maximum moves at half tile t + 1
    asc = torch.zeros(nq, dtype=torch.bool)
    if case == "wide":
        assert float(s.max()) > 120 and float(s.min()) < -120
        assert bool(((s.max(1).values > 89) & (s.min(1).values < -104)).any())  # exp overflows and underflows in one row
    elif case == "ascending":
        asc[:] = True
    elif case == "mixed":
        for lane in MIXED_ASCENDING_LANES:
            asc[lane::32] = True
    elif case == "all_negative":
        assert float(s.max()) < -150
    elif case == "all_positive":
        assert float(s.min()) > 150
    elif case == "equal":
        assert bool((s == s[:, :1]).all()) and float(s.abs().max()) > 89
    if case in ("ascending", "descending", "mixed"):
        assert bool(moves[asc].all()) and not bool(moves[~asc].any())
        if asc.any():  # "by about 16 per 32 keys" (the last half tile may be short)
            step = bm[asc][:, 1:-1] - bm[asc][:, :-2]
            assert 8 < float(step.min()) and float(step.max()) < 24


def att_case(case, run):
    """One launch: q, k, v [rows, 256] (NaN in rows a problem does not use), problems [[q_row0, nq, kv_row0, nk]], max_nq,
    the reference `ref` and bound `tol` [rows, 256] float64 (NaN outside every problem's queries), and B."""
    key = (case, run)
    if key in _ATT:
        return _ATT[key]
    shapes, split = ATT_RUNS[run]
    c = types.SimpleNamespace(name=f"{case}-{run}", case=case, run=run, split=split, problems=[])
    r0 = 0
    for nq, nk in shapes:
        c.problems.append([r0, nq, r0, nk])
        r0 += max(nq, nk)
    c.rows, c.max_nq = r0, max(nq for nq, _ in shapes)
    c.q, c.k, c.v = (torch.full((r0, 256), NAN) for _ in range(3))
    c.ref, c.tol = (torch.full((r0, 256), NAN, dtype=torch.float64) for _ in range(2))
    per_head, c.B = [], 0.0
    for z, (row, nq, _, nk) in enumerate(c.problems):
        for h in range(HEADS):
            cs = slice(64 * h, 64 * h + 64)
            q, k, v = _att_head(case, nq, nk, _gen("attention", case, nq, nk, z, h))
            c.q[row:row + nq, cs], c.k[row:row + nk, cs], c.v[row:row + nk, cs] = q, k, v
            s32 = (q @ k.T) * SCALE
            s = (q.double() @ k.double().T) * SCALE
            assert float(q.abs().sum(1).max() * k.abs().max()) < 2 ** 24 and torch.equal(s32.double(), s)  # exact logits
            _check_design(case, s)
            c.B = max(c.B, float((q.abs() @ k.abs().T).max()) * SCALE * LOG2E)
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            p = e / e.sum(-1, keepdim=True)
            o = p @ v.double()
            if case == "equal":  # the closed form: the mean of v, exactly 0 where the column sums to 0
                o = (v.double().sum(0) / nk).expand(nq, 64)
            per_head.append((row, nq, nk, cs, o, p @ v.double().abs()))
    for row, nq, nk, cs, o, pv in per_head:
        c.ref[row:row + nq, cs] = o
        if case == "equal":
            c.tol[row:row + nq, cs] = 4 * U * o.abs()
        else:
            arith = (2 * nk + 4 * ((nk + 31) // 32) + 16) * U
            c.tol[row:row + nq, cs] = LN2 * 70 * U * c.B * (pv + o.abs()) + arith * pv
    assert torch.isfinite(c.ref[~torch.isnan(c.ref)]).all()
    _ATT[key] = c
    return c


def att_ratio(c, o):
    """(worst |o - ref| / tol over every problem's queries, rows outside them still NaN)."""
    valid = ~torch.isnan(c.ref)
    return worst_ratio(o[valid], c.ref[valid], c.tol[valid]), bool(torch.isnan(o[~valid]).all())


def tiles_per_split(nk, split):
    """The kernel's share of 64-key tiles per split (attention_kernel: kt0, kt1)."""
    nt = (nk + 63) // 64
    per = (nt + split - 1) // split
    return [max(0, min(nt, (s + 1) * per) - s * per) for s in range(split)]


def _scores(q, k):
    """fp32 scores in log2 units, c = fl(scale log2 e) folded into q, accumulated in the matrix pipe's k order with one
    product and one rounding per step -- the same sequence for every key, so equal keys give bit-equal scores."""
    qs = q * (torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    s = torch.zeros(q.shape[0], k.shape[0])
    for d in [8 * g + 4 * hh + j for g in range(8) for j in range(4) for hh in range(2)]:
        s = (s.double() + qs[:, d, None].double() * k[None, :, d].double()).float()
    return s


def _emulate_head(s_all, v, split, variant):
    """One (problem, head) in the kernel's arithmetic and order, from its scores (_scores): per key share an online
    soft-max over half tiles of 32 keys (running maximum, l and O rescaled by exp2(m_old - m_new)); without a split O / l,
    with one the merge of the shares' (O, m, l) weighted by exp2(m_s - m), an empty share (m = -inf) by 0.  `variant` names one wrong algorithm (ATT_VARIANTS):
      no_max                bare exp2(s), no running maximum
      no_rescale_o / _l     O / l not rescaled when the maximum moves
      skip_by_lane0         the rescale of O skipped for a 32-query tile when its first query does not need it
      merge_no_max          merge weights exp2(m_s), the overall maximum not subtracted
      merge_w1              every share merged with weight 1
      merge_no_empty_guard  the merge combines normalised shares O_s / l_s with weights w_s l_s: 0 / 0 for an empty share
    """
    nq, nk = s_all.shape
    nt = (nk + 63) // 64
    per = (nt + split - 1) // split
    parts = []
    for sp in range(split):
        kt0, kt1 = sp * per, min(nt, (sp + 1) * per)
        m = torch.zeros(nq) if variant == "no_max" else torch.full((nq,), -INF)
        l, o = torch.zeros(nq), torch.zeros(nq, 64)
        for key0 in range(kt0 * 64, min(kt1 * 64, nk), 32):
            blk, vb = s_all[:, key0:min(key0 + 32, nk)], v[key0:min(key0 + 32, nk)]
            m_new = m if variant == "no_max" else torch.maximum(m, blk.max(1).values)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(blk - m_new[:, None])
            l = l + p.sum(1) if variant == "no_rescale_l" else l * alpha + p.sum(1)
            if variant == "skip_by_lane0":
                need = (m_new != m)[torch.arange(nq) // 32 * 32]  # the first query of each 32-query tile decides
                o = torch.where(need[:, None], o * alpha[:, None], o)
            elif variant != "no_rescale_o":  # (skipping where no lane needs it multiplies by exactly 1: bit-identical)
                o = o * alpha[:, None]
            o = o + p @ vb
            m = m_new
        parts.append((o, m, l))
    if split == 1:
        o, _, l = parts[0]
        return o * (1.0 / l)[:, None]
    mall = torch.stack([m for _, m, _ in parts]).max(0).values
    acc, lsum = torch.zeros(nq, 64), torch.zeros(nq)
    for o, m, l in parts:
        if variant == "merge_w1":
            w = torch.ones(nq)
        elif variant == "merge_no_max":
            w = torch.exp2(m)
        else:
            w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mall))
        if variant == "merge_no_empty_guard":
            acc = acc + (w * l)[:, None] * (o / l[:, None])
        else:
            acc = acc + w[:, None] * o
        lsum = lsum + w * l
    return acc / lsum[:, None]


def emulate_attention(c, variant=None):
    """The whole launch in the emulation (the scores are computed once per case and kept)."""
    o = torch.full((c.rows, 256), NAN)
    if not hasattr(c, "scores"):
        c.scores = {}
    for z, (row, nq, _, nk) in enumerate(c.problems):
        for h in range(HEADS):
            cs = slice(64 * h, 64 * h + 64)
            if (z, h) not in c.scores:
                c.scores[z, h] = _scores(c.q[row:row + nq, cs], c.k[row:row + nk, cs])
            o[row:row + nq, cs] = _emulate_head(c.scores[z, h], c.v[row:row + nk, cs], c.split, variant)
    return o


# ============================================================================================== detector head
# hidden holds integers in [-2, 2]; each of the 65 filters (the dustbin's included) 8 entries of +-1; the logits are exact
# integers.  Two modes:
#   affine   scale 16 on every channel, integer bias b_c in [-3, 3], shift_c = 96 - 16 b_c: logit_c = 16 acc_c + 96, in
#            [-160, 352] -- exp of a bare logit overflows in every cell
#   plain    no affine, bias 3 on every channel: logit_c = acc_c + 3
# Special cells (DH_SPECIAL, planted first and last in the launch, and on both sides of the 128-cell workgroup edge):
#   dust_max   hidden = 2 w[64]: the dustbin's acc is 16, every other |acc| <= 4: the dustbin is the maximum by 192 or more
#              (affine) and every heat-map value is 0 in fp32; a sum without the dustbin makes them O(1)
#   dust_over  hidden = 2 w[64] on three of its eight entries: the dustbin leads every heat-map channel by exactly 96
#              (affine), past the overflow threshold of expf (88.7): a maximum taken over the 64 heat-map channels only
#              leaves expf(96) = inf in the sum and 0 in every output, where the true values, exp(-96) = 2.0e-42, are
#              1400 units of the last place of an fp32 subnormal
#   dust_min   hidden = -2 w[64]
#   tie        hidden = 2 w[5] + 2 w[9] (disjoint supports): channels 5 and 9 tie exactly for the maximum; their outputs
#              must be equal
#   all_equal  hidden = 0: all 65 logits equal, every output is 1 / 65
# The bound.  The argument l_c - max of expf is an exact integer.  expf is within 1 ulp (2 u), the ordered sum of 65
# non-negative terms within 64 u of its value, the division within u: |p' - p| <= 67 u p (70 with second-order terms).
# Below 2^-126 the relative bound is replaced by the spacing of the subnormals, 2^-149: the library is built without
# flush-to-zero, expf delivers subnormal results down to exp(-103.3) (one rounding at that spacing, one more in its
# scaling step), the division by a sum in [1, 65] rounds once more -- under 3 spacings, taken as 4:
#   tol = 70 u p + 4 * 2^-149     per element
DH_SHAPES = ((2, 9, 15), (1, 1, 3))
DH_MODES = ("affine", "plain")
DH_VARIANTS = ("no_max", "max_over_64", "sum_over_64")
DH_SPECIAL = ("dust_max", "dust_min", "tie", "all_equal", "dust_over")
DH_TIE = (5, 9)
# cell kind -> {variant aimed at it: the modes in which it must be rejected}
DH_AIMED = {"dust_max": {"sum_over_64": DH_MODES, "no_max": ("affine",)}, "dust_over": {"max_over_64": ("affine",)},
            "dust_min": {"no_max": ("affine",)}, "tie": {"no_max": ("affine",)}, "all_equal": {"no_max": ("affine",)},
            "random": {"no_max": ("affine",), "sum_over_64": DH_MODES}}
_DH = {}


def dh_case(shape, mode):
    """hidden [cells, 512] (the merged head's row pitch; columns 256.. hold NaN-free filler the kernel must not use),
    w [65, 256], bias, scale, shift (None in plain mode), logits (exact, float64), ref / tol [cells, 64] and
    kind: {name: cell indices}."""
    key = (shape, mode)
    if key in _DH:
        return _DH[key]
    b, h8, w8 = shape
    cells = b * h8 * w8
    g = _gen("detector", shape)
    c = types.SimpleNamespace(name=f"{b}x{h8}x{w8}-{mode}", shape=shape, mode=mode, cells=cells)
    w = torch.zeros(65, 256)
    gw = _gen("detector", "filters")
    w.scatter_(1, torch.rand(65, 256, generator=gw).argsort(1)[:, :8], _randint(gw, 0, 1, 65, 8) * 2 - 1)
    assert float((w[DH_TIE[0]].abs() * w[DH_TIE[1]].abs()).sum()) == 0  # disjoint supports
    hidden = torch.zeros(cells, 512)
    hidden[:, :256] = _randint(g, -2, 2, cells, 256)
    hidden[:, 256:] = _randint(g, -2, 2, cells, 256) * 64  # the other half of the merged head: must not reach the logits
    w64_3 = w[64].clone()
    w64_3[w[64].nonzero().reshape(-1)[3:]] = 0
    special = {"dust_max": 2 * w[64], "dust_min": -2 * w[64], "tie": 2 * w[DH_TIE[0]] + 2 * w[DH_TIE[1]],
               "all_equal": torch.zeros(256), "dust_over": 2 * w64_3}
    if cells < 16:  # three cells: the tie, all equal, the dustbin on top
        plan = [(0, "tie"), (1, "all_equal"), (2, "dust_max")]
    else:
        where = [0, 1, 2, 3, 126, 127, 128, 129, 255, 256, cells - 3, cells - 2, cells - 1]
        plan = [(cell, DH_SPECIAL[i % 5]) for i, cell in enumerate(where)]
    c.kind = {n: [] for n in DH_SPECIAL}
    for cell, n in plan:
        hidden[cell, :256] = special[n]
        c.kind[n].append(cell)
    c.kind["random"] = [i for i in range(cells) if i not in dict(plan)]
    c.hidden, c.w = hidden, w
    if mode == "affine":
        c.bias = _randint(_gen("detector", "bias"), -3, 3, 65)
        c.scale, c.shift = torch.full((65,), 16.0), 96 - 16 * c.bias
    else:
        c.bias, c.scale, c.shift = torch.full((65,), 3.0), None, None
    c.logits32 = dh_logits(c, torch.float32)
    c.logits = dh_logits(c, torch.float64)
    assert torch.equal(c.logits32.double(), c.logits) and torch.equal(c.logits, c.logits.round())  # exact integers
    lg = c.logits
    if mode == "affine":
        assert float(lg.max()) > 100 and (cells < 16 or float(lg.min()) < -100) and float(lg.max(1).values.min()) > 89
        assert (lg[c.kind["dust_max"], 64] - lg[c.kind["dust_max"], :64].max(1).values).min() >= 192
        assert ((lg[c.kind["dust_over"], 64] - lg[c.kind["dust_over"], :64].max(1).values) == 96).all()
    for cell in c.kind["dust_max"]:
        assert int(lg[cell].argmax()) == 64
    for cell in c.kind["dust_min"]:
        assert int(lg[cell].argmin()) == 64 and float(lg[cell, 64]) < float(lg[cell, :64].min())
    for cell in c.kind["tie"]:
        top = lg[cell].topk(3).values.tolist()
        assert top[0] == top[1] > top[2] and float(lg[cell, DH_TIE[0]]) == float(lg[cell, DH_TIE[1]]) == top[0]
    for cell in c.kind["all_equal"]:
        assert bool((lg[cell] == lg[cell, 0]).all())
    p = torch.softmax(lg, 1)[:, :64]
    c.ref, c.tol = p, 70 * U * p + 4 * 2.0 ** -149
    assert torch.isfinite(c.ref).all()
    _DH[key] = c
    return c


def dh_logits(c, dtype):
    lg = c.hidden[:, :256].to(dtype) @ c.w.to(dtype).T + c.bias.to(dtype)
    return lg if c.scale is None else lg * c.scale.to(dtype) + c.shift.to(dtype)


def dh_to_heat(c, cells64):
    """[cells, 64] -> the heat-map [b, 8 h8, 8 w8] (depth-to-space)."""
    b, h8, w8 = c.shape
    return cells64.reshape(b, h8, w8, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h8 * 8, w8 * 8)


def dh_from_heat(c, heat):
    b, h8, w8 = c.shape
    return heat.reshape(b, h8, 8, w8, 8).permute(0, 1, 3, 2, 4).reshape(c.cells, 64)


def emulate_head(c, variant=None):
    """fp32: the maximum over the 65 logits, expf(l - max), the sum over c = 0..64 in order, the 64 heat-map channels
    divided by it.  `variant`: no_max (bare expf), max_over_64 (the dustbin left out of the maximum), sum_over_64 (the
    dustbin left out of the sum)."""
    lg = c.logits32
    if variant == "no_max":
        m = torch.zeros(c.cells, 1)
    else:
        m = lg[:, :64 if variant == "max_over_64" else 65].max(1, keepdim=True).values
    e = torch.exp((lg - m).double()).float()  # expf, correctly rounded (subnormal results included)
    s = torch.zeros(c.cells)
    for ch in range(64 if variant == "sum_over_64" else 65):
        s = s + e[:, ch]
    return e[:, :64] / s[:, None]


def dh_ratio(c, cells64, kind=None):
    rows = list(range(c.cells)) if kind is None else c.kind[kind]
    return worst_ratio(cells64[rows], c.ref[rows], c.tol[rows])
