"""Float64 closed form of the backward of LightGlue's bidirectional cross attention and of the `to_qk` / `to_v` linears
around it, written from the reference's text: gluefactory/models/matchers/lightglue.py:196-218 (CrossBlock.forward, the
non-flash branch without a mask).  Test infrastructure: torch only, no autograd: the host test holds the closed form to
torch's own float64 autograd on the same block.

Per pair and head (4 heads of 64, scale = 64^-0.5), q_a = to_qk(x_a), v_a = to_v(x_a), sides a in {0, 1}:
    S = scale q0 q1^T          P01 = softmax_j S          P10^T = softmax_i S         ctx0 = P01 v1, ctx1 = P10 v0
    D0[i] = dctx0[i] . ctx0[i]                            D1[j] = dctx1[j] . ctx1[j]
    dS[i,j] = P01[i,j] (dctx0[i] . v1[j] - D0[i]) + P10^T[i,j] (v0[i] . dctx1[j] - D1[j])
    dq0 = scale dS q1          dq1 = scale dS^T q0        dv1 = P01^T dctx0           dv0 = P10^T dctx1
    dWqk = dq^T x, dbqk = sum dq, dWv = dv^T x, dbv = sum dv  (rows of both sides)    dx = dx_in + dq Wqk + dv Wv

Rows are packed as `forward_layers` packs them: [B*M + B*N, 256], side 0 of every pair, then side 1.

Beside every output element stands its ERROR SUM in units of 2^-23, added up stage by stage by the first-order rules of
tests/output_stage_reference.py (a sum of K terms is charged E(K) = sqrt(K) + 1 times the sum of the absolute values of
its terms; a product passes on |b| err(a) + |a| err(b) + |a b|).  The rules that are this block's own:
    q = x W^T + b (gfc_linear)     err(q) = |W| err(x) + (E(256) + 1) (|x| |W|^T + |b|)
    S = scale q_a . q_b            err(S) = scale (E(64) |q_a| . |q_b| + err(q_a) . |q_b| + |q_a| . err(q_b)) + |S|
    lse_a[i] = log sum_j exp S     err(lse) = sum_j P[i,j] err(S[i,j]) + E(N_b) + 4 + |lse|   (a weighted mean of the
                                   errors of S, the sum's own relative error, exp and log, and the last addition)
    P = exp(S - lse)               an ABSOLUTE error of the exponent is a RELATIVE error of P:
                                   err(P) = P (err(S) + err(lse) + |S - lse| + 2) + 2^-126 / 2^-23 (below the smallest
                                   normal fp32 number a P has no relative accuracy: exp underflows to 0)
    T = dctx . v, D = dctx . ctx   E(64) times their absolute sums, plus what the operands bring
    dS                             each term P (T - D): err(P) |T - D| + P (err(T) + err(D)) + 2 |P (T - D)|, and |dS|
    dq = scale sum_j dS q_b        scale (sum err(dS) |q_b| + E(N_b) sum |dS| |q_b| + sum |dS| err(q_b)) + |dq|
    dv = sum_j P dctx_b            sum err(P) |dctx_b| + E(N_b) sum P |dctx_b| + sum P err(dctx_b)
The bounds are on the ABSOLUTE sums: P (dP - D) cancels (the to_qk gradient is about 80 times smaller than the to_v
gradient on the fixtures), so a bound relative to the result would be one no fp32 evaluation can hold.  The constants
depend on the shape alone; none is fitted to a result.

`variant` switches ONE deliberate mistake on (VARIANTS); the host test shows that each misses a bound widely.
"""
import math

import torch

U = 2.0 ** -23
D = 256
HEADS = 4
HD = 64
SCALE = HD ** -0.5
TINY = 2.0 ** -126 / U  # the smallest normal fp32 number, in units of 2^-23
VARIANTS = ("col_softmax_along_rows", "scale_twice", "no_scale_dq", "no_D", "D_from_dctx", "dv_swapped", "one_direction",
            "dwqk_transposed", "dbqk_from_dv", "heads_merged", "dx_no_v")
OUTPUTS = ("dWqk", "dbqk", "dWv", "dbv", "dx", "dx_att")
# The descent check on the twelve tensors of the last cross block: the step, and the float64 ratio
# (total(theta - eps grad) - total(theta)) / (-eps |grad|^2) the host test measures at loss.gamma 1.
DESCENT_EPS = 0.005
DESCENT_RATIO = {"a": 0.9858, "b": 0.9657}


def _e(k):
    return math.sqrt(k) + 1.0


def split_heads(rows, b, m, n, heads=HEADS):
    """[B*M + B*N, heads*hd] -> ([B,heads,M,hd], [B,heads,N,hd])."""
    hd = rows.shape[1] // heads
    s0 = rows[:b * m].reshape(b, m, heads, hd).transpose(1, 2)
    s1 = rows[b * m:].reshape(b, n, heads, hd).transpose(1, 2)
    return s0, s1


def merge_heads(t0, t1):
    """The inverse of split_heads."""
    b, h, m, hd = t0.shape
    n = t1.shape[2]
    return torch.cat([t0.transpose(1, 2).reshape(b * m, h * hd), t1.transpose(1, 2).reshape(b * n, h * hd)], 0)


def attention_forward(qk, v, b, m, n, scale=SCALE, heads=HEADS):
    """ctx [R,256] of the cross attention in the precision of its inputs."""
    q0, q1 = split_heads(qk, b, m, n, heads)
    v0, v1 = split_heads(v, b, m, n, heads)
    s = scale * (q0 @ q1.transpose(-1, -2))
    return merge_heads(torch.softmax(s, -1) @ v1, torch.softmax(s, -2).transpose(-1, -2) @ v0)


def attention_backward(qk, v, ctx, dctx, b, m, n, scale=SCALE, variant=None, err=None):
    """qk, v, ctx, dctx [R,256] float64 (ctx as the caller holds it: D is formed from it, as the kernel forms it).
    -> ({dqk, dv}, {dqk, dv} error sums), [R,256].  err: {name: the error sum its operand arrives with}, of qk, v, ctx,
    dctx (default 0: the same bits)."""
    heads = 1 if variant == "heads_merged" else HEADS
    z = torch.zeros_like(qk)
    err = err or {}
    sp = lambda t: split_heads(t, b, m, n, heads)  # noqa: E731
    q0, q1 = sp(qk)
    v0, v1 = sp(v)
    c0, c1 = sp(ctx)
    g0, g1 = sp(dctx)
    eq0, eq1 = sp(err.get("qk", z))
    ev0, ev1 = sp(err.get("v", z))
    ec0, ec1 = sp(err.get("ctx", z))
    eg0, eg1 = sp(err.get("dctx", z))
    hd = q0.shape[-1]
    t = lambda x: x.transpose(-1, -2)  # noqa: E731
    ab = torch.abs
    s = scale * (q0 @ t(q1))                                          # [B,h,M,N]
    es = scale * (_e(hd) * (ab(q0) @ t(ab(q1))) + eq0 @ t(ab(q1)) + ab(q0) @ t(eq1)) + ab(s)
    lse0 = torch.logsumexp(s, -1, keepdim=True)                       # of side 0's rows, over j
    lse1 = torch.logsumexp(s, -2, keepdim=True)                       # of side 1's rows, over i
    p01, p10t = torch.exp(s - lse0), torch.exp(s - lse1)
    el0 = (p01 * es).sum(-1, keepdim=True) + _e(n) + 4 + ab(lse0)
    el1 = (p10t * es).sum(-2, keepdim=True) + _e(m) + 4 + ab(lse1)
    ep01 = p01 * (es + el0 + ab(s - lse0) + 2) + TINY
    ep10t = p10t * (es + el1 + ab(s - lse1) + 2) + TINY
    if variant == "col_softmax_along_rows":
        p10t = p01
    t1 = g0 @ t(v1)                                                   # dctx0[i] . v1[j]
    t2 = v0 @ t(g1)                                                   # v0[i] . dctx1[j]
    et1 = _e(hd) * (ab(g0) @ t(ab(v1))) + eg0 @ t(ab(v1)) + ab(g0) @ t(ev1)
    et2 = _e(hd) * (ab(v0) @ t(ab(g1))) + ev0 @ t(ab(g1)) + ab(v0) @ t(eg1)
    d0 = (g0 * c0).sum(-1, keepdim=True)                              # [B,h,M,1]
    d1 = t((g1 * c1).sum(-1, keepdim=True))                           # [B,h,1,N]
    ed0 = (_e(hd) * ab(g0 * c0) + eg0 * ab(c0) + ab(g0) * ec0).sum(-1, keepdim=True)
    ed1 = t((_e(hd) * ab(g1 * c1) + eg1 * ab(c1) + ab(g1) * ec1).sum(-1, keepdim=True))
    if variant == "no_D":
        d0, d1 = torch.zeros_like(d0), torch.zeros_like(d1)
    elif variant == "D_from_dctx":
        d0, d1 = (g0 * g0).sum(-1, keepdim=True), t((g1 * g1).sum(-1, keepdim=True))
    a1, a2 = p01 * (t1 - d0), p10t * (t2 - d1)
    ds = a1 if variant == "one_direction" else a1 + a2
    eds = (ep01 * ab(t1 - d0) + p01 * (et1 + ed0) + 2 * ab(a1) + ep10t * ab(t2 - d1) + p10t * (et2 + ed1) + 2 * ab(a2)
           + ab(ds))
    k = {"scale_twice": scale * scale, "no_scale_dq": 1.0}.get(variant, scale)
    dq0, dq1 = k * (ds @ q1), k * (t(ds) @ q0)
    edq0 = scale * (eds @ ab(q1) + _e(n) * (ab(ds) @ ab(q1)) + ab(ds) @ eq1) + ab(dq0)
    edq1 = scale * (t(eds) @ ab(q0) + _e(m) * (t(ab(ds)) @ ab(q0)) + t(ab(ds)) @ eq0) + ab(dq1)
    if variant == "dv_swapped":  # each side with the other direction's soft-max
        dv0, dv1 = p01 @ g1, t(p10t) @ g0
    else:
        dv0, dv1 = p10t @ g1, t(p01) @ g0
    edv0 = ep10t @ ab(g1) + _e(n) * (p10t @ ab(g1)) + p10t @ eg1
    edv1 = t(ep01) @ ab(g0) + _e(m) * (t(p01) @ ab(g0)) + t(p01) @ eg0
    return ({"dqk": merge_heads(dq0, dq1), "dv": merge_heads(dv0, dv1)},
            {"dqk": merge_heads(edq0, edq1), "dv": merge_heads(edv0, edv1)})


def linear(x, w, bias, ex=None):
    """(x W^T + b, its error sum as gfc_linear evaluates it)."""
    y = x @ w.t() + bias
    e = (_e(D) + 1) * (x.abs() @ w.abs().t() + bias.abs())
    return y, e if ex is None else e + ex @ w.abs().t()


def backward(x, ctx, dctx, dx_in, p, b, m, n, variant=None, in_err=0.0, err=None):
    """The block entry: x, ctx, dctx [R,256], dx_in [R,256] or None, p: Wqk, bqk, Wv, bv (float64).
    -> (grads, error sums) keyed by OUTPUTS: `dx_att` = dq Wqk + dv Wv, the attention's share alone, `dx` = dx_in +
    dx_att (dx_att itself without dx_in).  in_err: the error x, ctx, dctx and dx_in arrive with, in units of 2^-23 of
    their magnitudes (a comparison ACROSS two evaluations of the trunk); err: the same per operand as error sums
    ({"x", "ctx", "dctx", "dx_in"}), added to it."""
    err = err or {}
    e_of = lambda name, t: in_err * t.abs() + err.get(name, 0.0)  # noqa: E731
    ex, ectx, edctx = e_of("x", x), e_of("ctx", ctx), e_of("dctx", dctx)
    wqk, bqk, wv, bv = p["Wqk"], p["bqk"], p["Wv"], p["bv"]
    rows = x.shape[0]
    red = _e(rows) + 2
    qk, eqk = linear(x, wqk, bqk, ex)
    v, ev = linear(x, wv, bv, ex)
    g, eg = attention_backward(qk, v, ctx, dctx, b, m, n, variant=variant,
                               err={"qk": eqk, "v": ev, "ctx": ectx, "dctx": edctx})
    dqk, dv, edqk, edv = g["dqk"], g["dv"], eg["dqk"], eg["dv"]
    grads = {"dWqk": x.t() @ dqk if variant == "dwqk_transposed" else dqk.t() @ x,
             "dbqk": dv.sum(0) if variant == "dbqk_from_dv" else dqk.sum(0), "dWv": dv.t() @ x, "dbv": dv.sum(0)}
    errs = {"dWqk": edqk.t() @ x.abs() + red * (dqk.abs().t() @ x.abs()) + dqk.abs().t() @ ex,
            "dbqk": (edqk + red * dqk.abs()).sum(0),
            "dWv": edv.t() @ x.abs() + red * (dv.abs().t() @ x.abs()) + dv.abs().t() @ ex,
            "dbv": (edv + red * dv.abs()).sum(0)}
    t1, t2 = dqk @ wqk, dv @ wv
    att = t1 if variant == "dx_no_v" else t1 + t2
    eatt = (edqk @ wqk.abs() + edv @ wv.abs() + _e(D) * (dqk.abs() @ wqk.abs() + dv.abs() @ wv.abs()) + att.abs())
    grads["dx_att"], errs["dx_att"] = att, eatt
    if dx_in is None:
        grads["dx"], errs["dx"] = att, eatt
    else:
        grads["dx"] = dx_in + att
        errs["dx"] = eatt + e_of("dx_in", dx_in) + grads["dx"].abs()
    return grads, errs


def bounds(errs, extra=0.0):
    """{output: the per-element bound}: 2^-23 * (1 + extra) * error sum."""
    return {k: (1.0 + extra) * U * v for k, v in errs.items()}


def worst_ratio(y, ref, tol):
    """max over elements of |y - ref| / tol; NaN or inf in y counts as infinite; 0 / 0 as 0."""
    err = (y.double() - ref).abs()
    r = torch.where((err == 0) & (tol == 0), torch.zeros_like(err), err / tol)
    return float(r.nan_to_num(nan=float("inf"), posinf=float("inf")).max())


def random_params(gen, gain=2.0):
    """to_qk / to_v with the magnitudes of a trained block: rows of W of norm about `gain` for to_qk (so that the
    soft-max rows are not flat: scale S spreads over several units), about 1 for to_v; float32."""
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    return {"Wqk": r(D, D) / D ** 0.5 * gain, "bqk": r(D) * 0.1, "Wv": r(D, D) / D ** 0.5, "bv": r(D) * 0.1}


def to64(p):
    return {k: v.double() for k, v in p.items()}


def random_core(b, m, n, seed, dctx_sign=None, q_gain=3.0):
    """(qk, v, ctx, dctx) float32 [R,256] for the core alone: q of a spread that gives soft-max rows whose maximum is
    several times uniform, ctx the float32 rounding of the float64 forward on these q and v."""
    g = torch.Generator().manual_seed(seed)
    rows = b * (m + n)
    qk = torch.randn((rows, D), generator=g) * (q_gain / HD ** 0.25)
    v = torch.randn((rows, D), generator=g)
    dctx = torch.randn((rows, D), generator=g) * 1e-3
    if dctx_sign is not None:
        dctx = dctx.abs() * dctx_sign
    ctx = attention_forward(qk.double(), v.double(), b, m, n).float()
    return qk, v, ctx, dctx


def stage_params(sd, layer):
    """to_qk and to_v of `transformers.{layer}.cross_attn` out of a state dict, keyed as `backward` takes them."""
    pre = f"transformers.{layer}.cross_attn."
    return {"Wqk": sd[pre + "to_qk.weight"], "bqk": sd[pre + "to_qk.bias"], "Wv": sd[pre + "to_v.weight"],
            "bv": sd[pre + "to_v.bias"]}


# ---- conditioning cases on exact data ---------------------------------------------------------------------------------
def identical_keys_case(m=40, seed=3):
    """B = 1, N = 64 keys that are all one row (qk and v): every P01 is 1 / 64, ctx0 is that v row, and side 1's own
    rows are indistinguishable, so dv1's rows are the same bits.  Integer-valued data over 8: every dot product of depth
    64 is exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    n = 64
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float() / 8  # noqa: E731
    qk = torch.cat([ri(m, D), ri(1, D).expand(n, D)], 0).contiguous()
    v = torch.cat([ri(m, D), ri(1, D).expand(n, D)], 0).contiguous()
    dctx = ri(m + n, D) / 128
    ctx = attention_forward(qk.double(), v.double(), 1, m, n).float()
    return qk, v, ctx, dctx, (1, m, n)


def dominant_key_case(m=37, n=70, key=33):
    """B = 1: side 0's rows all have q = 40 e_0 per head, key `key` of side 1 has q = 40 e_0 and every other key q = 0,
    so scale S is 200 at that key and 0 elsewhere: a gap of 200, where exp underflows to 0 in fp32 and P01 is exactly
    one-hot.  dctx is zero on side 1, integer-valued over 1024 on side 0, v integer-valued: ctx0 = v1[key] exactly,
    dctx0 . v1[key] - D0 is exactly 0, so dS, dq0, dq1 and dv0 are exact zeros, dv1 is zero but for row `key`, which
    holds the column sums of dctx0 (exact)."""
    g = torch.Generator().manual_seed(17)
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()  # noqa: E731
    qk = torch.zeros((m + n, D))
    qk[:m, ::HD] = 40.0
    qk[m + key, ::HD] = 40.0
    v = ri(m + n, D)
    dctx = torch.cat([ri(m, D) / 1024, torch.zeros((n, D))], 0)
    ctx = attention_forward(qk.double(), v.double(), 1, m, n).float()
    return qk, v, ctx, dctx, (1, m, n), key
