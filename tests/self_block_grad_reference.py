"""Float64 closed form of the backward of LightGlue's rotary self attention and of the `Wqkv` linear around it, written
from the reference's text: gluefactory/models/matchers/lightglue.py:43-50 (rotate_half, apply_cached_rotary_emb),
:124-129 (Attention.forward, the non-flash branch without a mask) and :151-162 (SelfBlock.forward up to the context).
Test infrastructure: torch only, no autograd: the host test holds the closed form to torch's own float64 autograd on the
same block.

Per side of a pair and per head (4 heads of 64, scale = 64^-0.5), on the rows of that side alone:
    t = x Wqkv^T + bqkv         q' = Rot(q), k' = Rot(k), adjacent columns paired, tables c, s [rows,64]:
                                o[2i] = t[2i] c[2i] - t[2i+1] s[2i],  o[2i+1] = t[2i+1] c[2i+1] + t[2i] s[2i+1]
    S = scale q' k'^T           P = softmax_j S            ctx = P v
    D[i] = dctx[i] . ctx[i]     dS = P (dctx v^T - D)
    dq' = scale dS k'           dk' = scale dS^T q'        dv = P^T dctx
    dq = Rot^T(dq'), dk = Rot^T(dk'):  dt[2i] = do[2i] c[2i] + do[2i+1] s[2i+1],  dt[2i+1] = do[2i+1] c[2i+1] - do[2i] s[2i]
    dWqkv = dqkv^T x, dbqkv = sum dqkv (rows of both sides)                     dx = dx_in + dqkv Wqkv

Rows are packed as `forward_layers` packs them: [B*M + B*N, .], side 0 of every pair, then side 1.  qkv, dqkv, Wqkv and
bqkv are in the library's PACKED order s*256 + head*64 + dd; `to_packed` / `to_state_dict` map rows from and to the state
dict's head*192 + dd*3 + s.

Beside every output element stands its ERROR SUM in units of 2^-23, added up stage by stage by the first-order rules of
tests/output_stage_reference.py and tests/cross_attn_grad_reference.py (a sum of K terms is charged E(K) = sqrt(K) + 1
times the sum of the absolute values of its terms; a product passes on |b| err(a) + |a| err(b) + |a b|).  The rules that
are this block's own:
    o = Rot(t)                     err(o[c]) = |c| err(t[c]) + |s| err(t[c^1]) + |t[c] c| + |t[c^1] s| + |o[c]|
                                   (two rounded products and one addition; the tables are operands, the same bits)
    S, lse, P, T, D                as in tests/cross_attn_grad_reference.py, with the keys on the row's own side
    dS = P (T - D)                 err(P) |T - D| + P (err(T) + err(D)) + 2 |dS|
    do = scale sum_j dS k'         scale (sum err(dS) |k'| + E(n) sum |dS| |k'| + sum |dS| err(k')) + |do|
    dt = Rot^T(do)                 the rule of Rot on do
    dv = sum_i P dctx              sum err(P) |dctx| + E(n) sum P |dctx| + sum P err(dctx)
The bounds are on the ABSOLUTE sums: P (dP - D) cancels.  The constants depend on the shape alone; none is fitted to a
result.

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
VARIANTS = ("rot_not_transposed", "dk_not_unrotated", "dv_rotated", "pair_half", "no_scale", "scale_twice",
            "softmax_over_queries", "dk_from_P", "D_all_columns", "dS_not_transposed", "row_order_confused", "dx_no_v")
BLOCK_VARIANTS = ("no_head_term",)  # of block_backward: head L - 2's term dropped from the layer's input rows
OUTPUTS = ("dWqkv", "dbqkv", "dx", "dx_att")
# The descent check on the 22 tensors of the last layer: the step, and the float64 ratio
# (f(theta - eps grad) - f(theta)) / (-eps |grad|^2), f = mean(total - confidence), the host test measures at loss.gamma 1.
DESCENT_EPS = 0.0025
DESCENT_RATIO = {"a": 0.9866, "b": 0.9680}


def _e(k):
    return math.sqrt(k) + 1.0


# ---- row orders ---------------------------------------------------------------------------------------------------------
def packed_index():
    """src[packed row] = state-dict row: packed s*256 + head*64 + dd <- head*192 + dd*3 + s."""
    idx = torch.arange(3 * D)
    s, rem = idx // D, idx % D
    return (rem // HD) * (3 * HD) + (rem % HD) * 3 + s


def to_packed(t):
    """Rows of Wqkv / bqkv (or of their gradients) from state-dict to packed order."""
    return t[packed_index()]


def to_state_dict(t):
    """The inverse of to_packed."""
    out = torch.empty_like(t)
    out[packed_index()] = t
    return out


# ---- rotation -----------------------------------------------------------------------------------------------------------
def _swap(t, half=False):
    """Column c <- column c^1 within every 64-wide head ((i, i+32) with `half`: the wrong pairing)."""
    r = t.reshape(t.shape[0], -1, HD)
    if half:
        return torch.cat([r[..., HD // 2:], r[..., :HD // 2]], -1).reshape(t.shape)
    return r.reshape(t.shape[0], -1, HD // 2, 2).flip(-1).reshape(t.shape)


def _sign(t, half=False):
    """-1 on the first column of a pair, +1 on the second, [1, width of t]."""
    hd = torch.arange(HD)
    first = (hd < HD // 2) if half else (hd % 2 == 0)
    sg = torch.where(first, -1.0, 1.0).to(t.dtype).to(t.device)
    return sg.repeat(t.shape[1] // HD)[None]


def _tab(c, width):
    return c.repeat(1, width // HD)


def rot(t, cos, sin, et=None, half=False):
    """(Rot(t), its error sum): t [R, k*64], cos / sin [R,64] used by every head."""
    c, s = _tab(cos, t.shape[1]), _tab(sin, t.shape[1])
    a, b = t * c, _sign(t, half) * _swap(t, half) * s
    o = a + b
    et = torch.zeros_like(t) if et is None else et
    return o, c.abs() * et + s.abs() * _swap(et, half) + a.abs() + b.abs() + o.abs()


def rot_t(g, cos, sin, eg=None, half=False):
    """(Rot^T(g), its error sum)."""
    c, s = _tab(cos, g.shape[1]), _tab(sin, g.shape[1])
    a, b = g * c, -_sign(g, half) * _swap(g * s, half)
    o = a + b
    eg = torch.zeros_like(g) if eg is None else eg
    return o, c.abs() * eg + _swap(s.abs() * eg, half) + a.abs() + b.abs() + o.abs()


# ---- the core -----------------------------------------------------------------------------------------------------------
def _sides(rows, b, m, n, heads=HEADS):
    """[B*M + B*N, heads*hd] -> [[B,heads,M,hd], [B,heads,N,hd]]."""
    hd = rows.shape[1] // heads
    return [rows[:b * m].reshape(b, m, heads, hd).transpose(1, 2), rows[b * m:].reshape(b, n, heads, hd).transpose(1, 2)]


def _merge(t0, t1):
    b, h, m, hd = t0.shape
    n = t1.shape[2]
    return torch.cat([t0.transpose(1, 2).reshape(b * m, h * hd), t1.transpose(1, 2).reshape(b * n, h * hd)], 0)


def attention_forward(qkv, b, m, n, scale=SCALE):
    """ctx [R,256] of the self attention on rotated q' | k' | v, in the precision of its input."""
    out = []
    for q, k, v in zip(_sides(qkv[:, :D], b, m, n), _sides(qkv[:, D:2 * D], b, m, n), _sides(qkv[:, 2 * D:], b, m, n)):
        out.append(torch.softmax(scale * (q @ k.transpose(-1, -2)), -1) @ v)
    return _merge(*out)


def attention_backward(qkv, ctx, dctx, cos, sin, b, m, n, scale=SCALE, variant=None, err=None):
    """qkv [R,768] (q' | k' | v, rotated), ctx, dctx [R,256], cos / sin [R,64] or None, float64.
    -> (dqkv [R,768], its error sums).  err: {name: the error sum its operand arrives with}, of qkv, ctx, dctx."""
    err = err or {}
    eqkv = err.get("qkv", torch.zeros_like(qkv))
    ab, t = torch.abs, lambda x: x.transpose(-1, -2)  # noqa: E731
    dheads = 1 if variant == "D_all_columns" else HEADS
    outs = {k: [] for k in ("dq", "dk", "dv", "edq", "edk", "edv")}
    sp = lambda x, h=HEADS: _sides(x, b, m, n, h)  # noqa: E731
    per_side = zip(sp(qkv[:, :D]), sp(qkv[:, D:2 * D]), sp(qkv[:, 2 * D:]), sp(ctx, dheads), sp(dctx, dheads), sp(dctx),
                   sp(eqkv[:, :D]), sp(eqkv[:, D:2 * D]), sp(eqkv[:, 2 * D:]), sp(err.get("ctx", torch.zeros_like(ctx)), dheads),
                   sp(err.get("dctx", torch.zeros_like(dctx))), (m, n))
    for q, k, v, c, gd, g, eq, ek, ev, ec, eg, rows in per_side:
        s = scale * (q @ t(k))
        es = scale * (_e(HD) * (ab(q) @ t(ab(k))) + eq @ t(ab(k)) + ab(q) @ t(ek)) + ab(s)
        dim = -2 if variant == "softmax_over_queries" else -1
        lse = torch.logsumexp(s, dim, keepdim=True)
        p = torch.exp(s - lse)
        el = (p * es).sum(dim, keepdim=True) + _e(rows) + 4 + ab(lse)
        ep = p * (es + el + ab(s - lse) + 2) + TINY
        tt = g @ t(v)
        et = _e(HD) * (ab(g) @ t(ab(v))) + eg @ t(ab(v)) + ab(g) @ t(ev)
        egd = eg if dheads == HEADS else torch.zeros_like(gd)
        dd = (gd * c).sum(-1, keepdim=True)
        ed = (_e(HD) * ab(gd * c) + egd * ab(c) + ab(gd) * ec).sum(-1, keepdim=True)
        ds = p * (tt - dd)
        eds = ep * ab(tt - dd) + p * (et + ed) + 2 * ab(ds)
        kq = {"no_scale": 1.0, "scale_twice": scale * scale}.get(variant, scale)
        dq = kq * (ds @ k)
        edq = scale * (eds @ ab(k) + _e(rows) * (ab(ds) @ ab(k)) + ab(ds) @ ek) + ab(dq)
        left = p if variant == "dk_from_P" else ds
        dk = kq * ((left if variant == "dS_not_transposed" else t(left)) @ q)
        edk = scale * (t(eds) @ ab(q) + _e(rows) * (t(ab(ds)) @ ab(q)) + t(ab(ds)) @ eq) + ab(dk)
        dv = t(p) @ g
        edv = t(ep) @ ab(g) + _e(rows) * (t(p) @ ab(g)) + t(p) @ eg
        for name, val in (("dq", dq), ("dk", dk), ("dv", dv), ("edq", edq), ("edk", edk), ("edv", edv)):
            outs[name].append(val)
    dq, dk, dv, edq, edk, edv = (_merge(*outs[k]) for k in ("dq", "dk", "dv", "edq", "edk", "edv"))
    if cos is not None:
        half = variant == "pair_half"
        back = rot if variant == "rot_not_transposed" else rot_t
        dq, edq = back(dq, cos, sin, edq, half=half)
        if variant != "dk_not_unrotated":
            dk, edk = back(dk, cos, sin, edk, half=half)
        if variant == "dv_rotated":
            dv = rot_t(dv, cos, sin)[0]
    return torch.cat([dq, dk, dv], 1), torch.cat([edq, edk, edv], 1)


# ---- the block entry ----------------------------------------------------------------------------------------------------
def qkv_forward(x, cos, sin, wqkv, bqkv, ex=None):
    """(q' | k' | v [R,768], its error sum) as gfc_linear evaluates it: Wqkv, bqkv in packed order."""
    y = x @ wqkv.t() + bqkv
    e = (_e(D) + 1) * (x.abs() @ wqkv.abs().t() + bqkv.abs())
    if ex is not None:
        e = e + ex @ wqkv.abs().t()
    o, eo = rot(y[:, :2 * D], cos, sin, e[:, :2 * D])
    return torch.cat([o, y[:, 2 * D:]], 1), torch.cat([eo, e[:, 2 * D:]], 1)


def backward(x, cos, sin, ctx, dctx, dx_in, wqkv, bqkv, b, m, n, variant=None, err=None):
    """The block entry: x, ctx, dctx [R,256], cos / sin [R,64], dx_in [R,256] or None, Wqkv [768,256] and bqkv [768] in
    PACKED order (float64).  -> (grads, error sums) keyed by OUTPUTS, the parameter gradients in packed order:
    `dx_att` = dqkv Wqkv, the attention's share alone, `dx` = dx_in + dx_att (dx_att itself without dx_in).
    err: error sums the operands arrive with ({"x", "ctx", "dctx", "dx_in"})."""
    err = err or {}
    ex = err.get("x")
    qkv, eqkv = qkv_forward(x, cos, sin, wqkv, bqkv, ex)
    core_err = {"qkv": eqkv, **{k: err[k] for k in ("ctx", "dctx") if k in err}}
    dqkv, edqkv = attention_backward(qkv, ctx, dctx, cos, sin, b, m, n, variant=variant, err=core_err)
    rows = x.shape[0]
    red = _e(rows) + 2
    exa = torch.zeros_like(x) if ex is None else ex
    dw = dqkv.t() @ x
    if variant == "row_order_confused":  # the packed gradient taken for one in state-dict order
        dw = to_packed(dw)
    grads = {"dWqkv": dw, "dbqkv": dqkv.sum(0)}
    errs = {"dWqkv": edqkv.t() @ x.abs() + red * (dqkv.abs().t() @ x.abs()) + dqkv.abs().t() @ exa,
            "dbqkv": (edqkv + red * dqkv.abs()).sum(0)}
    w_used = wqkv[:2 * D] if variant == "dx_no_v" else wqkv
    att = dqkv[:, :w_used.shape[0]] @ w_used
    eatt = edqkv @ wqkv.abs() + _e(3 * D) * (dqkv.abs() @ wqkv.abs()) + att.abs()
    grads["dx_att"], errs["dx_att"] = att, eatt
    if dx_in is None:
        grads["dx"], errs["dx"] = att, eatt
    else:
        grads["dx"] = dx_in + att
        errs["dx"] = eatt + err.get("dx_in", 0.0) + grads["dx"].abs()
    return grads, errs


# ---- the whole self block and the layer's input rows --------------------------------------------------------------------
STAGE_NAMES = {"Wout": "out_proj.weight", "bout": "out_proj.bias", "W0": "ffn.0.weight", "b0": "ffn.0.bias",
               "gamma": "ffn.1.weight", "beta": "ffn.1.bias", "W3": "ffn.3.weight", "b3": "ffn.3.bias"}
BLOCK_OUTPUTS = ("dWout", "dbout", "dW0", "db0", "dgamma", "dbeta", "dW3", "db3", "dWqkv", "dbqkv", "dx", "layer_input")


def stage_params(sd, layer):
    """(the eight FFN-part tensors of `transformers.{layer}.self_attn` keyed as tests/output_stage_reference.py takes
    them, Wqkv and bqkv in PACKED order) out of a state dict."""
    pre = f"transformers.{layer}.self_attn."
    return ({k: sd[pre + v] for k, v in STAGE_NAMES.items()}, to_packed(sd[pre + "Wqkv.weight"]),
            to_packed(sd[pre + "Wqkv.bias"]))


def block_backward(x, cos, sin, ctx, dy, head_dx, p, wqkv, bqkv, b, m, n, variant=None, erf_abs=0.0, in_err=0.0,
                   dy_err=None, head_err=None):
    """The last self block's backward as `layer_loss_backward(self_block=True)` chains it: the FFN part through
    tests/output_stage_reference.py (x: the rows of layer L - 2, ctx: the self attention's context, dy: the complete
    gradient at the block's output), its dctx / dx_in into `backward` above, and
        layer_input = dx + head_dx        head L - 2's direct gradient at the same rows (one more addition).
    -> (grads, per-element BOUNDS) keyed by BLOCK_OUTPUTS, Wqkv's in PACKED order.  The FFN part's bound (its error sum
    and its erf term with erf_abs) is carried into the attention part as the error its dctx and dx_in arrive with.
    in_err: the error x, ctx and dy arrive with, in units of 2^-23 of their magnitudes; dy_err / head_err: error sums of
    dy / head_dx on top, as tensors.  A dy_err is turned into the scalar form the FFN part takes row by row: a row's sum of
    errors over its sum of magnitudes, the largest row's (the products that follow sum over a row's columns)."""
    import output_stage_reference as osr

    rel = in_err
    if dy_err is not None:
        rel = rel + float((dy_err.sum(1) / dy.abs().sum(1).clamp(min=1e-300)).max())
    fg, sums, erfs = osr.backward(x, ctx, dy, p, in_err=rel)
    ftol = osr.bounds(sums, erfs, erf_abs)
    err = {"dctx": ftol["dctx"] / U, "dx_in": ftol["dx_in"] / U}
    if in_err:
        err.update(x=in_err * x.abs(), ctx=in_err * ctx.abs())
    ag, aerrs = backward(x, cos, sin, ctx, fg["dctx"], fg["dx_in"], wqkv, bqkv, b, m, n,
                         variant=variant if variant in VARIANTS else None, err=err)
    atol = bounds(aerrs)
    grads = {k: fg[k] for k in BLOCK_OUTPUTS[:8]}
    tol = {k: ftol[k] for k in BLOCK_OUTPUTS[:8]}
    for k in ("dWqkv", "dbqkv", "dx"):
        grads[k], tol[k] = ag[k], atol[k]
    grads["layer_input"] = ag["dx"] if variant == "no_head_term" else ag["dx"] + head_dx
    tol["layer_input"] = atol["dx"] + U * ((0.0 if head_err is None else head_err) + in_err * head_dx.abs()
                                           + grads["layer_input"].abs())
    return grads, tol


def bounds(errs, extra=0.0):
    """{output: the per-element bound}: 2^-23 * (1 + extra) * error sum."""
    return {k: (1.0 + extra) * U * v for k, v in errs.items()}


def worst_ratio(y, ref, tol):
    """max over elements of |y - ref| / tol; NaN or inf in y counts as infinite; 0 / 0 as 0."""
    e = (y.double() - ref).abs()
    r = torch.where((e == 0) & (tol == 0), torch.zeros_like(e), e / tol)
    return float(r.nan_to_num(nan=float("inf"), posinf=float("inf")).max())


# ---- an fp32 emulation --------------------------------------------------------------------------------------------------
def emulate_float32(x, cos, sin, ctx, dctx, dx_in, wqkv, bqkv, b, m, n):
    """The closed form evaluated in float32 torch, stage by stage, every intermediate rounded (no error sums)."""
    f = lambda t: None if t is None else t.float()  # noqa: E731
    x, cos, sin, ctx, dctx, dx_in, wqkv, bqkv = map(f, (x, cos, sin, ctx, dctx, dx_in, wqkv, bqkv))
    y = x @ wqkv.t() + bqkv
    qkv = torch.cat([rot(y[:, :2 * D], cos, sin)[0], y[:, 2 * D:]], 1)
    dq, dk, dv = [], [], []
    for q, k, v, c, g in zip(*(_sides(t, b, m, n) for t in (qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ctx, dctx))):
        s = SCALE * (q @ k.transpose(-1, -2))
        p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
        ds = p * (g @ v.transpose(-1, -2) - (g * c).sum(-1, keepdim=True))
        dq.append(SCALE * (ds @ k))
        dk.append(SCALE * (ds.transpose(-1, -2) @ q))
        dv.append(p.transpose(-1, -2) @ g)
    dqkv = torch.cat([rot_t(_merge(*dq), cos, sin)[0], rot_t(_merge(*dk), cos, sin)[0], _merge(*dv)], 1)
    att = dqkv @ wqkv
    return {"dWqkv": dqkv.t() @ x, "dbqkv": dqkv.sum(0), "dx_att": att, "dx": att if dx_in is None else dx_in + att}


# ---- data ---------------------------------------------------------------------------------------------------------------
def random_tables(rows, gen, equal_pairs=True):
    """cos, sin [rows,64] float32 of random angles; with equal_pairs both columns of a pair hold the same entry (what the
    positional encoding makes), without it every column has an angle of its own: the general transpose."""
    ang = torch.rand((rows, HD // 2 if equal_pairs else HD), generator=gen) * (2 * math.pi)
    if equal_pairs:
        ang = ang.repeat_interleave(2, -1)
    return torch.cos(ang).float(), torch.sin(ang).float()


def random_core(b, m, n, seed, dctx_sign=None, q_gain=3.0, equal_pairs=True):
    """(qkv, ctx, dctx, cos, sin) float32 for the core alone: q', k' of a spread that gives soft-max rows whose maximum
    is several times uniform, ctx the float32 rounding of the float64 forward on them."""
    g = torch.Generator().manual_seed(seed)
    rows = b * (m + n)
    qkv = torch.randn((rows, 3 * D), generator=g)
    qkv[:, :2 * D] *= q_gain / HD ** 0.25
    dctx = torch.randn((rows, D), generator=g) * 1e-3
    if dctx_sign is not None:
        dctx = dctx.abs() * dctx_sign
    cos, sin = random_tables(rows, g, equal_pairs)
    ctx = attention_forward(qkv.double(), b, m, n).float()
    return qkv, ctx, dctx, cos, sin


def random_params(gen, gain=2.0):
    """Wqkv, bqkv in STATE-DICT order with the magnitudes of a trained block: rows of norm about `gain` for q and k (so
    that the soft-max rows are not flat), about 1 for v; float32."""
    w = torch.randn((3 * D, D), generator=gen) / D ** 0.5
    bias = torch.randn((3 * D,), generator=gen) * 0.1
    s = torch.arange(3 * D) % 3
    w[s < 2] *= gain
    return w, bias


def random_block(b, m, n, seed):
    """(x, cos, sin, ctx, dctx, dx_in, Wqkv, bqkv) float32, the parameters in PACKED order; ctx is the float64 forward,
    rounded; dx_in two hundred times the attention's share, as at the last layer."""
    g = torch.Generator().manual_seed(seed)
    rows = b * (m + n)
    w, bias = random_params(g)
    w, bias = to_packed(w), to_packed(bias)
    x = torch.randn((rows, D), generator=g)
    dctx = torch.randn((rows, D), generator=g) * 1e-3
    dx_in = torch.randn((rows, D), generator=g) * 0.2
    cos, sin = random_tables(rows, g)
    qkv, _ = qkv_forward(x.double(), cos.double(), sin.double(), w.double(), bias.double())
    ctx = attention_forward(qkv, b, m, n).float()
    return x, cos, sin, ctx, dctx, dx_in, w, bias


# ---- conditioning cases on exact data -----------------------------------------------------------------------------------
def identical_keys_case(seed=3):
    """B = 1, M = N = 64, side 1's 64 rows all one row (q', k' and v): every P of side 1 is 1 / 64 and its rows are
    indistinguishable as keys with identical dctx, so dk's and dv's rows of side 1 are the same bits.  Integer-valued
    data over 8: every dot product of depth 64 is exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    m = n = 64
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float() / 8  # noqa: E731
    qkv = torch.cat([ri(m, 3 * D), ri(1, 3 * D).expand(n, 3 * D)], 0).contiguous()
    dctx = torch.cat([ri(m, D), ri(1, D).expand(n, D)], 0).contiguous() / 128
    ctx = attention_forward(qkv.double(), 1, m, n).float()
    return qkv, ctx, dctx, (1, m, n)


def dominant_key_case(m=37, n=70, key=33):
    """B = 1: on both sides every q' is 40 e_0 per head, row `key` has k' = 40 e_0 and every other row k' = 0, so scale S
    is 200 at that key and 0 elsewhere: a gap of 200, where exp underflows to 0 in fp32 and P is exactly one-hot.  v is
    integer-valued, dctx integer-valued over 1024: ctx = v[key] exactly, dctx . v[key] - D is exactly 0, so dS, dq and dk
    are exact zeros and dv is zero but for row `key` of each side, which holds the column sums of that side's dctx."""
    g = torch.Generator().manual_seed(17)
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()  # noqa: E731
    qkv = torch.zeros((m + n, 3 * D))
    qkv[:, 0:D:HD] = 40.0
    qkv[key, D:2 * D:HD] = 40.0
    qkv[m + key, D:2 * D:HD] = 40.0
    qkv[:, 2 * D:] = ri(m + n, D)
    dctx = ri(m + n, D) / 1024
    ctx = attention_forward(qkv.double(), 1, m, n).float()
    return qkv, ctx, dctx, (1, m, n), key
