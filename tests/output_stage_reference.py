"""Float64 closed form of the backward of one LightGlue FFN block with the projection in front of it (`to_out` /
`out_proj`, the concatenation, Linear(512,512) -> LayerNorm(512) -> GELU -> Linear(512,256) and the residual), written
from the reference's text: gluefactory/models/matchers/lightglue.py:143-148 (the FFN), :160-164 and :219-222 (the blocks
that call it).  Test infrastructure: CPU torch only.  No autograd: the host test holds the closed form to torch's own
float64 autograd on the same block.

R rows, d = 256:
    m = ctx Wout^T + bout          h = [x | m] W0^T + b0        mu, rstd (biased variance, eps 1e-5)
    n = (h - mu) rstd              u = n gamma + beta           a = u Phi(u)         y = x + a W3^T + b3
    da = dy W3                     dW3 = dy^T a                 db3 = sum dy
    du = da (Phi(u) + u phi(u))    dgamma = sum du n            dbeta = sum du
    dn = du gamma                  dh = rstd (dn - mean(dn) - n mean(dn n))
    dW0 = dh^T [x | m]             db0 = sum dh                 dcat = dh W0
    dm = dcat[:, 256:]             dWout = dm^T ctx             dbout = sum dm
    dx_in = dy + dcat[:, :256]     dctx = dm Wout  (dm itself without Wout)

Beside every output element stands its ERROR SUM, in units of 2^-23: the project's c * abs-sum (tests/
head_grad_reference.py) added up stage by stage instead of multiplied through.  Every stage adds its own c * abs-sum --
c the roundings of that stage, a sum of K terms charged E(K) = sqrt(K) + 1 times the sum of the absolute values of its
terms, with the float64 magnitudes of the factors -- and passes on what it received by the first-order rule of the stage:
    a sum y = A x of K terms        err(y) = |A| err(x) + E(K) |A| |x|
    a product z = a b               err(z) = |b| err(a) + |a| err(b) + |z|
    LayerNorm                       err(n) = rstd (err(h) + mean err(h)) + |n| rstd rms(err(h))   (an error in h moves n_j
                                    by rstd times it, the mean by its mean, and rstd by rstd^3 mean((h - mu) err) <=
                                    rstd^2 rms(err) relative, by Cauchy-Schwarz) + rstd E(512) mean|h| (the mean's own sum)
                                    + (2 E(512) + 6) |n| (the variance's sum, sqrt, reciprocal, subtraction, product)
    GELU                            g(u) = Phi(u) + u phi(u), g'(u) = (2 - u^2) phi(u): err(g) = |g'| err(u) + 8 (Phi +
                                    |u| phi); a = u Phi: err(a) = |g| err(u) + 8 |a|   (8: the erf polynomial, exp, the
                                    products, the sum)
The multiplied form would charge the abs-sum ratios of h (about 20), of n (about 40, squared in n mean(dn n)) and of da
(about 20) as one product, 10^7 times the rounding error of fp32, and no wrong variant could miss it; the added form is
the same first-order analysis without that.  The constants depend on the shape alone; none is fitted to a result.
With `exact_h` (the conditioning cases: integer data, h and every row sum of it exact in fp32 in any order) err(h) and
the term of the mean's own sum are 0.
An fp32 evaluation in another order differs from the float64 value by at most
    2^-23 * error sum + ERF_ABS / 2 * erf-sum      per element,
where the second term is the documented absolute error of the default build's erf (csrc/common.h: Abramowitz & Stegun
7.1.26, 1.5e-7 in exact arithmetic, 5.6e-7 evaluated in fp32), which is not a rounding error and does not scale with any
operand: Phi = (1 + erf) / 2 carries half of it, and the erf-sum is what one unit of error in every Phi adds to the
element by the same first-order rules (|da| in du, |u| in a).  The exact-erf build is held to ERF_ABS = 0.

`variant` switches ONE deliberate mistake on (VARIANTS); the host test shows that each misses a bound widely.
"""
import math

import torch

U = 2.0 ** -23
D = 256
H = 512
EPS = 1e-5
ERF_ABS = 5.6e-7  # csrc/common.h, gfc_gelu: the A&S erf evaluated in fp32
VARIANTS = ("one_pass_var", "no_eps", "unbiased_var", "no_n_term", "no_mean_term", "tanh_gelu", "phi_only",
            "no_residual", "folded_w0", "dwout_transposed", "dbout_from_dh", "halves_swapped")
# The descent check: the step, and the float64 ratio (total(theta - eps grad) - total(theta)) / (-eps |grad|^2) the host
# test measures on the two cases at loss.gamma 1 and the GPU test compares its own with.
DESCENT_EPS = 0.005
DESCENT_RATIO = {"a": 0.9859, "b": 0.9658}
OUTPUTS = ("dWout", "dbout", "dW0", "db0", "dgamma", "dbeta", "dW3", "db3", "dx_in", "dctx")


def _e(k):
    return math.sqrt(k) + 1.0


def _phi(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _cdf(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))


def forward(x, ctx, p):
    """y [R,256] of the block in the precision of its inputs; p: Wout, bout (or None, None), W0, b0, gamma, beta, W3, b3."""
    m = ctx if p["Wout"] is None else ctx @ p["Wout"].t() + p["bout"]
    h = torch.cat([x, m], 1) @ p["W0"].t() + p["b0"]
    u = torch.nn.functional.layer_norm(h, (H,), p["gamma"], p["beta"], EPS)
    return x + torch.nn.functional.gelu(u) @ p["W3"].t() + p["b3"]


def fold(p):
    """ffn.0 with to_out folded into its message half, as LightGlue._pack stores it: (W0', b0')."""
    w0, wo = p["W0"], p["Wout"]
    return torch.cat([w0[:, :D], w0[:, D:] @ wo], 1), p["b0"] + w0[:, D:] @ p["bout"]


def backward(x, ctx, dy, p, variant=None, exact_h=False, in_err=0.0):
    """x, ctx, dy [R,256] and the parameters p (float64).  -> (grads, error_sums, erf_sums), each keyed by OUTPUTS (dWout
    and dbout absent without Wout).  in_err: the error x, ctx and dy arrive with, in units of 2^-23 of their magnitudes
    (a comparison ACROSS two evaluations of the trunk); it is passed on by the same first-order rules."""
    wout, bout, w0, b0, gamma, beta, w3 = (p[k] for k in ("Wout", "bout", "W0", "b0", "gamma", "beta", "W3"))
    with_out = wout is not None
    rows = x.shape[0]
    red = _e(rows) + 2
    mean = lambda t: t.mean(1, keepdim=True)  # noqa: E731
    ex, ectx, edy = in_err * x.abs(), in_err * ctx.abs(), in_err * dy.abs()
    if with_out:
        m = ctx @ wout.t() + bout
        em = (_e(D) + 1) * (ctx.abs() @ wout.abs().t() + bout.abs()) + ectx @ wout.abs().t()
    else:
        m, em = ctx, ectx
    cat, ecat = torch.cat([x, m], 1), torch.cat([ex, em], 1)
    if variant == "halves_swapped":
        cat = torch.cat([m, x], 1)
    h = cat @ w0.t() + b0
    eh = ecat @ w0.abs().t() + (_e(H) + 1) * (cat.abs() @ w0.abs().t() + b0.abs())
    mu = mean(h)
    c = h - mu
    if variant == "one_pass_var":  # E[h^2] - mu^2 as fp32 evaluates it
        hf = h.float()
        var = ((hf * hf).sum(1, keepdim=True) * (1.0 / H) - hf.mean(1, keepdim=True) ** 2).double()
    elif variant == "unbiased_var":
        var = (c * c).sum(1, keepdim=True) / (H - 1)
    else:
        var = mean(c * c)
    rstd = 1.0 / torch.sqrt(var + (0.0 if variant == "no_eps" else EPS))
    n = c * rstd
    own_mean = rstd * _e(H) * mean(h.abs())
    if exact_h:
        eh, own_mean = torch.zeros_like(h), 0.0
    rel = rstd * mean(eh * eh).sqrt()  # of rstd
    en = rstd * (eh + mean(eh)) + n.abs() * rel + own_mean + (2 * _e(H) + 6) * n.abs()
    er = rel + _e(H) + 3
    u = n * gamma + beta
    eu = en * gamma.abs() + 2 * ((n * gamma).abs() + beta.abs())
    cdf, pdf = _cdf(u), _phi(u)
    if variant == "tanh_gelu":
        k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
        t = torch.tanh(k0 * (u + k1 * u ** 3))
        g = 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * k0 * (1 + 3 * k1 * u * u)
    elif variant == "phi_only":
        g = cdf
    else:
        g = cdf + u * pdf
    g_true = cdf + u * pdf
    eg = ((2.0 - u * u) * pdf).abs() * eu + 8 * (cdf + u.abs() * pdf)
    a = u * cdf
    ea = g_true.abs() * eu + 8 * a.abs()
    da, eda = dy @ w3, _e(D) * (dy.abs() @ w3.abs()) + edy @ w3.abs()
    du = da * g
    du_true = da * g_true
    edu, fdu = g_true.abs() * eda + da.abs() * eg + du_true.abs(), da.abs()
    dn = du * gamma
    edn, fdn = edu * gamma.abs() + (du_true * gamma).abs(), fdu * gamma.abs()
    s1, s2 = mean(dn), mean(dn * n)
    es1 = mean(edn) + _e(H) * mean(dn.abs())
    es2 = mean(edn * n.abs() + dn.abs() * en + (dn * n).abs()) + _e(H) * mean((dn * n).abs())
    t1 = 0.0 if variant == "no_mean_term" else s1
    t2 = 0.0 if variant == "no_n_term" else n * s2
    dh = rstd * (dn - t1 - t2)
    dh_true = rstd * (dn - s1 - n * s2)
    edh = rstd * (edn + es1 + en * s2.abs() + n.abs() * es2 + 3 * (dn.abs() + s1.abs() + (n * s2).abs())) + dh_true.abs() * er
    fdh = rstd * (fdn + mean(fdn) + n.abs() * mean(fdn * n.abs()))
    dcat = dh @ w0
    edcat, fdcat = edh @ w0.abs() + _e(H) * (dh_true.abs() @ w0.abs()), fdh @ w0.abs()
    dm, edm, fdm = dcat[:, D:], edcat[:, D:], fdcat[:, D:]
    if variant == "halves_swapped":
        dm = dcat[:, :D]
    lo = dcat[:, :D]
    grads = {"dW3": dy.t() @ a, "db3": dy.sum(0), "dgamma": (du * n).sum(0), "dbeta": du.sum(0), "dW0": dh.t() @ cat,
             "db0": dh.sum(0), "dx_in": lo + (0.0 if variant == "no_residual" else dy)}
    errs = {"dW3": dy.abs().t() @ ea + red * (dy.abs().t() @ a.abs()) + edy.t() @ a.abs(),
            "db3": (_e(rows) + 1) * dy.abs().sum(0) + edy.sum(0),
            "dgamma": (edu * n.abs() + du_true.abs() * en + (1 + red) * (du_true * n).abs()).sum(0),
            "dbeta": (edu + red * du_true.abs()).sum(0),
            "dW0": edh.t() @ cat.abs() + dh_true.abs().t() @ ecat + red * (dh_true.abs().t() @ cat.abs()),
            "db0": (edh + red * dh_true.abs()).sum(0), "dx_in": edcat[:, :D] + dy.abs() + lo.abs() + edy}
    erfs = {"dW3": dy.abs().t() @ u.abs(), "db3": torch.zeros(D, dtype=dy.dtype, device=dy.device),
            "dgamma": (fdu * n.abs()).sum(0), "dbeta": fdu.sum(0), "dW0": fdh.t() @ cat.abs(), "db0": fdh.sum(0),
            "dx_in": fdcat[:, :D]}
    if variant == "halves_swapped":
        grads["dx_in"] = dcat[:, D:] + dy
    if with_out:
        grads["dWout"] = ctx.t() @ dm if variant == "dwout_transposed" else dm.t() @ ctx
        grads["dbout"] = dh[:, :D].sum(0) if variant == "dbout_from_dh" else dm.sum(0)
        grads["dctx"] = dm @ wout
        errs["dWout"] = edm.t() @ ctx.abs() + red * (dm.abs().t() @ ctx.abs()) + dm.abs().t() @ ectx
        errs["dbout"] = (edm + red * dm.abs()).sum(0)
        errs["dctx"] = edm @ wout.abs() + _e(D) * (dm.abs() @ wout.abs())
        erfs["dWout"], erfs["dbout"], erfs["dctx"] = fdm.t() @ ctx.abs(), fdm.sum(0), fdm @ wout.abs()
        if variant == "folded_w0":  # the gradient of the folded W0' = [W0a | W0b Wout]: dh^T [x | ctx]
            grads["dW0"] = dh.t() @ torch.cat([x, ctx], 1)
    else:
        grads["dctx"], errs["dctx"], erfs["dctx"] = dm, edm, fdm
    return grads, errs, erfs


def bounds(errs, erfs, erf_abs=ERF_ABS, extra=0.0):
    """{output: the per-element bound}: 2^-23 * (1 + extra) * error sum + erf_abs / 2 * erf-sum."""
    return {k: (1.0 + extra) * U * errs[k] + 0.5 * erf_abs * erfs[k] for k in errs}


def worst_ratio(y, ref, tol):
    """max over elements of |y - ref| / tol; NaN or inf in y counts as infinite; 0 / 0 as 0."""
    err = (y.double() - ref).abs()
    r = torch.where((err == 0) & (tol == 0), torch.zeros_like(err), err / tol)
    return float(r.nan_to_num(nan=float("inf"), posinf=float("inf")).max())


def random_params(gen, with_out=True, scale=1.0):
    """A block's parameters with the magnitudes of a trained one: rows of W of norm about 1, float32."""
    r = lambda *s: torch.randn(*s, generator=gen)
    p = {"Wout": r(D, D) / D ** 0.5 * scale if with_out else None, "bout": r(D) * 0.1 if with_out else None,
         "W0": r(H, H) / H ** 0.5 * scale, "b0": r(H) * 0.1, "gamma": 1.0 + 0.2 * r(H), "beta": 0.1 * r(H),
         "W3": r(D, H) / H ** 0.5 * scale, "b3": r(D) * 0.1}
    return p


def to64(p):
    return {k: None if v is None else v.double() for k, v in p.items()}


# ---- conditioning rows: integer data, so that h is exact in fp32 in any order of accumulation -----------------------
COND_R = 133            # a full 128-row chunk and a tail of 5
COND_CONST = (7, 64, 130)
COL_POS, COL_NEG, COL_G0 = slice(0, 4), slice(4, 8), slice(8, 16)


def conditioning_case(offset):
    """NULL-Wout block whose pre-activation is exact: [x | ctx] integers in [-1, 1], two entries of +-1 per row of W0,
    b0 = offset (4096: rows of mean about 4096 and spread about 1.2, where E[h^2] - mu^2 loses the variance; 0: rows of
    mean about 0).  Rows COND_CONST hold zeros: h is constant there, the variance exactly 0, and eps decides.  Columns
    COL_POS / COL_NEG have gamma = 0 and beta = +-1e4 (u = +-1e4 in every row: a derivative of exactly 1 / 0), COL_G0
    gamma = 0 with an ordinary beta."""
    g = torch.Generator().manual_seed(11 + int(offset))
    a = torch.randint(-1, 2, (COND_R, H), generator=g).float()
    a[list(COND_CONST)] = 0
    w0 = torch.zeros(H, H)
    idx = torch.rand(H, H, generator=g).argsort(1)[:, :2]
    w0.scatter_(1, idx, torch.randint(0, 2, (H, 2), generator=g).float() * 2 - 1)
    p = random_params(g, False)
    p["W0"], p["b0"] = w0, torch.full((H,), float(offset))
    p["gamma"][COL_POS], p["gamma"][COL_NEG], p["gamma"][COL_G0] = 0.0, 0.0, 0.0
    p["beta"][COL_POS], p["beta"][COL_NEG] = 1e4, -1e4
    h32 = a @ w0.t() + p["b0"]
    h64 = a.double() @ w0.double().t() + p["b0"].double()
    assert torch.equal(h32.double(), h64) and float(h64.abs().sum(1).max()) < 2 ** 24  # exact, and so is every row sum
    sd = h64.std(1, unbiased=False)
    rest = [r for r in range(COND_R) if r not in COND_CONST]
    assert bool((sd[list(COND_CONST)] == 0).all()) and 0.5 < float(sd[rest].min()) and float(sd[rest].max()) < 2.5
    dy = torch.randint(-8, 9, (COND_R, D), generator=g).float() / 1024
    return a[:, :D].contiguous(), a[:, D:].contiguous(), dy, p


# ---- the last layer's output stage of a whole matcher, formed on the CPU in float64 ---------------------------------
STAGE_NAMES = {"Wout": "to_out.weight", "bout": "to_out.bias", "W0": "ffn.0.weight", "b0": "ffn.0.bias",
               "gamma": "ffn.1.weight", "beta": "ffn.1.bias", "W3": "ffn.3.weight", "b3": "ffn.3.bias"}


def stage_params(sd, layer):
    """The eight tensors of `transformers.{layer}.cross_attn` out of a state dict, keyed as `backward` takes them."""
    pre = f"transformers.{layer}.cross_attn."
    return {k: sd[pre + v] for k, v in STAGE_NAMES.items()}


def stage_inputs(olg, sd, case, n_layers, heads=4):
    """(xs0, xs1, x, ctx): every layer's descriptors of `case` from the CPU oracle (oracle/lightglue.py, `olg`) in the
    precision of `sd`, the rows [B*M + B*N, 256] the last cross block reads, and its attention context.  The context is
    what the oracle's cross block hands to `to_out`: read there, by wrapping the oracle's `_linear` for that one call."""
    f = lambda t: t.to(sd["posenc.Wr.weight"].dtype)  # noqa: E731
    out = olg.match(sd, f(case["keypoints0"]), f(case["keypoints1"]), f(case["descriptors0"]), f(case["descriptors1"]),
                    f(case["size"]), f(case["size"]), n_layers=n_layers, return_layers=True)
    xs0, xs1 = [a for a, _ in out["layers"]], [b for _, b in out["layers"]]
    last = n_layers - 1
    e0 = olg.positional_encoding(sd["posenc.Wr.weight"], olg.normalize_keypoints(f(case["keypoints0"]), f(case["size"])))
    e1 = olg.positional_encoding(sd["posenc.Wr.weight"], olg.normalize_keypoints(f(case["keypoints1"]), f(case["size"])))
    with torch.no_grad():
        x0 = olg.self_block(sd, f"transformers.{last}.self_attn", xs0[last - 1], e0, heads)
        x1 = olg.self_block(sd, f"transformers.{last}.self_attn", xs1[last - 1], e1, heads)
        seen, inner = [], olg._linear

        def spy(sd_, name, t):
            if name.endswith(".cross_attn.to_out"):
                seen.append(t)
            return inner(sd_, name, t)

        olg._linear = spy
        try:
            y0, y1 = olg.cross_block(sd, f"transformers.{last}.cross_attn", x0, x1, heads)
        finally:
            olg._linear = inner
    assert len(seen) == 2 and torch.equal(y0, xs0[last]) and torch.equal(y1, xs1[last])
    rows = lambda a, b: torch.cat([a.reshape(-1, D), b.reshape(-1, D)], 0)  # noqa: E731
    return xs0, xs1, rows(x0, x1), rows(seen[0], seen[1])
