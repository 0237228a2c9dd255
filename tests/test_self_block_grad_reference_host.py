"""The float64 closed form of the self-attention backward (tests/self_block_grad_reference.py) against torch's autograd
of the block as the reference writes it (state-dict Wqkv, rotate_half, soft-max attention), its bounds against float32
evaluations, the wrong variants against the bounds, the conditioning cases, the row orders, and the tenth header; then
(second half) the reference's own autograd on the whole matcher (tests/golden/self_block_grad_*.npz, float64 and float32
run) against the closed form on the oracle's float64 block, the head term of the layer's input rows, and the descent
along the gradient of the 22 tensors of the last layer.  CPU only."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import self_block_grad_reference as sbr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

D = sbr.D


def rotate_half(x):
    """gluefactory/models/matchers/lightglue.py:43-46."""
    x = x.unflatten(-1, (-1, 2))
    x1, x2 = x.unbind(dim=-1)
    return torch.stack((-x2, x1), dim=-1).flatten(start_dim=-2)


def autograd(x, cos, sin, dctx, dx_in, w_sd, b_sd, shape, dtype):
    """({output: gradient, the parameters' in STATE-DICT order}, ctx) of sum(ctx * dctx) by torch's autograd on Wqkv, the
    rotary encoding and the attention as the reference builds them (lightglue.py:43-50, 124-129, 151-162), per side."""
    b, m, n = shape
    leaf = lambda t: t.detach().to(dtype).requires_grad_()  # noqa: E731
    w, bias, xl = leaf(w_sd), leaf(b_sd), leaf(x)
    ctxs = []
    for rows, cnt in ((slice(0, b * m), m), (slice(b * m, None), n)):
        xs = xl[rows].reshape(b, cnt, D)
        c, s = (t[rows].to(dtype).reshape(b, 1, cnt, sbr.HD) for t in (cos, sin))
        qkv = (xs @ w.t() + bias).unflatten(-1, (sbr.HEADS, -1, 3)).transpose(1, 2)
        q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
        q, k = q * c + rotate_half(q) * s, k * c + rotate_half(k) * s
        attn = torch.softmax(torch.einsum("...id,...jd->...ij", q, k) * q.shape[-1] ** -0.5, -1)
        ctxs.append(torch.einsum("...ij,...jd->...id", attn, v).transpose(1, 2).reshape(b * cnt, D))
    ctx = torch.cat(ctxs, 0)
    (ctx * dctx.to(dtype)).sum().backward()
    return {"dWqkv": w.grad, "dbqkv": bias.grad, "dx_att": xl.grad, "dx": dx_in.to(dtype) + xl.grad}, ctx.detach()


def bare_block(shape, seed=0, equal_pairs=True):
    """x, cos, sin, dctx, dx_in and Wqkv, bqkv in STATE-DICT order, float32."""
    b, m, n = shape
    g = torch.Generator().manual_seed(seed)
    rows = b * (m + n)
    w, bias = sbr.random_params(g)
    x = torch.randn((rows, D), generator=g)
    dctx = torch.randn((rows, D), generator=g) * 1e-3
    dx_in = torch.randn((rows, D), generator=g) * 0.2
    cos, sin = sbr.random_tables(rows, g, equal_pairs)
    return x, cos, sin, dctx, dx_in, w, bias


def closed_form(x, cos, sin, ctx, dctx, dx_in, w_sd, b_sd, shape, variant=None):
    """sbr.backward on float64 copies, the parameter gradients (and their error sums) mapped to STATE-DICT order."""
    d = lambda t: t.double()  # noqa: E731
    want, sums = sbr.backward(d(x), d(cos), d(sin), d(ctx), d(dctx), d(dx_in), sbr.to_packed(d(w_sd)),
                              sbr.to_packed(d(b_sd)), *shape, variant=variant)
    for out in (want, sums):
        for k in ("dWqkv", "dbqkv"):
            out[k] = sbr.to_state_dict(out[k])
    return want, sums


@pytest.mark.parametrize("equal_pairs", [True, False], ids=["posenc-tables", "general-tables"])
@pytest.mark.parametrize("shape", [(2, 37, 50), (1, 130, 65)], ids=lambda s: "x".join(map(str, s)))
def test_closed_form_equals_float64_autograd_and_bounds_hold_float32(shape, equal_pairs):
    x, cos, sin, dctx, dx_in, w, bias = bare_block(shape, equal_pairs=equal_pairs)
    ref, ctx = autograd(x, cos, sin, dctx, dx_in, w, bias, shape, torch.float64)
    want, sums = closed_form(x, cos, sin, ctx, dctx, dx_in, w, bias, shape)
    assert set(want) == set(ref) == set(sums) == set(sbr.OUTPUTS)
    for k in want:
        assert float(((want[k] - ref[k]).abs() / sums[k].clamp(min=1e-300)).max()) <= 1e-10, k
    f32, ctx32 = autograd(x, cos, sin, dctx, dx_in, w, bias, shape, torch.float32)
    want32, sums32 = closed_form(x, cos, sin, ctx32, dctx, dx_in, w, bias, shape)
    tol = sbr.bounds(sums32)
    used = {k: sbr.worst_ratio(f32[k], want32[k], tol[k]) for k in want}
    print("float32 autograd, fraction of the bound used: " + ", ".join(f"{k} {v:.2e}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, used
    emu = sbr.emulate_float32(x, cos, sin, ctx32, dctx, dx_in, sbr.to_packed(w), sbr.to_packed(bias), *shape)
    for k in ("dWqkv", "dbqkv"):
        emu[k] = sbr.to_state_dict(emu[k])
    used = {k: sbr.worst_ratio(emu[k], want32[k], tol[k]) for k in want}
    print("float32 emulation, fraction of the bound used: " + ", ".join(f"{k} {v:.2e}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, used
    # the soft-max rows are not flat: a wrong soft-max can be told apart
    qkv, _ = sbr.qkv_forward(x.double(), cos.double(), sin.double(), sbr.to_packed(w.double()), sbr.to_packed(bias.double()))
    q, k = sbr._sides(qkv[:, :D], *shape)[1], sbr._sides(qkv[:, D:2 * D], *shape)[1]
    prob = torch.softmax(sbr.SCALE * (q @ k.transpose(-1, -2)), -1)
    assert float((prob.max(-1).values * shape[2]).median()) > 2.0


def test_the_attention_share_is_the_small_part():
    """dx_in is two hundred times the attention's share: a test on the summed dx alone would not see it."""
    shape = (2, 37, 50)
    x, cos, sin, dctx, dx_in, w, bias = bare_block(shape)
    _, ctx = autograd(x, cos, sin, dctx, dx_in, w, bias, shape, torch.float64)
    want, _ = closed_form(x, cos, sin, ctx, dctx, dx_in, w, bias, shape)
    assert float(want["dx_att"].abs().max()) < 0.05 * float(want["dx"].abs().max())


# variant -> (the outputs among which it must miss a bound on the bare block (2, 37, 50), by at least this factor).
# Measured factors are printed by the test.
AIMED = {
    "rot_not_transposed": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "dk_not_unrotated": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "dv_rotated": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "pair_half": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "no_scale": (("dWqkv", "dx_att"), 100.0),
    "scale_twice": (("dWqkv", "dx_att"), 50.0),                            # dWqkv 78.7: scale is 1/8, a small change
    "softmax_over_queries": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "dk_from_P": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "D_all_columns": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "dS_not_transposed": (("dWqkv", "dbqkv", "dx_att"), 100.0),
    "row_order_confused": (("dWqkv",), 100.0),
    "dx_no_v": (("dx_att", "dx"), 20.0),                                   # 22.1: the v third of a K = 768 product
}
BELOW_100 = {"scale_twice", "dx_no_v"}  # the rule is 100; these two miss by less and are listed with their factors


def test_every_variant_is_listed():
    assert set(AIMED) == set(sbr.VARIANTS)


@pytest.mark.parametrize("variant", sbr.VARIANTS)
def test_wrong_variants_miss_a_bound(variant):
    outputs, factor = AIMED[variant]
    shape = (2, 37, 50)
    x, cos, sin, dctx, dx_in, w, bias = bare_block(shape)
    _, ctx = autograd(x, cos, sin, dctx, dx_in, w, bias, shape, torch.float64)
    want, sums = closed_form(x, cos, sin, ctx, dctx, dx_in, w, bias, shape)
    tol = sbr.bounds(sums)
    wrong, _ = closed_form(x, cos, sin, ctx, dctx, dx_in, w, bias, shape, variant=variant)
    ratios = {k: sbr.worst_ratio(wrong[k], want[k], tol[k]) for k in outputs}
    print(f"{variant}: misses by " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert (factor >= 100.0 or variant in BELOW_100) and max(ratios.values()) >= factor, ratios


def test_row_orders_are_inverse_and_the_library_s():
    """to_packed is the index LightGlue._pack builds (packed s*256 + head*64 + dd <- head*192 + dd*3 + s)."""
    idx = sbr.packed_index()
    assert sorted(idx.tolist()) == list(range(3 * D))
    for s, head, dd in ((0, 0, 0), (1, 0, 0), (2, 3, 63), (1, 2, 17)):
        assert int(idx[s * D + head * 64 + dd]) == head * 192 + dd * 3 + s
    t = torch.arange(3 * D * 2.0).reshape(3 * D, 2)
    assert torch.equal(sbr.to_state_dict(sbr.to_packed(t)), t) and not torch.equal(sbr.to_packed(t), t)


def test_rotation_and_its_transpose():
    """<Rot(t), g> = <t, Rot^T(g)> on general tables, and Rot is the reference's t cos + rotate_half(t) sin."""
    g = torch.Generator().manual_seed(1)
    cos, sin = (t.double() for t in sbr.random_tables(9, g, equal_pairs=False))
    t, u = torch.randn((9, D), generator=g).double(), torch.randn((9, D), generator=g).double()
    assert abs(float((sbr.rot(t, cos, sin)[0] * u).sum() - (t * sbr.rot_t(u, cos, sin)[0]).sum())) <= 1e-12
    ref = t * cos.repeat(1, 4) + rotate_half(t) * sin.repeat(1, 4)
    assert float((sbr.rot(t, cos, sin)[0] - ref).abs().max()) <= 1e-15


def test_conditioning_cases_are_what_they_say():
    qkv, ctx, dctx, shape = sbr.identical_keys_case()
    m = shape[1]
    want, _ = sbr.attention_backward(qkv.double(), ctx.double(), dctx.double(), None, None, *shape)
    assert float((want[m:, D:] - want[m:m + 1, D:]).abs().max()) <= 1e-18
    qkv, ctx, dctx, shape, key = sbr.dominant_key_case()
    m = shape[1]
    assert torch.equal(ctx[:m], qkv[key, 2 * D:].expand(m, D)) and torch.equal(ctx[m:], qkv[m + key, 2 * D:].expand(shape[2], D))
    want, errs = sbr.attention_backward(qkv.double(), ctx.double(), dctx.double(), None, None, *shape)
    assert float(want[:, :2 * D].abs().max()) < 1e-80
    exact = torch.zeros_like(want)
    exact[key, 2 * D:] = dctx[:m].double().sum(0)
    exact[m + key, 2 * D:] = dctx[m:].double().sum(0)
    # what the kernel gives there (exact zeros, the column sums in row `key`) is inside the bound: exp underflows
    assert sbr.worst_ratio(exact, want, sbr.U * errs) <= 1.0


def test_the_tenth_header_declares_functions_only_and_is_exported():
    with open(nat.SELF_ATTN_BACKWARD_HEADER_PATH) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert not structs and not enums and not consts
    assert sorted(funcs) == ["gfc_attention_self_backward", "gfc_attention_self_backward_workspace_bytes",
                             "gfc_lg_layer_pairs_keep_self", "gfc_lg_self_attn_backward",
                             "gfc_lg_self_attn_backward_workspace_bytes"]
    assert funcs == nat.SELF_ATTN_BACKWARD_FUNCTIONS
    others = [nat.FUNCTIONS, nat.VALIDATION_FUNCTIONS, nat.SPARSE_MAP_FUNCTIONS, nat.DENSE_WARP_FUNCTIONS,
              nat.CROSS_ATTENTION_FUNCTIONS, nat.LAYER_SCORES_FUNCTIONS, nat.HEAD_BACKWARD_FUNCTIONS,
              nat.FFN_BACKWARD_FUNCTIONS, nat.CROSS_ATTN_BACKWARD_FUNCTIONS]
    for o in others:
        assert not set(funcs) & set(o)
    lib = nat.lib()
    for name in funcs:
        assert getattr(lib, name) is not None  # the symbol is exported


def test_host_refusals_of_the_module():
    """`keep_self_block` without `keep_output_stage`, `self_block` without `cross_attention`, and a prediction without the
    kept self block are refused on the host, before any GPU work."""
    from glue_factory_colon_amd import lightglue

    lg = lightglue.LightGlue({"weights": "synthetic"}).eval()
    nl = int(lg.conf.n_layers)
    with pytest.raises(ValueError, match="keep_output_stage"):
        lg.forward_layers({}, keep_self_block=True)
    z = lambda *s: torch.zeros(s)  # noqa: E731
    pred = {"ref_descriptors0": z(1, nl, 3, D), "ref_descriptors1": z(1, nl, 2, D),
            "output_stage_rows0": z(1, 3, D), "output_stage_rows1": z(1, 2, D), "output_stage_context0": z(1, 3, D),
            "output_stage_context1": z(1, 2, D)}
    with pytest.raises(ValueError, match="cross_attention=True"):
        lg.layer_loss_backward(pred, {}, output_stage=True, self_block=True)
    with pytest.raises(ValueError, match="cross_attention=True"):
        lg.layer_loss_backward(pred, {}, self_block=True)
    with pytest.raises(ValueError, match="keep_self_block"):
        lg.layer_loss_backward(pred, {}, output_stage=True, cross_attention=True, self_block=True)


def test_workspace_formula_of_the_header():
    """The slot lists of include/gfc_amd_self_attn_backward.h, restated, equal the exports."""
    lib = nat.lib()
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731

    def parts(r):
        p = min(-(-r // 1024), 128)
        k = -(-(-(-r // p)) // 16) * 16
        return -(-r // k)

    for b, m, n in ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 1024, 1025), (32, 1024, 1024), (1, 2796201, 1)):
        r = b * (m + n)
        core = 2 * al(r * 4 * 4)
        assert lib.gfc_attention_self_backward_workspace_bytes(b, m, n, 4) == core, (b, m, n)
        want = 2 * al(r * 768 * 4) + al(parts(r) * 196608 * 4) + al(-(-r // 128) * 768 * 4) + al(core)
        assert lib.gfc_lg_self_attn_backward_workspace_bytes(b, m, n) == want, (b, m, n)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 2796202, 1), (2, 1398101, 1)):
        assert lib.gfc_lg_self_attn_backward_workspace_bytes(*bad) == 0, bad
        assert lib.gfc_attention_self_backward_workspace_bytes(*bad, 4) == 0, bad
    assert lib.gfc_attention_self_backward_workspace_bytes(1, 1, 1, 8) == 0


# ---- the reference's own autograd on the whole matcher (tests/golden/self_block_grad_*.npz) -----------------------------
import numpy as np  # noqa: E402

import cross_attn_grad_reference as car  # noqa: E402
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402
import output_stage_reference as osr  # noqa: E402
import test_cross_attn_grad_reference_host as cah  # noqa: E402  (stage64: the oracle's float64 last cross block, cached)

from oracle import lightglue as olg  # noqa: E402

L = lc.N_LAYERS
GOLDEN = cah.GOLDEN
GAMMAS = {"05": 0.5, "1": 1.0}
VECTOR_KEYS = {"bqkv": "dbqkv", "bout": "dbout", "b0": "db0", "gamma_": "dgamma", "beta": "dbeta", "b3": "db3"}
WEIGHT_KEYS = {"wqkv": "dWqkv", "wout": "dWout", "w0": "dW0", "w3": "dW3"}
_BLOCKS = {}


def rows_of(a, b):
    return torch.cat([a.reshape(-1, D), b.reshape(-1, D)], 0)


def block64(name, gamma):
    """The last self block of the whole matcher on case `name` in float64, from the oracle: what sbr.block_backward takes
    (the rows of layer L - 2, the tables, the self context by the closed form's own forward -- held to the oracle's block
    output here --, the complete gradient at the block's output from the cross block's closed form, head L - 2's direct
    gradient and its error sum, the parameters), and the shape."""
    if (name, gamma) in _BLOCKS:
        return _BLOCKS[name, gamma]
    case, labels, xs0, xs1, shape, x_mid, ctx_c, og, _, _, pc = cah.stage64(name, gamma)
    sd = cah._CACHE["sd"]
    dy = car.backward(x_mid, ctx_c, og["dctx"], og["dx_in"], pc, *shape)[0]["dx"]
    x = rows_of(xs0[L - 2], xs1[L - 2])
    tabs = [olg.positional_encoding(sd["posenc.Wr.weight"], olg.normalize_keypoints(case[k].double(), case["size"].double()))
            for k in ("keypoints0", "keypoints1")]
    cos, sin = (torch.cat([tabs[0][i].reshape(-1, sbr.HD), tabs[1][i].reshape(-1, sbr.HD)], 0) for i in (0, 1))
    p, wqkv, bqkv = sbr.stage_params(sd, L - 1)
    ctx = sbr.attention_forward(sbr.qkv_forward(x, cos, sin, wqkv, bqkv)[0], *shape)
    assert float((osr.forward(x, ctx, p) - x_mid).abs().max()) <= 1e-12 * float(x_mid.abs().max())  # the oracle's block
    g, sums, c = hg.model_grads(xs0, xs1, sd, labels, gamma=gamma, descriptor_grads=True)
    k0, k1 = "grad_ref_descriptors0", "grad_ref_descriptors1"
    head = rows_of(g[k0][:, L - 2], g[k1][:, L - 2])
    head_sum = rows_of(sums[k0][:, L - 2], sums[k1][:, L - 2])
    _BLOCKS[name, gamma] = (x, cos, sin, ctx, dy, head, head_sum, hg.head_c(*shape)["dx"], p, wqkv, bqkv, shape)
    return _BLOCKS[name, gamma]


def in_state_dict_order(d):
    return {k: sbr.to_state_dict(v) if k in ("dWqkv", "dbqkv") else v for k, v in d.items()}


def fixture_ratios(z, suffix, got, tol, shape):
    """{output: the worst |got - stored| / tol} over every array of one run (suffix "" or "_f32") of a fixture; `got`
    and `tol` in state-dict order."""
    t = lambda k: torch.from_numpy(z[k + suffix]).double()  # noqa: E731
    out = {o: sbr.worst_ratio(t(k), got[o].reshape(t(k).shape), tol[o].reshape(t(k).shape)) for k, o in VECTOR_KEYS.items()}
    for k, o in WEIGHT_KEYS.items():
        rows, cols = torch.from_numpy(z[k + "_pick_rows"]), torch.from_numpy(z[k + "_pick_cols"])
        u, v = torch.from_numpy(z[k + "_u"]), torch.from_numpy(z[k + "_v"])
        g = got[o]
        out[o] = max(sbr.worst_ratio(t(k + "_rows"), g[rows], tol[o][rows]),
                     sbr.worst_ratio(t(k + "_cols"), g[:, cols], tol[o][:, cols]),
                     float((u @ g @ v - float(z[k + "_bilinear" + suffix])).abs() / (u.abs() @ tol[o] @ v.abs())),
                     float(((g ** 2).sum() - float(z[k + "_sumsq" + suffix])).abs() / (2 * g.abs() * tol[o]).sum()))
    b, m, _ = shape
    r0, r1 = torch.from_numpy(z["rows0"]), torch.from_numpy(z["rows1"]) + b * m
    out["layer_input"] = max(sbr.worst_ratio(t("dx0"), got["layer_input"][r0], tol["layer_input"][r0]),
                             sbr.worst_ratio(t("dx1"), got["layer_input"][r1], tol["layer_input"][r1]))
    return out


@pytest.mark.parametrize("tag", list(GAMMAS))
@pytest.mark.parametrize("name", ["a", "b"])
def test_closed_form_against_the_references_autograd(name, tag):
    """The closed form on the oracle's float64 block equals the REFERENCE's float64 autograd (pre-hook on the last
    `self_attn`, `retain_grad`) within 1e-10 of each element's error sum -- the ten tensors and the kept inputs' gradient,
    which is `layer_input` -- and the reference's own float32 run stays inside every bound, with the trunk's float32
    error (head_grad_reference.trunk_c) and the error sums of the earlier stages carried in.  That second bound is loose
    (the carried error of dy is larger than dy); the float64 comparison and the same-bits comparisons on the GPU are the
    sharp ones."""
    gamma = GAMMAS[tag]
    x, cos, sin, ctx, dy, head, head_sum, head_c, p, wqkv, bqkv, shape = block64(name, gamma)
    z = np.load(os.path.join(GOLDEN, f"self_block_grad_{name}_gamma{tag}.npz"))
    assert float(z["gamma"]) == gamma
    assert torch.equal(lc.input_checksum(lc.make_case(name, int(z["seed"]))), torch.from_numpy(z["input_checksum"]))
    want, tol = sbr.block_backward(x, cos, sin, ctx, dy, head, p, wqkv, bqkv, *shape, head_err=head_c * head_sum)
    want, tol = in_state_dict_order(want), in_state_dict_order(tol)
    tiny = {k: 1e-10 / sbr.U * v for k, v in tol.items()}
    f64 = fixture_ratios(z, "", want, tiny, shape)
    print(f"case {name} gamma {gamma}: float64 run, fraction of 1e-10 error sum: "
          + ", ".join(f"{k} {v:.2e}" for k, v in f64.items()))
    assert max(f64.values()) <= 1.0, f64
    trunk = hg.trunk_c(L)
    _, _, _, _, _, x_mid, ctx_c, og, oe, _, pc = cah.stage64(name, gamma, in_err=trunk + hg.head_c(*shape)["dx"])
    _, errs_in = car.backward(x_mid, ctx_c, og["dctx"], og["dx_in"], pc, *shape,
                              err={"x": trunk * x_mid.abs(), "ctx": trunk * ctx_c.abs(), "dctx": oe["dctx"],
                                   "dx_in": oe["dx_in"]})
    _, tol32 = sbr.block_backward(x, cos, sin, ctx, dy, head, p, wqkv, bqkv, *shape, erf_abs=0.0, in_err=trunk,
                                  dy_err=errs_in["dx"], head_err=(head_c + trunk) * head_sum)
    f32 = fixture_ratios(z, "_f32", want, in_state_dict_order(tol32), shape)
    print(f"case {name} gamma {gamma}: float32 run, fraction of the bound used: "
          + ", ".join(f"{k} {v:.2e}" for k, v in f32.items()))
    assert max(f32.values()) <= 1.0, f32


def test_the_head_term_belongs_to_the_layer_input_rows():
    """Head L - 2's direct gradient dropped from `grad_layer_input_rows` misses the bound.  The rule for a wrong variant is
    100 x; this one misses by 32.7 x and is listed with its factor (head L - 2's direct gradient is the smaller part of
    the complete gradient there, and the bound carries the whole chain's error sums)."""
    x, cos, sin, ctx, dy, head, head_sum, head_c, p, wqkv, bqkv, shape = block64("a", 1.0)
    want, tol = sbr.block_backward(x, cos, sin, ctx, dy, head, p, wqkv, bqkv, *shape, head_err=head_c * head_sum)
    assert set(want) == set(tol) == set(sbr.BLOCK_OUTPUTS)
    for variant in sbr.BLOCK_VARIANTS:
        wrong, _ = sbr.block_backward(x, cos, sin, ctx, dy, head, p, wqkv, bqkv, *shape, variant=variant)
        ratio = sbr.worst_ratio(wrong["layer_input"], want["layer_input"], tol["layer_input"])
        print(f"{variant}: misses by layer_input {ratio:.3g}")
        assert ratio >= 30.0
        assert all(torch.equal(wrong[k], want[k]) for k in want if k != "layer_input")


def descent_ratio(name, eps):
    """(f(theta - eps grad) - f(theta)) / (-eps |grad|^2), f = mean(total - confidence), for the 22 tensors of the last
    layer, float64, loss.gamma 1."""
    case, labels, xs0, xs1, shape, x_mid, ctx_c, og, _, p_os, pc = cah.stage64(name, 1.0)
    x, cos, sin, ctx, dy, head, _, _, p, wqkv, bqkv, _ = block64(name, 1.0)
    sd = cah._CACHE["sd"]
    b, m, n = shape
    cross, _ = car.backward(x_mid, ctx_c, og["dctx"], og["dx_in"], pc, *shape)
    mine, _ = sbr.block_backward(x, cos, sin, ctx, dy, head, p, wqkv, bqkv, *shape)
    before = cah.smooth_total(xs0, xs1, sd, labels).mean()
    names = {"Wout": "dWout", "bout": "dbout", "W0": "dW0", "b0": "db0", "gamma": "dgamma", "beta": "dbeta", "W3": "dW3",
             "b3": "db3"}
    p2 = {k: v - eps * mine[names[k]] for k, v in p.items()}
    ctx2 = sbr.attention_forward(sbr.qkv_forward(x, cos, sin, wqkv - eps * mine["dWqkv"], bqkv - eps * mine["dbqkv"])[0],
                                 *shape)
    mid2 = osr.forward(x, ctx2, p2)
    pc2 = {k: v - eps * cross[cah.CA_GRAD[k]] for k, v in pc.items()}
    cctx2 = car.attention_forward(mid2 @ pc2["Wqk"].t() + pc2["bqk"], mid2 @ pc2["Wv"].t() + pc2["bv"], *shape)
    y = osr.forward(mid2, cctx2, {k: v - eps * og[cah.OS_GRAD[k]] for k, v in p_os.items()})
    after = cah.smooth_total(xs0[:-1] + [y[:b * m].reshape(b, m, 256)], xs1[:-1] + [y[b * m:].reshape(b, n, 256)], sd,
                             labels).mean()
    sq = (sum(float((og[g] ** 2).sum()) for g in cah.OS_GRAD.values())
          + sum(float((cross[g] ** 2).sum()) for g in cah.CA_GRAD.values())
          + sum(float((mine[g] ** 2).sum()) for g in sbr.BLOCK_OUTPUTS[:10]))
    return float(after - before) / (-eps * sq), float(before), float(after), sq


@pytest.mark.parametrize("name", ["a", "b"])
def test_descent_along_the_gradient(name):
    """An SGD step of eps on the 22 tensors of the last layer lowers `total - confidence` by eps |grad|^2 to first order:
    the ratio lies in [0.95, 1.05] at sbr.DESCENT_EPS, its distance from 1 halves with the step, and it is the recorded
    figure the GPU test compares its own ratio with."""
    eps = sbr.DESCENT_EPS
    ratio, before, after, sq = descent_ratio(name, eps)
    half = descent_ratio(name, eps / 2)[0]
    print(f"case {name}: descent ratio {ratio:.4f} at eps {eps} ({half:.4f} at eps / 2): total {before:.6f} -> "
          f"{after:.6f}, |grad|^2 {sq:.4e}")
    assert 0.95 <= ratio <= 1.05
    assert abs((1 - ratio) / (1 - half) - 2.0) <= 0.2
    assert abs(ratio - sbr.DESCENT_RATIO[name]) <= 5e-4
    assert abs(after - before) >= 1e-4 * abs(before)  # large enough to be seen in fp32 on the GPU
