"""The float64 closed form of the output stage's backward (tests/output_stage_reference.py) against autograd, its bounds
against a float32 evaluation, the reference's own autograd (tests/golden/output_stage_*.npz, float64 and float32 run) on
the output stage of the whole matcher formed on the CPU by the oracle, the descent along the gradient, the wrong variants
against the bounds, and the eighth header.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402
import layer_loss_reference as lr  # noqa: E402
import output_stage_reference as osr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import weights  # noqa: E402
from oracle import lightglue as olg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_OF = {"dWout": "Wout", "dbout": "bout", "dW0": "W0", "db0": "b0", "dgamma": "gamma", "dbeta": "beta", "dW3": "W3",
            "db3": "b3"}
R = 150  # a 128-row chunk and a tail
GOLDEN = os.path.join(ROOT, "tests", "golden")
L = lc.N_LAYERS
GAMMAS = {"05": 0.5, "1": 1.0}
WEIGHT_KEYS = {"wout": "dWout", "w0": "dW0", "w3": "dW3"}
VECTOR_KEYS = {"bout": "dbout", "b0": "db0", "gamma_": "dgamma", "beta": "dbeta", "b3": "db3"}
_CACHE = {}


def stage64(name, gamma):
    """(case, labels, xs0, xs1, x, ctx, dy, p) of the whole matcher on case `name` in float64: every layer's descriptors
    and the last cross block's rows and context from the oracle, dy = head L - 1's direct gradient from the closed form
    of tests/head_grad_reference.py (which its own host test holds to the reference), p the eight tensors."""
    if "sd" not in _CACHE:
        _CACHE["sd"] = {k: v.double() for k, v in weights.lightglue_state_dict(0).items()}
    sd = _CACHE["sd"]
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"output_stage_{name}_gamma1.npz"))
        case = lc.make_case(name, int(z["seed"]))
        assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"]))
        _CACHE[name] = (case,) + osr.stage_inputs(olg, sd, case, L)
    case, xs0, xs1, x, ctx = _CACHE[name]
    labels = {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"],
              "gt_assignment": case["gt_assignment"]}
    g, _, _ = hg.model_grads(xs0, xs1, sd, labels, gamma=gamma, descriptor_grads=True)
    dy = torch.cat([g["grad_ref_descriptors0"][:, L - 1].reshape(-1, 256),
                    g["grad_ref_descriptors1"][:, L - 1].reshape(-1, 256)], 0)
    return case, labels, xs0, xs1, x, ctx, dy, osr.stage_params(sd, L - 1)


def fixture_ratios(z, suffix, got, tol):
    """{output: the worst |got - stored| / tol} over every array of one run (suffix "" or "_f32") of a fixture."""
    t = lambda k: torch.from_numpy(z[k + suffix]).double()  # noqa: E731
    out = {o: osr.worst_ratio(got[o], t(k), tol[o]) for k, o in VECTOR_KEYS.items()}
    for k, o in WEIGHT_KEYS.items():
        rows, cols = torch.from_numpy(z[k + "_pick_rows"]), torch.from_numpy(z[k + "_pick_cols"])
        u, v = torch.from_numpy(z[k + "_u"]), torch.from_numpy(z[k + "_v"])
        g = got[o]
        out[o] = max(osr.worst_ratio(g[rows], t(k + "_rows"), tol[o][rows]),
                     osr.worst_ratio(g[:, cols], t(k + "_cols"), tol[o][:, cols]),
                     float((u @ g @ v - float(z[k + "_bilinear" + suffix])).abs() / (u.abs() @ tol[o] @ v.abs())),
                     float(((g ** 2).sum() - float(z[k + "_sumsq" + suffix])).abs() / (2 * g.abs() * tol[o]).sum()))
    return out


@pytest.mark.parametrize("tag", list(GAMMAS))
@pytest.mark.parametrize("name", ["a", "b"])
def test_closed_form_against_the_references_autograd(name, tag):
    """The closed form on the oracle's float64 stage equals the REFERENCE's float64 autograd within 1e-10 of each
    element's error sum, and the reference's own float32 run stays inside every bound: its rows, context and head
    gradient come from a float32 evaluation of the trunk and the head, whose error (head_grad_reference.trunk_c and
    head_c, dx) arrives as an input error."""
    case, _, _, _, x, ctx, dy, p = stage64(name, GAMMAS[tag])
    z = np.load(os.path.join(GOLDEN, f"output_stage_{name}_gamma{tag}.npz"))
    assert float(z["gamma"]) == GAMMAS[tag]
    want, errs, erfs = osr.backward(x, ctx, dy, p)
    b, m, n = case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1]
    r0, r1 = torch.from_numpy(z["rows0"]), torch.from_numpy(z["rows1"]) + b * m
    tiny = {k: 1e-10 * v for k, v in errs.items()}
    f64 = fixture_ratios(z, "", want, tiny)
    f64["dctx"] = max(osr.worst_ratio(want["dctx"][r0], torch.from_numpy(z["dctx0"]), tiny["dctx"][r0]),
                      osr.worst_ratio(want["dctx"][r1], torch.from_numpy(z["dctx1"]), tiny["dctx"][r1]))
    print(f"case {name} gamma {GAMMAS[tag]}: float64 run, fraction of 1e-10 error sum: "
          + ", ".join(f"{k} {v:.2e}" for k, v in f64.items()))
    assert max(f64.values()) <= 1.0, f64
    _, errs_in, erfs_in = osr.backward(x, ctx, dy, p, in_err=hg.trunk_c(L) + hg.head_c(b, m, n)["dx"])
    tol = osr.bounds(errs_in, erfs_in, erf_abs=0.0)  # torch's erf
    f32 = fixture_ratios(z, "_f32", want, tol)
    f32["dctx"] = max(osr.worst_ratio(want["dctx"][r0], torch.from_numpy(z["dctx0_f32"]).double(), tol["dctx"][r0]),
                      osr.worst_ratio(want["dctx"][r1], torch.from_numpy(z["dctx1_f32"]).double(), tol["dctx"][r1]))
    print(f"case {name} gamma {GAMMAS[tag]}: float32 run, fraction of the bound used: "
          + ", ".join(f"{k} {v:.2e}" for k, v in f32.items()))
    assert max(f32.values()) <= 1.0, f32


def smooth_total(xs0, xs1, sd, labels):
    """`total - confidence` [B] at loss.gamma 1: the part of the training loss that the eight tensors move smoothly.
    The confidence term reads other layers' descriptors and depends on the last layer only through its targets (the
    arg-max agreement, lightglue.py:82-95), which carry no gradient and change by jumps."""
    las = [hg.head_forward(xs0[i], xs1[i], *hg.head_params(sd, i)) for i in range(L)]
    lo0 = [xs0[i] @ hg.token_params(sd, i)[0] + hg.token_params(sd, i)[1] for i in range(L - 1)]
    lo1 = [xs1[i] @ hg.token_params(sd, i)[0] + hg.token_params(sd, i)[1] for i in range(L - 1)]
    losses, _, _ = lr.layer_loss(las, lo0, lo1, labels, [0.5] * (L - 1), gamma=1.0, balancing=0.5)
    return losses["total"] - losses["confidence"]


def descent_ratio(name, eps):
    """(f(theta - eps grad) - f(theta)) / (-eps |grad|^2), f = mean(total - confidence), for the eight tensors, float64,
    loss.gamma 1."""
    case, labels, xs0, xs1, x, ctx, dy, p = stage64(name, 1.0)
    sd = _CACHE["sd"]
    want, _, _ = osr.backward(x, ctx, dy, p)
    grad = {"Wout": "dWout", "bout": "dbout", "W0": "dW0", "b0": "db0", "gamma": "dgamma", "beta": "dbeta", "W3": "dW3",
            "b3": "db3"}
    before = smooth_total(xs0, xs1, sd, labels).mean()
    y = osr.forward(x, ctx, {k: v - eps * want[grad[k]] for k, v in p.items()})
    b, m, n = xs0[-1].shape[0], xs0[-1].shape[1], xs1[-1].shape[1]
    after = smooth_total(xs0[:-1] + [y[:b * m].reshape(b, m, 256)], xs1[:-1] + [y[b * m:].reshape(b, n, 256)], sd,
                         labels).mean()
    sq = sum(float((want[g] ** 2).sum()) for g in grad.values())
    return float(after - before) / (-eps * sq), float(before), float(after), sq


@pytest.mark.parametrize("name", ["a", "b"])
def test_descent_along_the_gradient(name):
    """An SGD step of eps on the eight tensors lowers `total - confidence` by eps |grad|^2 to first order: the ratio lies in [0.95,
    1.05] at osr.DESCENT_EPS, its distance from 1 halves with the step (the second-order term), and it is the recorded
    figure the GPU test compares its own ratio with.  (The heads' step of 0.05 is outside the stage's linear range.)"""
    eps = osr.DESCENT_EPS
    ratio, before, after, sq = descent_ratio(name, eps)
    half = descent_ratio(name, eps / 2)[0]
    print(f"case {name}: descent ratio {ratio:.4f} at eps {eps} ({half:.4f} at eps / 2): total {before:.6f} -> "
          f"{after:.6f}, |grad|^2 {sq:.4e}")
    assert 0.95 <= ratio <= 1.05
    assert abs((1 - ratio) / (1 - half) - 2.0) <= 0.2
    assert abs(ratio - osr.DESCENT_RATIO[name]) <= 5e-4
    assert abs(after - before) >= 1e-4 * abs(before)  # large enough to be seen in fp32 on the GPU


def block(with_out, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = osr.random_params(g, with_out)
    x, ctx = torch.randn((R, 256), generator=g) / 16, torch.randn((R, 256), generator=g) / 16
    dy = torch.randn((R, 256), generator=g) * 1e-3
    return x, ctx, dy, p


def autograd(x, ctx, dy, p, dtype):
    """{output: gradient} of sum(y * dy) by torch's autograd on the block as the reference builds it (nn.Linear,
    nn.LayerNorm, nn.GELU, the concatenation and the residual); ctx is a leaf, so dx_in does not follow it."""
    leaf = lambda t: None if t is None else t.detach().to(dtype).requires_grad_()  # noqa: E731
    q = {k: leaf(v) for k, v in p.items()}
    xl, cl = leaf(x), leaf(ctx)
    (osr.forward(xl, cl, q) * dy.to(dtype)).sum().backward()
    out = {k: q[v].grad for k, v in PARAM_OF.items() if q[v] is not None}
    out["dx_in"], out["dctx"] = xl.grad, cl.grad
    return out


@pytest.mark.parametrize("with_out", [True, False])
def test_closed_form_equals_float64_autograd_and_bounds_hold_float32(with_out):
    x, ctx, dy, p = block(with_out)
    want, sums, erfs = osr.backward(x.double(), ctx.double(), dy.double(), osr.to64(p))
    ref = autograd(x, ctx, dy, p, torch.float64)
    assert set(want) == set(ref) == set(sums) == set(erfs)
    for k in want:
        assert float(((want[k] - ref[k]).abs() / sums[k].clamp(min=1e-300)).max()) <= 1e-10, k
    tol = osr.bounds(sums, erfs, erf_abs=0.0)  # torch's erf is exact to fp32 rounding
    f32 = autograd(x, ctx, dy, p, torch.float32)
    used = {k: osr.worst_ratio(f32[k], want[k], tol[k]) for k in want}
    print("float32 autograd, fraction of the bound used: " + ", ".join(f"{k} {v:.2e}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, used


# variant -> (the case it is aimed at, the outputs among which it must miss a bound, by at least this factor).  The cases:
# "plain" random data with Wout (the bound carries the fp32 error of h, about 1e-5 relative), "centred" / "offset" the
# exact conditioning cases with b0 = 0 / 4096 (h exact: the bound is the backward's own arithmetic).  Measured factors
# are printed; where one is below 100 it stands beside the entry.
AIMED = {
    "one_pass_var": ("offset", ("dW0", "db0", "dgamma", "dx_in", "dctx"), 100.0),
    "no_eps": ("offset", ("dW0", "db0", "dgamma", "dx_in", "dctx"), float("inf")),   # NaN on the constant rows
    "unbiased_var": ("centred", ("dgamma", "dW0", "dW3"), 50.0),      # an error of 1e-3 relative: measured 71
    "no_n_term": ("centred", ("dW0", "db0", "dx_in", "dctx"), 100.0),
    "no_mean_term": ("centred", ("dW0", "db0", "dx_in", "dctx"), 100.0),
    # differs from the erf form by <= 5e-4 of g: 11 in the sums over rows, 60 in the rows themselves
    "tanh_gelu": ("centred", ("dbeta", "dgamma", "dx_in", "dctx"), 40.0),
    "phi_only": ("plain", ("dbeta", "dgamma", "dW0"), 100.0),
    "no_residual": ("centred", ("dx_in",), 100.0),
    "folded_w0": ("plain", ("dW0",), 100.0),
    "dwout_transposed": ("plain", ("dWout",), 30.0),        # measured 52
    "dbout_from_dh": ("plain", ("dbout",), 20.0),             # measured 31
    "halves_swapped": ("plain", ("dW0", "dx_in", "dctx"), 100.0),
}


def test_every_variant_is_listed():
    assert set(AIMED) == set(osr.VARIANTS)


@pytest.mark.parametrize("variant", osr.VARIANTS)
def test_wrong_variants_miss_a_bound(variant):
    case, outputs, factor = AIMED[variant]
    if case == "plain":
        x, ctx, dy, p = block(True, seed=1)
        exact, rows, with_out = False, R, True
    else:
        x, ctx, dy, p = osr.conditioning_case(4096 if case == "offset" else 0)
        exact, rows, with_out = True, osr.COND_R, False
    want, sums, erfs = osr.backward(x.double(), ctx.double(), dy.double(), osr.to64(p), exact_h=exact)
    tol = osr.bounds(sums, erfs)
    wrong, _, _ = osr.backward(x.double(), ctx.double(), dy.double(), osr.to64(p), variant=variant, exact_h=exact)
    ratios = {k: osr.worst_ratio(wrong[k], want[k], tol[k]) for k in outputs}
    print(f"{variant}: misses by " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) >= factor, ratios


def test_conditioning_case_is_what_it_says():
    for offset in (4096, 0):
        x, ctx, dy, p = osr.conditioning_case(offset)
        want, sums, erfs = osr.backward(x.double(), ctx.double(), dy.double(), osr.to64(p), exact_h=True)
        assert all(bool(torch.isfinite(v).all()) for v in want.values())
        # u = -1e4: the derivative is exactly 0; gamma = 0: nothing reaches dh from those columns
        assert bool((want["dbeta"][osr.COL_NEG] == 0).all()) and bool((want["dgamma"][osr.COL_NEG] == 0).all())
        da = dy.double() @ p["W3"].double()
        assert torch.equal(want["dbeta"][osr.COL_POS], da.sum(0)[osr.COL_POS])  # exactly 1


def test_the_eighth_header_declares_functions_only():
    with open(os.path.join(ROOT, "include", "gfc_amd_ffn_backward.h")) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert not structs and not enums and not consts
    assert sorted(funcs) == ["gfc_lg_ffn_backward", "gfc_lg_ffn_backward_workspace_bytes", "gfc_lg_layer_pairs_keep"]
    assert funcs == nat.FFN_BACKWARD_FUNCTIONS
    others = [nat.FUNCTIONS, nat.VALIDATION_FUNCTIONS, nat.SPARSE_MAP_FUNCTIONS, nat.DENSE_WARP_FUNCTIONS,
              nat.CROSS_ATTENTION_FUNCTIONS, nat.LAYER_SCORES_FUNCTIONS, nat.HEAD_BACKWARD_FUNCTIONS]
    for o in others:
        assert not set(funcs) & set(o)
    keep, pairs = funcs["gfc_lg_layer_pairs_keep"][1], nat.LAYER_SCORES_FUNCTIONS["gfc_lg_layer_pairs"][1]
    assert [q for q in keep if q[0] not in ("x_mid", "ctx")] == pairs  # gfc_lg_layer_pairs with two more outputs


def test_workspace_formula_of_the_header():
    """The slot list of include/gfc_amd_ffn_backward.h, restated, equals the export."""
    lib = nat.lib()
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731

    def parts(r):
        p = min(-(-r // 1024), 128)
        k = -(-(-(-r // p)) // 16) * 16
        return -(-r // k)

    for r in (1, 2, 127, 128, 129, 1024, 1025, 2049, 128 * 1024, 128 * 1024 + 17, 8388607):
        chunks = -(-r // 128)
        want = (2 * al(r * 256 * 4) + 2 * al(r * 512 * 4) + al(parts(r) * 262144 * 4) + al(chunks * 520 * 4)
                + al(chunks * 1536 * 4))
        assert lib.gfc_lg_ffn_backward_workspace_bytes(r) == want, r
    assert lib.gfc_lg_ffn_backward_workspace_bytes(0) == 0 and lib.gfc_lg_ffn_backward_workspace_bytes(8388608) == 0
    assert parts(128 * 1024 + 17) == 127  # past the cap the parts grow to 1040 rows
