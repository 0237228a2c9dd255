"""The float64 closed form of the cross-attention backward (tests/cross_attn_grad_reference.py) against autograd, its
bounds against a float32 evaluation, the reference's own autograd (tests/golden/cross_attn_grad_*.npz, float64 and
float32 run) on the last cross block of the whole matcher formed on the CPU by the oracle, the descent along the gradient
of the twelve tensors, the wrong variants against the bounds, the conditioning cases, and the ninth header.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_attn_grad_reference as car  # noqa: E402
import head_grad_reference as hg  # noqa: E402
import layer_loss_cases as lc  # noqa: E402
import layer_loss_reference as lr  # noqa: E402
import output_stage_reference as osr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402
from glue_factory_colon_amd import weights  # noqa: E402
from oracle import lightglue as olg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
L = lc.N_LAYERS
GAMMAS = {"05": 0.5, "1": 1.0}
WEIGHT_KEYS = {"wqk": "dWqk", "wv": "dWv"}
VECTOR_KEYS = {"bqk": "dbqk", "bv": "dbv"}
_CACHE = {}


def stage64(name, gamma, in_err=0.0):
    """The last cross block of the whole matcher on case `name` in float64: (case, labels, xs0, xs1, shape, x, ctx, the
    output stage's gradients and error sums from tests/output_stage_reference.py (whose host test holds them to the
    reference; in_err as there), its eight tensors, and to_qk / to_v)."""
    if "sd" not in _CACHE:
        _CACHE["sd"] = {k: v.double() for k, v in weights.lightglue_state_dict(0).items()}
    sd = _CACHE["sd"]
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"cross_attn_grad_{name}_gamma1.npz"))
        case = lc.make_case(name, int(z["seed"]))
        assert torch.equal(lc.input_checksum(case), torch.from_numpy(z["input_checksum"]))
        _CACHE[name] = (case,) + osr.stage_inputs(olg, sd, case, L)
    case, xs0, xs1, x, ctx = _CACHE[name]
    labels = {"gt_matches0": case["gt_matches0"], "gt_matches1": case["gt_matches1"],
              "gt_assignment": case["gt_assignment"]}
    g, _, _ = hg.model_grads(xs0, xs1, sd, labels, gamma=gamma, descriptor_grads=True)
    dy = torch.cat([g["grad_ref_descriptors0"][:, L - 1].reshape(-1, 256),
                    g["grad_ref_descriptors1"][:, L - 1].reshape(-1, 256)], 0)
    shape = (case["keypoints0"].shape[0], case["keypoints0"].shape[1], case["keypoints1"].shape[1])
    p_os = osr.stage_params(sd, L - 1)
    os_grads, os_errs, _ = osr.backward(x, ctx, dy, p_os, in_err=in_err)
    return case, labels, xs0, xs1, shape, x, ctx, os_grads, os_errs, p_os, car.stage_params(sd, L - 1)


def fixture_ratios(z, suffix, got, tol):
    """{output: the worst |got - stored| / tol} over every array of one run (suffix "" or "_f32") of a fixture."""
    t = lambda k: torch.from_numpy(z[k + suffix]).double()  # noqa: E731
    out = {o: car.worst_ratio(got[o], t(k), tol[o]) for k, o in VECTOR_KEYS.items()}
    for k, o in WEIGHT_KEYS.items():
        rows, cols = torch.from_numpy(z[k + "_pick_rows"]), torch.from_numpy(z[k + "_pick_cols"])
        u, v = torch.from_numpy(z[k + "_u"]), torch.from_numpy(z[k + "_v"])
        g = got[o]
        out[o] = max(car.worst_ratio(g[rows], t(k + "_rows"), tol[o][rows]),
                     car.worst_ratio(g[:, cols], t(k + "_cols"), tol[o][:, cols]),
                     float((u @ g @ v - float(z[k + "_bilinear" + suffix])).abs() / (u.abs() @ tol[o] @ v.abs())),
                     float(((g ** 2).sum() - float(z[k + "_sumsq" + suffix])).abs() / (2 * g.abs() * tol[o]).sum()))
    return out


def row_ratios(z, suffix, want, tol, shape, dx_in):
    """The stored rows of the gradient at the block's inputs against `dx`, and -- the closed form's dx_in taken off them
    -- against the attention's share `dx_att` on its own (about 200 times smaller than dx, which is blind to it)."""
    b, m, _ = shape
    out = {"dx": 0.0, "dx_att": 0.0}
    for rows, key in ((torch.from_numpy(z["rows0"]), "dx0"), (torch.from_numpy(z["rows1"]) + b * m, "dx1")):
        stored = torch.from_numpy(z[key + suffix]).double()
        out["dx"] = max(out["dx"], car.worst_ratio(stored, want["dx"][rows], tol["dx"][rows]))
        out["dx_att"] = max(out["dx_att"], car.worst_ratio(stored - dx_in[rows], want["dx_att"][rows], tol["dx"][rows]))
    return out


@pytest.mark.parametrize("tag", list(GAMMAS))
@pytest.mark.parametrize("name", ["a", "b"])
def test_closed_form_against_the_references_autograd(name, tag):
    """The closed form on the oracle's float64 stage equals the REFERENCE's float64 autograd within 1e-10 of each
    element's error sum, and the reference's own float32 run stays inside every bound: its rows and context come from a
    float32 evaluation of the trunk (head_grad_reference.trunk_c) and its dctx and dx_in from a float32 output stage
    (the error sums of tests/output_stage_reference.py), which arrive as input errors.  That second bound is a sanity
    check only: the output stage's carried error sum of dctx is larger than dctx itself, so the float32 run uses 1e-9 to
    1e-6 of it; the float64 comparison above and the same-bits comparisons on the GPU are the sharp ones."""
    _, _, _, _, shape, x, ctx, og, _, _, pc = stage64(name, GAMMAS[tag])
    z = np.load(os.path.join(GOLDEN, f"cross_attn_grad_{name}_gamma{tag}.npz"))
    assert float(z["gamma"]) == GAMMAS[tag]
    want, errs = car.backward(x, ctx, og["dctx"], og["dx_in"], pc, *shape)
    tiny = {k: 1e-10 * v for k, v in errs.items()}
    f64 = {**fixture_ratios(z, "", want, tiny), **row_ratios(z, "", want, tiny, shape, og["dx_in"])}
    print(f"case {name} gamma {GAMMAS[tag]}: float64 run, fraction of 1e-10 error sum: "
          + ", ".join(f"{k} {v:.2e}" for k, v in f64.items()))
    assert max(f64.values()) <= 1.0, f64
    # the attention's share is the small part: a test on the summed dx alone would not see it
    assert float(want["dx_att"].abs().max()) < 0.02 * float(want["dx"].abs().max())
    assert float(want["dWqk"].abs().max()) < 0.1 * float(want["dWv"].abs().max())  # P (dP - D) cancels
    trunk = hg.trunk_c(L)
    _, _, _, _, _, _, _, _, oe, _, _ = stage64(name, GAMMAS[tag], in_err=trunk + hg.head_c(*shape)["dx"])
    _, errs_in = car.backward(x, ctx, og["dctx"], og["dx_in"], pc, *shape,
                              err={"x": trunk * x.abs(), "ctx": trunk * ctx.abs(), "dctx": oe["dctx"], "dx_in": oe["dx_in"]})
    tol = car.bounds(errs_in)
    f32 = {**fixture_ratios(z, "_f32", want, tol), **row_ratios(z, "_f32", want, tol, shape, og["dx_in"])}
    print(f"case {name} gamma {GAMMAS[tag]}: float32 run, fraction of the bound used: "
          + ", ".join(f"{k} {v:.2e}" for k, v in f32.items()))
    assert max(f32.values()) <= 1.0, f32


def bare_block(shape, seed=0):
    b, m, n = shape
    g = torch.Generator().manual_seed(seed)
    rows = b * (m + n)
    p = car.random_params(g)
    x = torch.randn((rows, 256), generator=g)
    dctx = torch.randn((rows, 256), generator=g) * 1e-3
    dx_in = torch.randn((rows, 256), generator=g) * 0.2
    return x, dctx, dx_in, p


def autograd(x, dctx, dx_in, p, shape, dtype):
    """({output: gradient}, ctx) of sum(ctx * dctx) by torch's autograd on to_qk, to_v and the attention as the
    reference builds them (lightglue.py:196-218), plus dx_in at the rows."""
    leaf = lambda t: t.detach().to(dtype).requires_grad_()  # noqa: E731
    q = {k: leaf(v) for k, v in p.items()}
    xl = leaf(x)
    qk, v = xl @ q["Wqk"].t() + q["bqk"], xl @ q["Wv"].t() + q["bv"]
    b, m, n = shape
    q0, q1 = car.split_heads(qk, b, m, n)
    v0, v1 = car.split_heads(v, b, m, n)
    q0, q1 = q0 * car.SCALE ** 0.5, q1 * car.SCALE ** 0.5
    sim = torch.einsum("bhid, bhjd -> bhij", q0, q1)
    attn01 = torch.softmax(sim, -1)
    attn10 = torch.softmax(sim.transpose(-2, -1).contiguous(), -1)
    m0 = torch.einsum("bhij, bhjd -> bhid", attn01, v1)
    m1 = torch.einsum("bhji, bhjd -> bhid", attn10.transpose(-2, -1), v0)
    ctx = car.merge_heads(m0, m1)
    (ctx * dctx.to(dtype)).sum().backward()
    out = {"dWqk": q["Wqk"].grad, "dbqk": q["bqk"].grad, "dWv": q["Wv"].grad, "dbv": q["bv"].grad, "dx_att": xl.grad,
           "dx": dx_in.to(dtype) + xl.grad}
    return out, ctx.detach()


@pytest.mark.parametrize("shape", [(2, 37, 50), (1, 130, 65)], ids=lambda s: "x".join(map(str, s)))
def test_closed_form_equals_float64_autograd_and_bounds_hold_float32(shape):
    x, dctx, dx_in, p = bare_block(shape)
    ref, ctx = autograd(x, dctx, dx_in, p, shape, torch.float64)
    want, sums = car.backward(x.double(), ctx, dctx.double(), dx_in.double(), car.to64(p), *shape)
    assert set(want) == set(ref) == set(sums) == set(car.OUTPUTS)
    for k in want:
        assert float(((want[k] - ref[k]).abs() / sums[k].clamp(min=1e-300)).max()) <= 1e-10, k
    f32, ctx32 = autograd(x, dctx, dx_in, p, shape, torch.float32)
    want32, sums32 = car.backward(x.double(), ctx32.double(), dctx.double(), dx_in.double(), car.to64(p), *shape)
    tol = car.bounds(sums32)
    used = {k: car.worst_ratio(f32[k], want32[k], tol[k]) for k in want}
    print("float32 autograd, fraction of the bound used: " + ", ".join(f"{k} {v:.2e}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, used
    # the soft-max rows are not flat: a wrong soft-max can be told apart
    q0, q1 = car.split_heads(x.double() @ p["Wqk"].double().t() + p["bqk"].double(), *shape)
    prob = torch.softmax(car.SCALE * (q0 @ q1.transpose(-1, -2)), -1)
    assert float((prob.max(-1).values * shape[2]).median()) > 2.0


# variant -> (the outputs among which it must miss a bound on the last cross block of case "a" at loss.gamma 1, by at
# least this factor).  Measured factors are printed; the smallest stands beside its entry.
AIMED = {
    "col_softmax_along_rows": (("dWqk", "dWv", "dbv", "dx_att"), 100.0),   # dWqk 131, dWv 1270
    "scale_twice": (("dWqk", "dx_att"), 100.0),                            # dWqk 191
    "no_scale_dq": (("dWqk", "dx_att"), 1000.0),
    "no_D": (("dWqk", "dbqk", "dx_att"), 500.0),
    "D_from_dctx": (("dWqk", "dbqk", "dx_att"), 500.0),
    "dv_swapped": (("dWv", "dbv"), 1000.0),
    "one_direction": (("dWqk", "dx_att"), 50.0),                           # dWqk 103, dx_att 68
    "dwqk_transposed": (("dWqk",), 300.0),
    "dbqk_from_dv": (("dbqk",), 1000.0),
    "heads_merged": (("dWqk", "dWv", "dx_att"), 500.0),
    "dx_no_v": (("dx_att", "dx"), 100.0),
}


def test_every_variant_is_listed():
    assert set(AIMED) == set(car.VARIANTS)


@pytest.mark.parametrize("variant", car.VARIANTS)
def test_wrong_variants_miss_a_bound(variant):
    outputs, factor = AIMED[variant]
    _, _, _, _, shape, x, ctx, og, _, _, pc = stage64("a", 1.0)
    want, errs = car.backward(x, ctx, og["dctx"], og["dx_in"], pc, *shape)
    tol = car.bounds(errs)
    wrong, _ = car.backward(x, ctx, og["dctx"], og["dx_in"], pc, *shape, variant=variant)
    ratios = {k: car.worst_ratio(wrong[k], want[k], tol[k]) for k in outputs}
    print(f"{variant}: misses by " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert factor >= 10.0 and max(ratios.values()) >= factor, ratios


def test_conditioning_cases_are_what_they_say():
    qk, v, ctx, dctx, shape = car.identical_keys_case()
    m = shape[1]
    q0, q1 = car.split_heads(qk.double(), *shape)
    p01 = torch.softmax(car.SCALE * (q0 @ q1.transpose(-1, -2)), -1)
    assert float((p01 - 1.0 / 64).abs().max()) <= 1e-15
    assert float((ctx[:m].double() - v[m].double()).abs().max()) <= 1e-6  # every row of side 0 attends to the one v row
    want, _ = car.attention_backward(qk.double(), v.double(), ctx.double(), dctx.double(), *shape)
    assert float((want["dv"][m:] - want["dv"][m:m + 1]).abs().max()) <= 1e-18
    qk, v, ctx, dctx, shape, key = car.dominant_key_case()
    m = shape[1]
    assert torch.equal(ctx[:m], v[m + key].expand(m, 256))
    want, errs = car.attention_backward(qk.double(), v.double(), ctx.double(), dctx.double(), *shape)
    assert float(want["dqk"].abs().max()) < 1e-80 and float(want["dv"][:m].abs().max()) == 0.0
    assert torch.equal(want["dv"][m + key], dctx[:m].double().sum(0))
    # what the kernel gives there (exact zeros, the column sums in row `key`) is inside the bound: exp underflows
    exact = torch.zeros_like(want["dv"])
    exact[m + key] = dctx[:m].double().sum(0)
    tol = car.bounds(errs)
    assert car.worst_ratio(exact, want["dv"], tol["dv"]) <= 1.0
    assert car.worst_ratio(torch.zeros_like(want["dqk"]), want["dqk"], tol["dqk"]) <= 1.0


def smooth_total(xs0, xs1, sd, labels):
    """`total - confidence` [B] at loss.gamma 1 (tests/test_output_stage_reference_host.py: the part of the training
    loss that the last layer's tensors move smoothly)."""
    las = [hg.head_forward(xs0[i], xs1[i], *hg.head_params(sd, i)) for i in range(L)]
    lo0 = [xs0[i] @ hg.token_params(sd, i)[0] + hg.token_params(sd, i)[1] for i in range(L - 1)]
    lo1 = [xs1[i] @ hg.token_params(sd, i)[0] + hg.token_params(sd, i)[1] for i in range(L - 1)]
    losses, _, _ = lr.layer_loss(las, lo0, lo1, labels, [0.5] * (L - 1), gamma=1.0, balancing=0.5)
    return losses["total"] - losses["confidence"]


OS_GRAD = {"Wout": "dWout", "bout": "dbout", "W0": "dW0", "b0": "db0", "gamma": "dgamma", "beta": "dbeta", "W3": "dW3",
           "b3": "db3"}
CA_GRAD = {"Wqk": "dWqk", "bqk": "dbqk", "Wv": "dWv", "bv": "dbv"}


def descent_ratio(name, eps):
    """(f(theta - eps grad) - f(theta)) / (-eps |grad|^2), f = mean(total - confidence), for the twelve tensors of the
    last cross block, float64, loss.gamma 1."""
    _, labels, xs0, xs1, shape, x, ctx, og, _, p_os, pc = stage64(name, 1.0)
    sd = _CACHE["sd"]
    b, m, n = shape
    want, _ = car.backward(x, ctx, og["dctx"], og["dx_in"], pc, *shape)
    before = smooth_total(xs0, xs1, sd, labels).mean()
    pc2 = {k: v - eps * want[CA_GRAD[k]] for k, v in pc.items()}
    ctx2 = car.attention_forward(x @ pc2["Wqk"].t() + pc2["bqk"], x @ pc2["Wv"].t() + pc2["bv"], *shape)
    y = osr.forward(x, ctx2, {k: v - eps * og[OS_GRAD[k]] for k, v in p_os.items()})
    after = smooth_total(xs0[:-1] + [y[:b * m].reshape(b, m, 256)], xs1[:-1] + [y[b * m:].reshape(b, n, 256)], sd,
                         labels).mean()
    sq = sum(float((og[g] ** 2).sum()) for g in OS_GRAD.values()) + sum(float((want[g] ** 2).sum())
                                                                         for g in CA_GRAD.values())
    return float(after - before) / (-eps * sq), float(before), float(after), sq


@pytest.mark.parametrize("name", ["a", "b"])
def test_descent_along_the_gradient(name):
    """An SGD step of eps on the twelve tensors lowers `total - confidence` by eps |grad|^2 to first order: the ratio
    lies in [0.95, 1.05] at car.DESCENT_EPS, its distance from 1 halves with the step, and it is the recorded figure the
    GPU test compares its own ratio with."""
    eps = car.DESCENT_EPS
    ratio, before, after, sq = descent_ratio(name, eps)
    half = descent_ratio(name, eps / 2)[0]
    print(f"case {name}: descent ratio {ratio:.4f} at eps {eps} ({half:.4f} at eps / 2): total {before:.6f} -> "
          f"{after:.6f}, |grad|^2 {sq:.4e}")
    assert 0.95 <= ratio <= 1.05
    assert abs((1 - ratio) / (1 - half) - 2.0) <= 0.2
    assert abs(ratio - car.DESCENT_RATIO[name]) <= 5e-4
    assert abs(after - before) >= 1e-4 * abs(before)  # large enough to be seen in fp32 on the GPU


def test_the_forward_of_the_closed_form_is_the_oracles():
    """attention_forward on to_qk / to_v of the oracle's rows is the context the oracle hands to to_out."""
    _, _, _, _, shape, x, ctx, _, _, _, pc = stage64("a", 1.0)
    mine = car.attention_forward(x @ pc["Wqk"].t() + pc["bqk"], x @ pc["Wv"].t() + pc["bv"], *shape)
    assert float((mine - ctx).abs().max()) <= 1e-13 * float(ctx.abs().max())


def test_the_ninth_header_declares_functions_only_and_is_exported():
    with open(nat.CROSS_ATTN_BACKWARD_HEADER_PATH) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert not structs and not enums and not consts
    assert sorted(funcs) == ["gfc_attention_cross_backward", "gfc_attention_cross_backward_workspace_bytes",
                             "gfc_lg_cross_attn_backward", "gfc_lg_cross_attn_backward_workspace_bytes"]
    assert funcs == nat.CROSS_ATTN_BACKWARD_FUNCTIONS
    others = [nat.FUNCTIONS, nat.VALIDATION_FUNCTIONS, nat.SPARSE_MAP_FUNCTIONS, nat.DENSE_WARP_FUNCTIONS,
              nat.CROSS_ATTENTION_FUNCTIONS, nat.LAYER_SCORES_FUNCTIONS, nat.HEAD_BACKWARD_FUNCTIONS,
              nat.FFN_BACKWARD_FUNCTIONS]
    for o in others:
        assert not set(funcs) & set(o)
    lib = nat.lib()
    for name in funcs:
        assert getattr(lib, name) is not None  # the symbol is exported


def test_workspace_formula_of_the_header():
    """The slot lists of include/gfc_amd_cross_attn_backward.h, restated, equal the exports."""
    lib = nat.lib()
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731

    def parts(r):
        p = min(-(-r // 1024), 128)
        k = -(-(-(-r // p)) // 16) * 16
        return -(-r // k)

    for b, m, n in ((1, 1, 1), (2, 63, 64), (3, 130, 65), (1, 1024, 1025), (32, 1024, 1024), (1, 8388606, 1)):
        r = b * (m + n)
        core = 2 * al(r * 4 * 4)
        assert lib.gfc_attention_cross_backward_workspace_bytes(b, m, n, 4) == core, (b, m, n)
        want = 5 * al(r * 256 * 4) + al(parts(r) * 65536 * 4) + al(-(-r // 128) * 520 * 4) + al(core)
        assert lib.gfc_lg_cross_attn_backward_workspace_bytes(b, m, n) == want, (b, m, n)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 8388607, 1), (2, 4194304, 1)):
        assert lib.gfc_lg_cross_attn_backward_workspace_bytes(*bad) == 0, bad
        assert lib.gfc_attention_cross_backward_workspace_bytes(*bad, 4) == 0, bad
    assert lib.gfc_attention_cross_backward_workspace_bytes(1, 1, 1, 8) == 0
