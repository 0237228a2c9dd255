"""The conditioning cases (tests/conditioning_cases.py) can fail, and the data the suite used before cannot: proven here
on the CPU.

For every case: the quantity under test is exact (the builders assert fp32 == float64), the reference is finite, the fp32
emulation of the algorithm the kernel implements meets the case's bound, and every wrong variant aimed at the case misses
the bound by a factor of 100 or more (so that no bound is loose enough to hide the failure it exists for).  REJECTED_BY
names, for every variant, one case that rejects it.  The last two tests keep the findings that motivated the cases: on
the data of test_linear_layernorm_gelu_fused and test_attention_peaky_rows the wrong variants pass the suite's 2e-5."""
import types

import pytest
import torch
import torch.nn.functional as F

import conditioning_cases as C

MARGIN = 100.0

# variant -> the case (and launch) named as rejecting it; every aimed pair of C.*_AIMED is checked as well
REJECTED_BY = {
    "layernorm": {"one_pass_var": "offset", "no_eps": "const", "eps_1e-6": "tiny", "eps_outside_sqrt": "tiny"},
    "attention": {"no_max": ("wide", "single"), "no_rescale_o": ("ascending", "single"), "no_rescale_l": ("ascending", "pair"),
                  "skip_by_lane0": ("mixed", "single"), "merge_no_max": ("all_positive", "split8"),
                  "merge_w1": ("ascending", "split8"), "merge_no_empty_guard": ("equal", "split3")},
    "head": {"no_max": ("dust_min", "affine"), "max_over_64": ("dust_over", "affine"), "sum_over_64": ("dust_max", "plain")},
}


def test_every_variant_is_listed_and_aimed():
    assert set(REJECTED_BY["layernorm"]) == set(C.LN_VARIANTS)
    assert set(REJECTED_BY["attention"]) == set(C.ATT_VARIANTS)
    assert set(REJECTED_BY["head"]) == set(C.DH_VARIANTS)
    for v, case in REJECTED_BY["layernorm"].items():
        assert v in C.LN_CASES[case][1]
    for v, (case, run) in REJECTED_BY["attention"].items():
        assert run in C.ATT_AIMED[case][v]
    for v, (kind, mode) in REJECTED_BY["head"].items():
        assert mode in C.DH_AIMED[kind][v]
    assert all(C.LN_CASES[case][1] for case in C.LN_CASES) and all(C.ATT_AIMED[case] for case in C.ATT_CASES)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", list(C.LN_CASES))
def test_layernorm_case(case):
    launch, aimed = C.LN_CASES[case]
    c = C.ln_launch(launch)  # asserts exactness and the designed statistics
    assert torch.isfinite(c.h_ref).all() and torch.isfinite(c.y_ref).all()
    assert C.ln_ratio(case, C.emulate_layernorm(c)) <= 1.0
    assert C.ln_ratio(case, C.emulate_ffn(c), "y") <= 1.0
    for v in aimed:
        assert C.ln_ratio(case, C.emulate_layernorm(c, v)) >= MARGIN, v
        if case in C.LN_FFN_CONDITION_CASES:
            assert C.ln_ratio(case, C.emulate_ffn(c, v), "y") >= MARGIN, v
        else:  # rejected at the FFN output too, by the margin the docstring of the cases explains
            assert C.ln_ratio(case, C.emulate_ffn(c, v), "y") >= 10.0, v
    if case == "const":  # the closed form, and the variant's NaN
        rows = C.ln_rows("const")
        want = F.gelu(c.beta.double()).expand(len(rows), -1)
        assert float((c.h_ref[rows] - want).abs().max()) < 1e-15
        assert torch.equal(C.emulate_layernorm(c)[rows], F.gelu(c.beta).expand(len(rows), -1))
        assert torch.isnan(C.emulate_layernorm(c, "no_eps")[rows]).all()
    if case == "spike":
        h = c.h_ref[C.ln_rows("spike"), C.LN_SPIKE_COL]
        assert float(h.max()) > 10 and float(h.abs().min()) < 1e-30  # both tails of the GELU: the identity and 0
    # a variant not aimed at the case may pass it: the cases are specific
    if case == "tiny":
        assert C.ln_ratio(case, C.emulate_layernorm(c, "one_pass_var")) <= 1.0


def test_layernorm_special_rows_share_a_tile_with_ordinary_rows():
    special = set(C.LN_CONST_ROWS) | set(C.LN_SPIKE_ROWS)
    first_tile = [r for r in special if r < 128]
    assert any(r in C.LN_CONST_ROWS for r in first_tile) and any(r in C.LN_SPIKE_ROWS for r in first_tile)
    assert any(r >= 128 for r in special) and C.LN_M == 133
    for r in first_tile:  # an ordinary neighbour in the same group of four rows (one workgroup of gfc_layernorm_gelu)
        assert any(n not in special for n in range(r // 4 * 4, r // 4 * 4 + 4))
    vals = set(C.LN_SPIKE_ROWS.values())
    assert {3, -3} <= vals


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("case", C.ATT_CASES)
def test_attention_case(case):
    for run in C.ATT_RUNS:
        c = C.att_case(case, run)  # asserts exact logits and the designed pattern of the running maximum
        ratio, canary = C.att_ratio(c, C.emulate_attention(c))
        assert ratio <= 1.0 and canary, (run, ratio)
        for v, runs in C.ATT_AIMED[case].items():
            if run in runs:
                r, _ = C.att_ratio(c, C.emulate_attention(c, v))
                assert r >= MARGIN, (run, v, r)


def test_attention_bound_scales_with_the_largest_logit_sum():
    """B differs between the cases, and the bound with it; `equal` has its closed-form bound."""
    b = {case: C.att_case(case, "single").B for case in C.ATT_CASES}
    assert 250 < b["all_negative"] < 350 < b["ascending"] < 500, b
    c = C.att_case("equal", "single")
    valid = ~torch.isnan(c.ref)
    assert torch.equal(c.tol[valid], 4 * C.U * c.ref[valid].abs())
    row, nq, _, nk = c.problems[0]
    assert torch.equal(c.ref[row:row + nq, :64], (c.v[row:row + nk, :64].double().sum(0) / nk).expand(nq, 64))


def test_attention_split_shares_are_the_designed_ones():
    assert C.tiles_per_split(600, 8) == [2, 2, 2, 2, 2, 0, 0, 0] and C.tiles_per_split(600, 3) == [4, 4, 2]
    assert C.tiles_per_split(100, 3) == [1, 1, 0] and C.tiles_per_split(100, 8) == [1, 1, 0, 0, 0, 0, 0, 0]
    # ascending, split by 8: the merge weights of the early shares underflow to exactly 0
    c = C.att_case("ascending", "split8")
    C.emulate_attention(c)
    s = c.scores[0, 0]  # 96 x 600, log2 units
    w = torch.exp2(s[:, :128].max(1).values - s.max(1).values)
    assert bool((w == 0).all())
    # a variant that is not aimed at a split launch is still the correct algorithm there: merge variants need a split
    c1 = C.att_case("ascending", "nosplit")
    assert torch.equal(C.emulate_attention(c1, "merge_w1").nan_to_num(), C.emulate_attention(c1).nan_to_num())


def test_attention_cases_are_specific():
    """skip_by_lane0 is the correct algorithm wherever a 32-query tile moves as one: only `mixed` tells it apart."""
    for case in ("ascending", "descending"):
        c = C.att_case(case, "single")
        assert torch.equal(C.emulate_attention(c, "skip_by_lane0").nan_to_num(), C.emulate_attention(c).nan_to_num())
    c = C.att_case("descending", "single")  # the maximum never moves after the first half tile: no rescale is live
    assert torch.equal(C.emulate_attention(c, "no_rescale_o").nan_to_num(), C.emulate_attention(c).nan_to_num())


# ------------------------------------------------------------------------------------------------ detector head
@pytest.mark.parametrize("mode", C.DH_MODES)
@pytest.mark.parametrize("shape", C.DH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_case(shape, mode):
    c = C.dh_case(shape, mode)  # asserts integer logits and the designed cells
    assert C.dh_ratio(c, C.emulate_head(c)) <= 1.0
    for kind, aimed in C.DH_AIMED.items():
        for v, modes in aimed.items():
            if mode in modes and c.kind[kind]:
                assert C.dh_ratio(c, C.emulate_head(c, v), kind) >= MARGIN, (kind, v)
    out = C.emulate_head(c)
    for cell in c.kind["tie"]:
        assert out[cell, C.DH_TIE[0]] == out[cell, C.DH_TIE[1]] == out[cell].max()
    for cell in c.kind["all_equal"]:
        assert bool((out[cell] == out[cell, 0]).all()) and abs(float(out[cell, 0]) - 1 / 65) < 1e-8
    assert torch.equal(C.dh_from_heat(c, C.dh_to_heat(c, out)), out)


def test_head_shapes_cover_two_workgroups_and_a_tail():
    c = C.dh_case(C.DH_SHAPES[0], "affine")
    assert c.cells == 270 and all(c.kind[k] for k in C.DH_SPECIAL)
    special = sorted(i for k in C.DH_SPECIAL for i in c.kind[k])
    assert {127, 128, 255, 256, 269} <= set(special)
    assert C.dh_case(C.DH_SHAPES[1], "affine").cells == 3


# ------------------------------------------------------------------------------------- why the cases exist
def test_old_layernorm_data_admits_the_wrong_variants():
    """The data of test_linear_layernorm_gelu_fused (m = 100), rebuilt from its seed: a one-pass variance, no eps and
    eps 1e-6 all stay within that test's 2e-5."""
    m = 100
    g = torch.Generator().manual_seed(m)
    x, msg = torch.randn((m, 256), generator=g), torch.randn((m, 256), generator=g) * 2 + 0.3
    w = torch.randn((512, 512), generator=g) / 512 ** 0.5
    b = torch.randn((512,), generator=g)
    gamma, beta = torch.rand((512,), generator=g) + 0.5, torch.randn((512,), generator=g) * 0.2
    pre = F.linear(torch.cat([x, msg], 1), w, b)
    ref = F.gelu(F.layer_norm(F.linear(torch.cat([x, msg], 1).double(), w.double(), b.double()), (512,), gamma.double(),
                              beta.double(), 1e-5))
    c = types.SimpleNamespace(pre=pre, gamma=gamma, beta=beta)
    for v in (None, "one_pass_var", "no_eps", "eps_1e-6"):
        err = float((C.emulate_layernorm(c, v).double() - ref).abs().max())
        print(v, err)
        assert err < 2e-5, (v, err)


def test_old_peaky_attention_data_admits_no_max():
    """The data of test_attention_peaky_rows, rebuilt from its seed: its spike reaches a logit of about 48, where a bare
    exp does not overflow, so an online soft-max without the running maximum stays within that test's 2e-5."""
    g = torch.Generator().manual_seed(77)
    n = 320
    q, k, v = (torch.randn((n, 256), generator=g) for _ in range(3))
    k[200] = q[5] * 6
    k[3] = q[9] * 6
    for h in range(C.HEADS):
        cs = slice(64 * h, 64 * h + 64)
        s = C._scores(q[:, cs], k[:, cs])
        ref = torch.softmax(q[:, cs].double() @ k[:, cs].double().T * C.SCALE, -1) @ v[:, cs].double()
        assert 30 < float(s.max()) / C.LOG2E < 88
        for variant in (None, "no_max"):
            err = float((C._emulate_head(s, v[:, cs], 1, variant).double() - ref).abs().max())
            assert err < 2e-5, (h, variant, err)
