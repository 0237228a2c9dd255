"""The fp16 kernel cases (tests/fp16_kernel_cases.py) can fail: proven here on the CPU.

For every exact case the range proof holds (the builder asserts it) and an independent evaluation of the contract --
the kernel's own arithmetic in plain torch: fp16 operands, fp32 sums, P rounded to fp16, the stored type -- reproduces
the expected tensor exactly.  For every bounded case that emulation stays within the tolerance.  And the acceptance
predicate rejects each named wrong variant of the contract on at least one case of each family."""
import pytest
import torch

import fp16_kernel_cases as K


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("form,m", K.GEMM_EXACT)
def test_gemm_exact_case_is_exact(form, m):
    c = K.gemm_case(form, m, "int")  # asserts the ranges
    ok, _ = c.accept(K.emulate_gemm(c))  # fp32 arithmetic gives the float64 integers: nothing was rounded
    assert ok
    rows = slice(0, m) if m <= 333 else slice(m - 200, m)  # int64 matmul: every row, or the last 200 of the large case
    a = c.a0[rows, :c.K0].long() if c.a1 is None else torch.cat([c.a0[rows, :c.K0].long(), c.a1[rows, :c.K1].long()], 1)
    acc = a @ c.w[:, :c.K0 + c.K1].long().T
    if not c.rot_cols:  # bias, alpha (in quarters), residual in integers
        y4 = (acc + c.bias.long()) * int(4 * c.alpha) + (4 * c.resid_values[rows].long() if c.resid else 0)
        assert torch.equal(y4, (c.expected[rows, :c.N].double() * 4).long())
    else:  # the rotation permutes and signs the pairs: the multiset of |t| per pair is unchanged
        t = (acc + c.bias.long())[:, :c.rot_cols].abs().reshape(len(a), -1, 2).sort(-1).values
        e = c.expected[rows, :c.rot_cols].double().long().abs().reshape(len(a), -1, 2).sort(-1).values
        assert torch.equal(t, e)
        assert torch.equal((acc + c.bias.long())[:, c.rot_cols:], c.expected[rows, c.rot_cols:c.N].double().long())
    # canaries: one row below and every column right of N
    assert torch.isnan(c.expected[m]).all() and torch.isnan(c.expected[:, c.N:]).all()
    assert not torch.isnan(c.expected[:m, :c.N]).any()


@pytest.mark.parametrize("form,m", K.GEMM_RANDOM)
def test_gemm_bounded_case_admits_the_contract(form, m):
    c = K.gemm_case(form, m, "rand")
    ok, ratio = c.accept(K.emulate_gemm(c))
    assert ok and ratio <= 1.0, ratio


def _applies(c, variant):
    return {"klast": True, "a1_for_a0": c.K1 > 0, "rot_sign": c.rot_cols > 0, "rot_swap": c.rot_cols > 0,
            "bias_after_rot": c.rot_cols > 0, "resid_before_alpha": c.form == "alpha_resid"}[variant]


@pytest.mark.parametrize("data", ["int", "rand"])
@pytest.mark.parametrize("variant", K.GEMM_VARIANTS)
def test_gemm_predicate_rejects(variant, data):
    """Every form the variant applies to rejects it, in the exact family and in the bounded one."""
    hit = 0
    for form in K.GEMM_FORMS:
        c = K.gemm_case(form, 129 if data == "int" else 333, data)
        if _applies(c, variant):
            y, _ = K.gemm_contract(c, variant)
            assert not c.accept(c.into_buffer(y))[0], (form, variant)
            hit += 1
    assert hit


def test_gemm_predicate_rejects_a_touched_canary_and_an_off_by_one():
    c = K.gemm_case("kmin", 129, "int")
    y = c.expected.clone()
    assert c.accept(y)[0]
    y[129, 3] = 0.0
    assert not c.accept(y)[0]
    y = c.expected.clone()
    y[5, 70] = 1.0
    assert not c.accept(y)[0]
    y = c.expected.clone()
    y[7, 64] += 1  # the last column of the ragged tile, off by one
    assert not c.accept(y)[0]


@pytest.mark.parametrize("k0", K.STAGING)
def test_staging_case_catches_wrong_rounding(k0):
    c = K.staging_case(k0)
    edges = K.staging_edge_values()
    assert torch.isfinite(c.a0.half()).all()  # no value overflows
    for v in (2.0 ** -25, 3 * 2.0 ** -25, 65504.0, -65504.0, 0.0):
        assert (c.a0 == v).any(), v
    assert (c.a0 == 0).any() and (torch.signbit(c.a0) & (c.a0 == 0)).any()  # +0 and -0
    assert float(c.a0.abs().max()) < 65520 and (c.a0 > 65504).any()
    # halfway points round to even; one ulp either side rounds away from it
    assert float(torch.tensor(1 + 2.0 ** -11).half()) == 1.0 and float(torch.tensor(1 + 3 * 2.0 ** -11).half()) == 1 + 2.0 ** -9
    assert float(torch.tensor(2.0 ** -25).half()) == 0.0 and float(torch.tensor(3 * 2.0 ** -25).half()) == 2.0 ** -23
    good = K.emulate_gemm(c)
    assert c.accept(good, K.emulate_gemm(c, a0=c.a0.half()))[0]
    for wrong in (K.truncate_to_half, K.double_round_to_half):
        assert (wrong(edges) != edges.half()).any()
        assert not c.accept(good, K.emulate_gemm(c, a0=wrong(c.a0)))[0], wrong.__name__
    # fp32 A truncated to fp16 instead of rounded: also far outside the bounded family's tolerance
    b = K.gemm_case("input_proj128", 333, "rand")
    y, _ = K.gemm_contract(b, a0=K.truncate_to_half(b.a0).float())
    assert not b.accept(b.into_buffer(y))[0]


# ------------------------------------------------------------------------------------------------ batched NT
@pytest.mark.parametrize("args", K.NT_CASES, ids=lambda a: "-".join(map(str, a)))
def test_nt_case(args):
    c = K.nt_case(*args)
    y = K.emulate_nt(c)
    ok, ratio = c.accept(y)
    assert ok and ratio <= 1.0
    bad = y.clone()
    bad[-1, c.M - 1, c.N - 1] += 1.0 if c.exact else 0.01 * max(1.0, float(c.ref.abs().max()))
    assert not c.accept(bad)[0]
    bad = y.clone()
    bad[0, c.M, 0] = 0.0  # the dustbin row
    assert not c.accept(bad)[0]
    if args[-1]:
        assert c.strideA > c.M * c.K and c.strideB > c.N * c.K and c.strideA % 8 == 0 and c.strideB % 8 == 0


# ------------------------------------------------------------------------------------------------ attention
SPLITS = (1, 3, 8)


def _bounded(name):
    c = K.att_case("many", n_problems=2) if name == "many" else K.att_case(name)  # the GPU test runs 64 problems
    if not hasattr(c, "host_accept"):
        c.host_accept = K.bounded_accept(c, *K.attention_reference(c))
    return c, c.host_accept


@pytest.mark.parametrize("name", K.ATT_EXACT)
def test_attention_exact_case_is_exact(name):
    c = K.att_case(name)
    for split in SPLITS:  # o * (1 / l) without a split, acc / l through the merge
        assert c.accept(K.emulate_attention(c, split))[0], split
    for q0, nq, k0, nk in c.problems:
        assert not torch.isnan(c.expected[q0:q0 + nq, :256]).any()
    if name.startswith("onehot"):
        for z, (q0, nq, k0, nk) in enumerate(c.problems):
            t, must = K.onehot_targets(nq, nk)
            used = set(t.reshape(-1).tolist())
            assert nk - 1 in used
            for split in SPLITS + (2, 4, 5, 6, 7):  # the first and last key of every split's tile range
                first = 0
                for n in K.tiles_per_split(nk, split):
                    if n:
                        assert 64 * first in used and min(64 * (first + n), nk) - 1 in used
                    first += n


@pytest.mark.parametrize("name", K.ATT_BOUNDED)
def test_attention_bounded_case_admits_the_contract(name):
    c, accept = _bounded(name)
    for split in SPLITS:
        ok, ratio = accept(K.emulate_attention(c, split))
        assert ok and ratio <= 1.0, (split, ratio)


@pytest.mark.parametrize("variant", K.ATT_VARIANTS)
def test_attention_predicates_reject(variant):
    """Each wrong kernel is rejected by at least one exact case and by at least one bounded case (the merge variants
    need a split; a duplicated last key needs nk off the 32-key chunk, and is invisible to a one-hot row)."""
    exact = ["onehot-self-2", "onehot-cross-1", "uniform-self-table", "uniform-cross-single65"]
    rejected = {n: any(not K.att_case(n).accept(K.emulate_attention(K.att_case(n), s, variant))[0] for s in SPLITS)
                for n in exact}
    assert any(rejected.values()), rejected
    if variant in ("drop_last", "drop_tile", "v_swap", "empty_w1"):
        assert rejected["onehot-self-2"] and rejected["onehot-cross-1"]
    if variant in ("drop_last", "dup_last", "drop_tile", "empty_w1"):
        assert rejected["uniform-self-table"] and rejected["uniform-cross-single65"]
    rejected = {}
    for n in ("ragged-cross", "spiked", "padded"):
        c, accept = _bounded(n)
        rejected[n] = any(not accept(K.emulate_attention(c, s, variant))[0] for s in SPLITS)
    assert rejected["ragged-cross"] and rejected["padded"], rejected


def test_attention_predicate_rejects_a_touched_canary():
    c = K.att_case("padded")
    _, accept = _bounded("padded")
    o = K.emulate_attention(c, 1)
    assert accept(o)[0]
    for r, col in ((c.o_rows - 1, 0), (0, 256), (c.problems[0][0] + c.problems[0][1], 10)):  # spare row, column 256,
        bad = o.clone()                                                                    # a key-only row
        assert torch.isnan(bad[r, col])
        bad[r, col] = 0.0
        assert not accept(bad)[0]
