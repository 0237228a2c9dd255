"""Case builders for the fp16 matcher kernels (csrc/lg_fp16.hip): gfc_linear_f16, gfc_batched_nt_f16, gfc_attention_f16.

Plain torch on the CPU, no GPU import.  Every case carries its inputs (laid out as the C ABI takes them, NaN in every
element the kernel must neither read nor write), its reference and its acceptance predicate `accept(y) -> (ok, ratio)`.
tests/test_fp16_kernel_cases_host.py proves without a GPU that the predicates reject wrong kernels (named variants of
the contract below); tests/test_gpu_fp16_kernels.py applies the same predicates to the kernels.

Three kinds of case:
  exact    small-integer data chosen so that every product, partial sum, epilogue value and stored output is exactly
           representable; the builder asserts the ranges; the output must EQUAL the integer reference.
  staging  fp32 A with values on every rounding edge of fp16: the run on A (rounded while staged) must equal, bit for
           bit, the run on A.half().
  bounded  random data against float64 on the fp16-rounded operands, per element:
             GEMM       1e-5 * sum|a||w| + 1e-6 |ref|   (+ 2^-11 |ref| + 2^-24 for an fp16 output)
             attention  2^-11 (sum_j p_j|v_j| + |O|) + 2^-24 sum_j|v_j| / l + 1e-5 sum_j p_j|v_j|,  l = sum_j exp(s_j - max s)
           (fp16 rounding of P, fp16 rounding of the output, weights in the fp16 subnormal range, fp32 statistics).
"""
import math
import types

import torch

NAN = float("nan")
HEADS = 4
SCALE = 0.125
LOG2E = 1.4426950408889634


def _gen(*key):
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % 2147483647
    return torch.Generator().manual_seed(seed)


def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def nan_pattern_equal(y, want):
    return torch.equal(torch.isnan(y), torch.isnan(want))


# =================================================================================================== GEMM
# The forms: each mirrors one call of the matcher (lg_layer_impl / gfc_lg_assign / lg_input_proj in csrc/api.hip).
# gaps = (lda0 - K0, lda1 - K1, ldw - K, ldy - N)
def _form(K0, N, K1=0, a0_f16=0, bias=True, alpha=1.0, resid=None, rot=None, y_f16=0, gaps=(0, 0, 0, 0)):
    return dict(K0=K0, K1=K1, N=N, a0_f16=a0_f16, bias=bias, alpha=alpha, resid=resid, rot=rot,
                rot_cols=512 if rot else 0, y_f16=y_f16, gaps=gaps)


GEMM_FORMS = {
    "wqkv_packed": _form(256, 768, rot="packed", y_f16=1),       # self block Wqkv: rotary on q and k, fp16 qkv
    "wqkv_tables": _form(256, 768, rot="tables", y_f16=1),
    "cross_qkv": _form(256, 512, y_f16=1),                       # cross block to_qk | to_v
    "out_proj": _form(256, 256, a0_f16=1, y_f16=1),              # fp16 context -> fp16 message
    "ffn0": _form(256, 512, K1=256),                             # [x | message] -> hbuf
    "ffn0_gap": _form(256, 512, K1=256, gaps=(4, 8, 8, 4)),      # the same with every leading dimension padded
    "ffn3": _form(512, 256, resid="inplace"),                    # hbuf -> x += ...
    "final_proj": _form(256, 256, alpha=0.25, y_f16=1),          # assignment head, scaled by dim^-1/4
    "input_proj128": _form(128, 256),                            # 128-d descriptors
    "kmin": _form(32, 65, gaps=(4, 0, 8, 7)),                    # the smallest K, a ragged column tile, ldy 72
    "alpha_resid": _form(256, 256, alpha=0.25, resid="separate"),  # tells "alpha, then residual" from the reverse
}
GEMM_ROWS = (1, 127, 128, 129, 333)
GEMM_BIG_M = 65536 - 37  # 512 row tiles: what 32 pairs dispatch
GEMM_EXACT = [(f, m) for f in GEMM_FORMS for m in GEMM_ROWS] + [("wqkv_packed", GEMM_BIG_M), ("ffn3", GEMM_BIG_M)]
GEMM_RANDOM = [(f, 333) for f in GEMM_FORMS]
GEMM_VARIANTS = ("klast", "a1_for_a0", "rot_sign", "rot_swap", "bias_after_rot", "resid_before_alpha")


def _rot_tables(M, data, g):
    """cos, sin per (row, frequency): [M, 32].  Integer data: only 0 and +-1, a different pattern per row and per
    frequency, so the rotation is exact and a swapped partner or a wrong sign changes the result."""
    if data == "int":
        r = torch.arange(M)[:, None]
        f = torch.arange(32)[None, :]
        idx = (7 * r + 3 * f + (r * f) // 5) % 4
        return torch.tensor([1.0, 0.0, -1.0, 0.0])[idx], torch.tensor([0.0, 1.0, 0.0, -1.0])[idx]
    ang = torch.rand(M, 32, generator=g) * 6.3
    return ang.cos(), ang.sin()


def gemm_contract(c, variant=None, a0=None):
    """float64 evaluation of Y = epilogue([A0 | A1] W^T) in the documented order: bias, rotary, alpha, residual, on the
    operands as the kernel multiplies them (A already rounded to fp16).  Returns (y [M, N], sum|a||w| bound [M, N]).
    `variant` names one wrong kernel (GEMM_VARIANTS)."""
    a0 = (c.a0 if a0 is None else a0)[:, :c.K0].half().double()
    a = a0 if c.a1 is None else torch.cat([a0, c.a1[:, :c.K1].double()], 1)
    w = c.w[:, :c.K0 + c.K1].double()
    if variant == "klast":          # the last 32-wide K step dropped
        a = a.clone()
        a[:, -32:] = 0
    if variant == "a1_for_a0":      # A1's K block read in place of A0's
        a = torch.cat([a[:, c.K0:], a[:, c.K0:]], 1)
    y = a @ w.T
    s = a.abs() @ w.abs().T
    late_bias = variant == "bias_after_rot"
    if c.bias is not None and not late_bias:
        y = y + c.bias.double()
    bound = s
    if c.rot_cols:
        rc = c.rot_cols
        cos = c.cos.double().repeat_interleave(2, 1).repeat(1, rc // 64)
        sin = c.sin.double().repeat_interleave(2, 1).repeat(1, rc // 64)
        t = y[:, :rc]
        partner = torch.stack([-t[:, 1::2], t[:, 0::2]], -1).reshape(t.shape)
        if variant == "rot_sign":   # the rotary partner's sign flipped
            partner = -partner
        out = t * cos + partner * sin
        if variant == "rot_swap":   # even and odd columns swapped
            out = out.reshape(-1, rc // 2, 2).flip(-1).reshape(t.shape)
        y = torch.cat([out, y[:, rc:]], 1)
        sp = s[:, :rc].reshape(-1, rc // 2, 2).flip(-1).reshape(-1, rc)
        bound = torch.cat([s[:, :rc] + sp, s[:, rc:]], 1)
    if c.bias is not None and late_bias:
        y = y + c.bias.double()
    if c.resid is not None and variant == "resid_before_alpha":
        y = (y + c.resid_values.double()) * c.alpha
    else:
        y = y * c.alpha
        if c.resid is not None:
            y = y + c.resid_values.double()
    return y, bound * abs(c.alpha)


def emulate_gemm(c, a0=None):
    """The kernel's arithmetic in plain torch: fp16-rounded operands, fp32 accumulation, fp32 epilogue in the kernel's
    order, store in Y's type.  Returns the whole Y buffer (canaries included)."""
    a0 = (c.a0 if a0 is None else a0)[:, :c.K0].half().float()
    a = a0 if c.a1 is None else torch.cat([a0, c.a1[:, :c.K1].float()], 1)
    y = a @ c.w[:, :c.K0 + c.K1].float().T
    if c.bias is not None:
        y = y + c.bias
    if c.rot_cols:
        rc = c.rot_cols
        cos = c.cos.repeat_interleave(2, 1).repeat(1, rc // 64)
        sin = c.sin.repeat_interleave(2, 1).repeat(1, rc // 64)
        t = y[:, :rc]
        partner = torch.stack([-t[:, 1::2], t[:, 0::2]], -1).reshape(t.shape)
        y = torch.cat([t * cos + partner * sin, y[:, rc:]], 1)
    y = y * c.alpha
    if c.resid is not None:
        y = c.resid_values + y
    return c.into_buffer(y)


def _finish_gemm(c, data):
    """Reference, range proof or tolerance, and the predicate."""
    def into_buffer(y):
        buf = c.y_init.clone()
        buf[:c.M, :c.N] = y.to(buf.dtype)
        return buf

    c.into_buffer = into_buffer
    ref, bound = gemm_contract(c)
    c.ref = ref
    if data == "int":
        # the range proof: every operand is a small integer (or 0 / +-1 in the rotary tables), so every partial sum is
        # an integer no larger than sum|a||w| + |bias| (twice that through the rotation) -- below 2^24, exact in fp32
        k = c.K0 + c.K1
        amax = max(float(c.a0[:, :c.K0].abs().max()), float(c.a1[:, :c.K1].abs().max()) if c.a1 is not None else 0.0)
        worst = 2 * (k * amax * float(c.w[:, :k].abs().max()) + (float(c.bias.abs().max()) if c.bias is not None else 0))
        worst += float(c.resid_values.abs().max()) if c.resid is not None else 0.0
        assert worst < 2 ** 24, worst
        assert torch.equal(ref * 4, (ref * 4).round())                    # integers or quarter-integers
        lim = 2048 if c.alpha == 1.0 else 512
        assert not c.y_f16 or float(ref.abs().max()) <= lim, float(ref.abs().max())
        c.expected = into_buffer(ref)
        assert torch.equal(c.expected[:c.M, :c.N].double(), ref)          # the stored value is the reference itself
        c.exact = True

        def accept(y):
            ok = torch.equal(y[:c.M, :c.N], c.expected[:c.M, :c.N]) and nan_pattern_equal(y, c.expected)
            return ok, 0.0
    else:
        tol = 1e-5 * bound + 1e-6 * ref.abs()
        if c.y_f16:
            tol = tol + 2.0 ** -11 * ref.abs() + 2.0 ** -24  # the output's own rounding to fp16
        c.tol = tol
        c.exact = False
        canary = torch.ones_like(c.y_init, dtype=torch.bool)  # NaN everywhere but in the output
        canary[:c.M, :c.N] = False

        def accept(y):
            err = (y[:c.M, :c.N].double() - ref).abs()
            ratio = float((err / tol).nan_to_num(nan=float("inf")).max())
            return bool((err <= tol).all()) and torch.equal(torch.isnan(y), canary), ratio
    c.accept = accept
    return c


def gemm_case(form, M, data="int"):
    """data "int": the exact family; "rand": the bounded one."""
    f = GEMM_FORMS[form]
    g = _gen("gemm", form, M, data)
    c = types.SimpleNamespace(name=f"{form}-M{M}-{data}", form=form, M=M, **{k: v for k, v in f.items() if k != "gaps"})
    K0, K1, N = c.K0, c.K1, c.N
    c.lda0, c.lda1, c.ldw, c.ldy = K0 + f["gaps"][0], K1 + f["gaps"][1], K0 + K1 + f["gaps"][2], N + f["gaps"][3]
    c.a1_f16 = 1

    def operand(rows, k, ld, lo, hi, scale, f16):
        t = torch.full((rows, ld), NAN)
        t[:, :k] = _randint(g, lo, hi, rows, k) if data == "int" else torch.randn(rows, k, generator=g) * scale
        return t.half() if f16 else t

    c.a0 = operand(M, K0, c.lda0, -4, 4, 1.0, c.a0_f16)
    c.a1 = operand(M, K1, c.lda1, -4, 4, 1.0, True) if K1 else None
    c.w = operand(N, K0 + K1, c.ldw, -3, 3, 1 / 16, True)
    c.bias = (_randint(g, -8, 8, N) if data == "int" else torch.randn(N, generator=g)) if f["bias"] else None
    c.cos = c.sin = c.cs = None
    if c.rot:
        c.cos, c.sin = _rot_tables(M, data, g)
        c.cs = torch.stack([c.cos, c.sin], -1).reshape(M, 64).contiguous()        # packed [M][32][cos, sin]
        c.cos64 = c.cos.repeat_interleave(2, 1).contiguous()                       # [M, 64], each value twice
        c.sin64 = c.sin.repeat_interleave(2, 1).contiguous()
    ydt = torch.float16 if c.y_f16 else torch.float32
    c.y_init = torch.full((M + 1, c.ldy), NAN, dtype=ydt)  # one canary row below, canary columns right of N
    c.resid_values = None
    c.resid_buf = None
    if c.resid:
        c.resid_values = _randint(g, -64, 64, M, N) if data == "int" else torch.randn(M, N, generator=g)
        if c.resid == "inplace":
            c.y_init[:M, :N] = c.resid_values
        else:
            c.resid_buf = torch.full((M + 1, c.ldy), NAN)
            c.resid_buf[:M, :N] = c.resid_values
    return _finish_gemm(c, data)


# --------------------------------------------------------------------------------------- staging rounding (family B)
def staging_edge_values():
    """fp32 values on every rounding edge of fp16 (none overflows)."""
    f32 = torch.float32
    vals = []
    for base in (1.0, 1.0 + 2.0 ** -10, 1.5, 1.5 + 2.0 ** -10, 1024.0, 1025.0, 2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -10)):
        ulp = 2.0 ** (math.floor(math.log2(base)) - 10)
        half = torch.tensor(base + ulp / 2, dtype=f32)  # exact halfway; lower neighbour even (first of each pair) / odd
        vals += [half, torch.nextafter(half, torch.tensor(0.0)), torch.nextafter(half, torch.tensor(1e9))]
    # rounds up into the next binade
    vals += [torch.tensor(v, dtype=f32) for v in (2 - 2.0 ** -11, 2 - 2.0 ** -12, 4096 - 1.0, 4096 - 0.5)]
    # the fp16 subnormal range: spacing 2^-24
    sub = [2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -26, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -24,
           1023.5 * 2.0 ** -24, 7 * 2.0 ** -26]
    for v in sub:
        t = torch.tensor(v, dtype=f32)
        vals += [t, torch.nextafter(t, torch.tensor(0.0)), torch.nextafter(t, torch.tensor(1.0))]
    vals += [torch.tensor(v, dtype=f32) for v in (0.0, 65504.0, 65504.0 + 8, 65504.0 - 16)]
    vals.append(torch.nextafter(torch.tensor(65520.0), torch.tensor(0.0)))  # the largest fp32 that does not overflow
    v = torch.stack(vals)
    v = torch.cat([v, -v])
    assert torch.isfinite(v.half()).all()
    return v


def truncate_to_half(a):
    """fp32 -> fp16 rounded toward zero (the wrong staging family B is there to catch)."""
    h = a.half()
    bits = h.view(torch.int16)
    too_big = h.float().abs() > a.abs()
    return torch.where(too_big, bits - 1, bits).view(torch.float16)


def double_round_to_half(a):
    """fp32 -> 13 significant bits -> fp16: the other wrong staging (a value just above halfway lands on it first)."""
    m, e = torch.frexp(a.double())
    mid = torch.ldexp((m * 2 ** 13).round() / 2 ** 13, e).float()
    return torch.where(a.abs() < 2.0 ** -14, a, mid).half()


STAGING = (256, 512)


def staging_case(K0):
    """fp32 A with the edge values planted through every row tile and every staging slot, random elsewhere; fp32 Y.
    `equal(y_from_f32, y_from_half)` is the predicate: both runs execute the same code after staging."""
    g = _gen("staging", K0)
    M, N = 200, 128
    a = torch.randn(M, K0, generator=g)
    edges = staging_edge_values()
    flat = a.reshape(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:4 * edges.numel()]
    flat[pos] = edges.repeat(4)
    a[0, :edges.numel()] = edges[:K0] if edges.numel() > K0 else edges
    a[M - 1, -min(K0, edges.numel()):] = edges[:min(K0, edges.numel())]
    c = types.SimpleNamespace(name=f"staging-K{K0}", form="staging", M=M, N=N, K0=K0, K1=0, a0_f16=0, a1_f16=1, bias=None,
                              alpha=1.0, resid=None, resid_values=None, resid_buf=None, rot=None, rot_cols=0, cos=None,
                              sin=None, cs=None, y_f16=0, lda0=K0, lda1=0, ldw=K0, ldy=N, a0=a, a1=None)
    # W: powers of two and small integers mixed with random values, so that a one-ulp change of A is never rounded away
    c.w = torch.where(torch.rand(N, K0, generator=g) < 0.5, _randint(g, -2, 2, N, K0), torch.randn(N, K0, generator=g) / 16).half()
    c.y_init = torch.full((M + 1, N), NAN)

    def into_buffer(y):
        buf = c.y_init.clone()
        buf[:M, :N] = y
        return buf

    c.into_buffer = into_buffer

    def accept(y_f32_run, y_half_run):
        return torch.equal(y_f32_run.view(torch.int32), y_half_run.view(torch.int32)), 0.0

    c.accept = accept
    return c


# =================================================================================================== batched NT
NT_CASES = [(b, m, n, k, data, 0) for (b, m, n) in ((1, 1, 1), (2, 128, 128), (3, 129, 257), (1, 1024, 1025))
            for k in (32, 256) for data in ("int", "rand")] + [(3, 129, 257, 32, "int", 24), (3, 129, 257, 256, "rand", 8)]


def nt_case(B, M, N, K, data, gap):
    """Y_z = A_z B_z^T into the [B, M+1, N+1] log-assignment layout; the dustbin row and column are canaries.
    gap > 0: strideA and strideB exceed M*K and N*K (the gap holds NaN)."""
    g = _gen("nt", B, M, N, K, data, gap)
    c = types.SimpleNamespace(name=f"nt-{B}x{M}x{N}-K{K}-{data}-gap{gap}", B=B, M=M, N=N, K=K,
                              strideA=M * K + gap, strideB=N * K + gap)

    def operand(rows, stride):
        buf = torch.full((B, stride), NAN)
        buf[:, :rows * K] = (_randint(g, -4, 4, B, rows * K) if data == "int" else torch.randn(B, rows * K, generator=g))
        return buf.half()

    c.a, c.b = operand(M, c.strideA), operand(N, c.strideB)
    ad = c.a[:, :M * K].reshape(B, M, K).double()
    bd = c.b[:, :N * K].reshape(B, N, K).double()
    ref = ad @ bd.transpose(1, 2)
    c.ref = ref
    c.y_init = torch.full((B, M + 1, N + 1), NAN)
    c.exact = data == "int"
    if c.exact:
        assert K * 16 < 2 ** 24
        c.expected = c.y_init.clone()
        c.expected[:, :M, :N] = ref.float()
        assert torch.equal(c.expected[:, :M, :N].double(), ref)

        def accept(y):
            return torch.equal(y[:, :M, :N], c.expected[:, :M, :N]) and nan_pattern_equal(y, c.expected), 0.0
    else:
        tol = 1e-5 * (ad.abs() @ bd.abs().transpose(1, 2))
        c.tol = tol
        canary = torch.ones_like(c.y_init, dtype=torch.bool)  # NaN everywhere but in the output
        canary[:, :M, :N] = False

        def accept(y):
            err = (y[:, :M, :N].double() - ref).abs()
            ratio = float((err / tol).nan_to_num(nan=float("inf")).max())
            return bool((err <= tol).all()) and torch.equal(torch.isnan(y), canary), ratio
    c.accept = accept
    return c


def emulate_nt(c):
    a = c.a[:, :c.M * c.K].reshape(c.B, c.M, c.K).float()
    b = c.b[:, :c.N * c.K].reshape(c.B, c.N, c.K).float()
    y = c.y_init.clone()
    y[:, :c.M, :c.N] = a @ b.transpose(1, 2)
    return y


# =================================================================================================== attention
# Layouts.  "self": one [rows, 768] buffer Q | K | V, problem z uses rows off_z .. off_z + max(nq, nk) for both sides.
# "cross": one [rows, 512] buffer QK | V with Q and K read through the SAME pointer; a problem's queries and keys are
# different row ranges.  Rows / columns a problem does not use hold NaN.
ATT_VARIANTS = ("drop_last", "dup_last", "drop_tile", "merge_w1", "empty_w1", "v_swap")
ONEHOT_PROBLEMS = ((64, 64), (300, 65), (129, 576), (1000, 1000), (37, 2048), (2048, 2048))
UNIFORM_NK = (1, 31, 33, 64, 65, 1000, 2047, 2048)
UNIFORM_NQ = (1, 31, 129, 64, 300, 200, 37, 130)
RAGGED_NS = (1, 31, 64, 65, 1000, 2048)


def _att_shell(name, layout, shapes, ldo=256, max_nq=None, extra_o_rows=0):
    """shapes: [(nq, nk)].  Allocates the buffer (NaN) and the problem table."""
    c = types.SimpleNamespace(name=name, layout=layout)
    c.ld, c.qcol, c.kcol, c.vcol = (768, 0, 256, 512) if layout == "self" else (512, 0, 0, 256)
    off, c.problems = 0, []
    for nq, nk in shapes:
        if layout == "self":
            c.problems.append([off, nq, off, nk])
            off += max(nq, nk)
        else:
            c.problems.append([off, nq, off + nq, nk])
            off += nq + nk
    c.rows = off
    c.x = torch.full((off, c.ld), NAN)
    c.max_nq = max_nq or max(nq for nq, _ in shapes)
    c.ldo = ldo
    c.o_rows = off + extra_o_rows
    return c


def att_parts(c, z, head):
    """(Q [nq, 64], K [nk, 64], V [nk, 64]) of problem z, one head, as stored (fp16)."""
    q0, nq, k0, nk = c.problems[z]
    h = slice(64 * head, 64 * head + 64)
    return (c.x[q0:q0 + nq, c.qcol:c.qcol + 256][:, h], c.x[k0:k0 + nk, c.kcol:c.kcol + 256][:, h],
            c.x[k0:k0 + nk, c.vcol:c.vcol + 256][:, h])


def o_blank(c, dtype=torch.float16):
    return torch.full((c.o_rows, c.ldo), NAN, dtype=dtype)


def _exact_accept(c):
    def accept(o):
        valid = ~torch.isnan(c.expected)
        return torch.equal(o[valid], c.expected[valid]) and nan_pattern_equal(o, c.expected), 0.0
    return accept


def _onehot_key(j):
    """16 (e_{j mod 16} + e_{16 + (j div 16) mod 16} + e_{32 + (j div 256) mod 16}): distinct for j < 4096."""
    k = torch.zeros(j.numel(), 64)
    r = torch.arange(j.numel())
    k[r, j % 16] = 16.0
    k[r, 16 + (j // 16) % 16] = 16.0
    k[r, 32 + (j // 256) % 16] = 16.0
    return k


def onehot_targets(nq, nk):
    """t[i, head]: the last key, the first and last key of every 64-key tile (which include the first and last key of
    every split's tile range, whatever the split), then the spread (5 i + 3) mod nk; dealt over the nq * HEADS slots."""
    must = sorted({nk - 1} | {k for t in range(0, nk, 64) for k in (t, min(t + 63, nk - 1))})
    pool = must + [(5 * i + 3) % nk for i in range(max(0, nq * HEADS - len(must)))]
    assert len(must) <= nq * HEADS, (nq, nk)
    return torch.tensor(pool[:nq * HEADS]).reshape(HEADS, nq).T.contiguous(), must


def onehot_case(layout, shapes, name=None):
    """Query (i, head) is the key vector of its target: the target scores 16 * 16 * 3 / 8 = 96, every other key at most
    64, so every other weight is at most e^-32 (0 in fp16) and O[i] must equal V[target] exactly."""
    c = _att_shell(name or f"onehot-{layout}-" + "+".join(f"{a}x{b}" for a, b in shapes), layout, shapes)
    c.expected = o_blank(c)
    for z, (q0, nq, k0, nk) in enumerate(c.problems):
        assert nk <= 4096
        keys = _onehot_key(torch.arange(nk))
        t, must = onehot_targets(nq, nk)
        assert set(must) <= set(t.reshape(-1).tolist())
        j = torch.arange(nk)[:, None]
        col = torch.arange(256)[None, :]
        a = (7 * col + 13 * z) % 4000 + 1  # 1 .. 4000, and 4001 is prime: j -> a j + b is injective mod 4001
        v = ((j * a + 31 * col + 977 * z) % 4001 - 2000).float()  # distinct integers in [-2000, 2000] down each column
        assert nk == 1 or (v.sort(0).values.diff(dim=0) > 0).all()
        for h in range(HEADS):
            cs = slice(64 * h, 64 * h + 64)
            c.x[q0:q0 + nq, c.qcol + 64 * h:c.qcol + 64 * h + 64] = keys[t[:, h]]
            c.x[k0:k0 + nk, c.kcol + 64 * h:c.kcol + 64 * h + 64] = keys
            # the proof: target 96, every other key <= 64 after the 0.125 scale
            s = keys[t[:, h]] @ keys.T * SCALE
            top2 = s.topk(min(2, nk), -1).values
            assert (top2[:, 0] == 96).all() and (nk == 1 or (top2[:, 1] <= 64).all())
            c.expected[q0:q0 + nq, cs] = v[t[:, h], cs].half()
        c.x[k0:k0 + nk, c.vcol:c.vcol + 256] = v
    c.x = c.x.half()
    assert float(c.x.nan_to_num().abs().max()) <= 2000
    c.exact = True
    c.accept = _exact_accept(c)
    return c


def uniform_case(layout, shapes, name=None):
    """Q = 0: every score is 0, every weight exactly 1, O is the mean of V.  V = c_col + d with integer c_col in
    [-16, 16] and integer d in [-8, 8] whose last row makes every column of d sum to zero: O must equal c_col exactly
    (the sums are integers below 2^24; nk c fl(1/nk) and nk c / nk both round to c in fp16).  Dropping the last key, or
    counting a clamped copy of it, moves most columns by many fp16 ulps."""
    c = _att_shell(name or f"uniform-{layout}-{len(shapes)}", layout, shapes)
    g = _gen("uniform", layout, shapes)
    c.expected = o_blank(c)
    for z, (q0, nq, k0, nk) in enumerate(c.problems):
        ccol = _randint(g, -16, 16, 256)
        d = _randint(g, -8, 8, nk, 256)
        d[nk - 1] = 0
        d[nk - 1] = -d.sum(0)
        v = ccol + d
        assert float(v.abs().max()) <= 2048 and float(v.abs().sum(0).max()) < 2 ** 24
        assert torch.equal(v.double().sum(0), nk * ccol.double())
        c.x[k0:k0 + nk, c.kcol:c.kcol + 256] = torch.randn(nk, 256, generator=g)
        c.x[q0:q0 + nq, c.qcol:c.qcol + 256] = 0.0  # Q and K: different columns (self) or different rows (cross)
        c.x[k0:k0 + nk, c.vcol:c.vcol + 256] = v
        c.expected[q0:q0 + nq, :256] = ccol.half()
    c.x = c.x.half()
    c.exact = True
    c.accept = _exact_accept(c)
    return c


def attention_reference(c, device="cpu", problems=None):
    """float64 on the fp16-rounded operands, and the per-element tolerance of the module docstring.  Returns
    (ref, tol) as [o_rows, ldo] float64 tensors on the CPU, NaN outside every problem."""
    ref, tol = o_blank(c, torch.float64), o_blank(c, torch.float64)
    x = c.x.to(device).double()
    for z in (range(len(c.problems)) if problems is None else problems):
        q0, nq, k0, nk = c.problems[z]
        for h in range(HEADS):
            cs = slice(64 * h, 64 * h + 64)
            q = x[q0:q0 + nq, c.qcol:c.qcol + 256][:, cs]
            k = x[k0:k0 + nk, c.kcol:c.kcol + 256][:, cs]
            v = x[k0:k0 + nk, c.vcol:c.vcol + 256][:, cs]
            s = q @ k.T * SCALE
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            l = e.sum(-1, keepdim=True)
            p = e / l
            o, pv = p @ v, p @ v.abs()
            t = 2.0 ** -11 * (pv + o.abs()) + 2.0 ** -24 * v.abs().sum(0, keepdim=True) / l + 1e-5 * pv
            ref[q0:q0 + nq, cs] = o.cpu()
            tol[q0:q0 + nq, cs] = t.cpu()
    return ref, tol


def bounded_accept(c, ref, tol):
    def accept(o):
        valid = ~torch.isnan(ref)
        err = (o.double()[valid] - ref[valid]).abs()
        ratio = float((err / tol[valid]).nan_to_num(nan=float("inf")).max())
        return bool((err <= tol[valid]).all()) and nan_pattern_equal(o, ref), ratio
    return accept


def _random_fill(c, g):
    c.x = (torch.randn(c.rows, c.ld, generator=g) * 1.5).half()


def ragged_case(layout):
    """The problem tables of test_attention_f16_ragged_vs_float64."""
    ns = RAGGED_NS
    if layout == "self":
        c = _att_shell("ragged-self", "self", [(n, n) for n in ns])
    else:  # each image's rows are queries of one problem and keys of its mirror: (1, 2048), (31, 1000), (64, 65) and back
        c = _att_shell("ragged-cross", "cross", [(1, 1)])
        offs = [sum(ns[:i]) for i in range(len(ns))]
        c.problems = []
        for a, b in ((0, 5), (1, 4), (2, 3)):
            c.problems += [[offs[a], ns[a], offs[b], ns[b]], [offs[b], ns[b], offs[a], ns[a]]]
        c.rows = c.o_rows = sum(ns)
        c.max_nq = max(ns)
    _random_fill(c, _gen("ragged", layout))
    c.exact = False
    return c


def many_case(n_problems=64):
    """n problems of 1024 x 1024: with 64 of them no key split even with scratch (one launch of 2048 workgroups)."""
    c = _att_shell(f"many-{n_problems}x1024", "self", [(1024, 1024)] * n_problems)
    _random_fill(c, _gen("many"))
    c.exact = False
    return c


def spiked_case():
    """One late and one early spiked key (as test_attention_peaky_rows): the running-max rescale at a chosen tile."""
    n = 320
    c = _att_shell("spiked", "self", [(n, n)])
    g = _gen("spiked")
    x = torch.randn(n, 768, generator=g)
    x[200, 256:512] = x[5, :256] * 6   # late, very large score for query 5
    x[3, 256:512] = x[9, :256] * 6     # early spike for query 9
    c.x = x.half()
    c.exact = False
    return c


def padded_case():
    """max_nq above every problem's nq, ldo = 260, two spare rows: rows and columns outside every problem stay NaN."""
    c = _att_shell("padded-ldo260", "cross", [(40, 100), (200, 77), (129, 300)], ldo=260, max_nq=256, extra_o_rows=2)
    _random_fill(c, _gen("padded"))
    c.exact = False
    return c


ATT_EXACT = ([f"onehot-{lay}-{i}" for lay in ("self", "cross") for i in range(len(ONEHOT_PROBLEMS) + 1)] +
             [f"uniform-{lay}-{k}" for lay in ("self", "cross") for k in ("table", "single65")])
ATT_BOUNDED = ["ragged-self", "ragged-cross", "many", "spiked", "padded"]
_CACHE = {}


def att_case(name, **kw):
    """Cases by name (built once per process and never modified)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        kind, _, rest = name.partition("-")
        if kind == "onehot":
            lay, i = rest.split("-")
            shapes = list(ONEHOT_PROBLEMS) if int(i) == len(ONEHOT_PROBLEMS) else [ONEHOT_PROBLEMS[int(i)]]
            c = onehot_case(lay, shapes, name)
        elif kind == "uniform":
            lay, which = rest.split("-")
            shapes = list(zip(UNIFORM_NQ, UNIFORM_NK)) if which == "table" else [(130, 65)]
            c = uniform_case(lay, shapes, name)
        elif name == "many":
            c = many_case(**kw)
        else:
            c = {"ragged-self": lambda: ragged_case("self"), "ragged-cross": lambda: ragged_case("cross"),
                 "spiked": spiked_case, "padded": padded_case}[name]()
        _CACHE[key] = c
    return _CACHE[key]


def tiles_per_split(nk, split):
    """The kernel's share of 64-key tiles per split (attention_f16_kernel: kt0, kt1)."""
    nt = (nk + 63) // 64
    per = (nt + split - 1) // split
    return [max(0, min(nt, (s + 1) * per) - s * per) for s in range(split)]


def _emulate_head(q, k, v, split, variant):
    """One (problem, head) in the kernel's arithmetic: fp32 scores of the fp16 operands, per split the weights relative
    to the split's maximum, rounded to fp16 for P V, fp32 sums, the merge of the partials, an fp16 store.  `variant`
    names one wrong kernel (ATT_VARIANTS)."""
    nq, nk = q.shape[0], k.shape[0]
    nt = (nk + 63) // 64
    idx = torch.arange(nt * 64).clamp(max=nk - 1)  # the kernel's clamped loads
    kf, vf = k.float()[idx], v.float()[idx]
    valid = torch.arange(nt * 64) < nk
    if variant == "drop_last":     # the last key dropped
        valid[nk - 1] = False
    if variant == "dup_last":      # the last key counted again for each padded slot of its 32-key chunk
        valid[nk:(nk + 31) // 32 * 32] = True
    if variant == "drop_tile":     # one whole 64-key tile dropped
        t = nt // 2
        valid[64 * t:64 * t + 64] = False
    if variant == "v_swap":        # keys 4-7 and 8-11 of a 16-key step swapped when V is read
        perm = torch.arange(nt * 64).reshape(-1, 4, 4)[:, [0, 2, 1, 3]].reshape(-1)
        vf = vf[perm]
    s = (q.float() @ kf.T) * (SCALE * LOG2E)
    s = torch.where(valid[None, :], s, torch.tensor(-float("inf")))
    per = (nt + split - 1) // split
    parts = []
    for sp in range(split):
        lo, hi = 64 * sp * per, 64 * min(nt, (sp + 1) * per)
        if lo >= hi:
            if variant == "empty_w1":  # an empty split merged with weight 1, as if its slot held the clamped last key
                parts.append((v.float()[nk - 1].expand(nq, 64), None, torch.ones(nq)))
            continue
        ss = s[:, lo:hi]
        m = ss.max(-1).values
        p = torch.exp2(ss - torch.where(torch.isinf(m), torch.zeros_like(m), m)[:, None])
        parts.append((p.half().float() @ vf[lo:hi], m, p.sum(-1)))
    if split == 1:
        o, _, l = parts[0]
        return (o * (1.0 / l)[:, None]).half()
    mall = torch.stack([m for _, m, _ in parts if m is not None]).max(0).values
    acc, lsum = torch.zeros(nq, 64), torch.zeros(nq)
    for o, m, l in parts:
        if m is None or variant == "merge_w1":  # split partials merged with weight 1 instead of exp2(m_s - m)
            wgt = torch.ones(nq) if m is None else (~torch.isinf(m)).float()
        else:
            wgt = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - mall))
        acc += wgt[:, None] * o
        lsum += wgt * l
    return (acc / lsum[:, None]).half()


def emulate_attention(c, split=1, variant=None, problems=None):
    o = o_blank(c)
    for z in (range(len(c.problems)) if problems is None else problems):
        q0, nq = c.problems[z][:2]
        for h in range(HEADS):
            o[q0:q0 + nq, 64 * h:64 * h + 64] = _emulate_head(*att_parts(c, z, h), split, variant)
    return o
