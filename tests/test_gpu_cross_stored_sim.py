"""Cross attention with sim = qk0 . qk1^T evaluated once (gfc_attention_cross_stored, csrc/attention.hip): the first
direction stores its raw score tiles, the second one, launched after it, loads them instead of multiplying.

Directly, on four small shapes (4 heads, head dim 64, unit-variance inputs):
 (a) the first direction's rows are gfc_attention's bit for bit;
 (b) the second direction's rows against float64 soft-max attention on the CPU, next to gfc_attention's own error on
     the same inputs.  The two differ in which operand of a score carries scale * log2(e): every product of the dot
     product is rounded once more or once less, so a score s = sum_k a_k b_k c moves by at most 2 * 2^-24 * sum_k |a_k b_k c|
     <= 2^-23 * c * |a| |b| (log2 units); a soft-max weight then by the factor 2^(+-2 ds) (numerator and normaliser), i.e.
     relatively by 2 ln2 ds, and an output, a convex combination of values, by at most that times max |v|:
         margin = 2 ln2 * 2^-23 * c * max|qk0_i| * max|qk1_j| * max|v|      (norms per head, from the inputs)
     bound   = gfc_attention's measured error + margin  (about 1.5e-5 here; a wrong tile, row or mask is off by 1e-1);
 (c) the score array is handed over full of NaN: every output is finite (what the first direction does not write the
     second must not use), and rows outside every pair stay untouched;
 (d) the bytes behind gfc_attention_cross_stored_workspace_bytes() keep their pattern, and one byte less is refused.
At model level gfc_lg_forward_packed runs the smallest uniform batch that passes the gate of the stored path (8 pairs of
128 x 128 key points, csrc/api.hip: lg_cross_chunk), and one of 129 pairs of 128 x 136 (chunks of 128 pairs: a second
chunk, of one pair), with the gate and, in a child process (GFC_CROSS_STORED=0: the knobs are read once per process),
without it."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from glue_factory_colon_amd import _native as nat  # noqa: E402
from parity_utils import record  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
HEADS, HD, SCALE = 4, 64, 0.125
GUARD, GUARD_BYTES = 0xA5, 1 << 16
WORKSPACE = 2
SHAPES = [(2, 70, 130), (3, 256, 64), (1, 333, 257), (2, 128, 128)]  # pairs, M, N
CHILD_OUT = "GFC_TEST_CROSS_STORED_OUT"  # set for the child process of the model-level test: where it leaves its outputs


def P(t):
    return nat.ptr(t)


def st():
    return nat.stream_ptr(DEV)


def _reference(qk, v, tables):
    """float64 soft-max attention, both directions; rows of no pair stay NaN."""
    qk, v = qk.double(), v.double()
    out = torch.full(qk.shape, float("nan"), dtype=torch.float64)
    for q0, nq, k0, nk in tables:
        for h in range(HEADS):
            c = slice(h * HD, (h + 1) * HD)
            p = torch.softmax(qk[q0:q0 + nq, c] @ qk[k0:k0 + nk, c].T * SCALE, dim=-1)
            out[q0:q0 + nq, c] = p @ v[k0:k0 + nk, c]
    return out


def _margin(qk, v, first):
    """The module docstring's bound on what moving the scale to the other operand can do to an output."""
    c = SCALE * math.log2(math.e)
    worst = 0.0
    for r0, m, r1, n in first:
        for h in range(HEADS):
            s = slice(h * HD, (h + 1) * HD)
            a, b = qk[r0:r0 + m, s].double().norm(dim=1).max(), qk[r1:r1 + n, s].double().norm(dim=1).max()
            vmax = max(v[r0:r0 + m, s].abs().max(), v[r1:r1 + n, s].abs().max())
            worst = max(worst, float(2 * math.log(2) * 2.0 ** -23 * c * a * b * vmax))
    return worst


@pytest.mark.parametrize("pairs,m,n", SHAPES, ids=[f"{p}x{m}x{n}" for p, m, n in SHAPES])
def test_cross_stored_direct(pairs, m, n):
    lib = nat.lib()
    g = torch.Generator().manual_seed(1000 * pairs + m + n)
    rows = pairs * (m + n)
    qk, v = torch.randn((rows, 256), generator=g), torch.randn((rows, 256), generator=g)
    first = [[p * (m + n), m, p * (m + n) + m, n] for p in range(pairs)]  # image-0 rows, then image-1 rows, per pair
    second = [[r1, nn, r0, mm] for r0, mm, r1, nn in first]
    ref = _reference(qk, v, first + second)
    dqk, dv = qk.to(DEV), v.to(DEV)
    t_first = torch.tensor(first, dtype=torch.int32, device=DEV)
    t_both = torch.tensor(first + second, dtype=torch.int32, device=DEV)

    # today's launch: the two directions as two problems (no key split: no scratch offered)
    old = torch.full((rows + 1, 256), float("nan"), device=DEV)
    nat.check(lib.gfc_attention(P(dqk), 256, P(dqk), 256, P(dv), 256, P(old), 256, P(t_both), 2 * pairs, max(m, n), HEADS,
                                SCALE, None, 0, st()), "gfc_attention")

    need = int(lib.gfc_attention_cross_stored_workspace_bytes(pairs, m, n, HEADS))
    r32 = lambda x: (x + 31) // 32 * 32  # noqa: E731
    assert need == (pairs * HEADS * r32(n) * r32(m) * 4 + 255) // 256 * 256
    buf = torch.full((need + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    buf[:need].view(torch.float32).fill_(float("nan"))  # (c)
    new = torch.full((rows + 1, 256), float("nan"), device=DEV)

    def call(nbytes):
        return lib.gfc_attention_cross_stored(P(dqk), 256, P(dv), 256, P(new), 256, P(t_first), pairs, m, n, HEADS, SCALE,
                                              P(buf), nbytes, st())

    assert call(need - 1) == WORKSPACE and call(0) == WORKSPACE  # (d), before anything is launched
    torch.cuda.synchronize()
    assert torch.isnan(new).all()
    nat.check(call(need), "gfc_attention_cross_stored")
    torch.cuda.synchronize()
    assert bool((buf[need:] == GUARD).all()), "wrote behind the score array"  # (d)
    old, new = old.cpu(), new.cpu()
    assert torch.isnan(new[rows]).all() and torch.isnan(old[rows]).all()
    assert torch.isfinite(new[:rows]).all()  # (c)

    is_first = torch.zeros(rows, dtype=torch.bool)
    for r0, mm, _, _ in first:
        is_first[r0:r0 + mm] = True
    assert torch.equal(new[:rows][is_first], old[:rows][is_first])  # (a)

    sec = ~is_first
    err_old_first = float((old[:rows][is_first].double() - ref[is_first]).abs().max())
    err_old = float((old[:rows][sec].double() - ref[sec]).abs().max())
    err_new = float((new[:rows][sec].double() - ref[sec]).abs().max())
    diff = float((new[:rows][sec] - old[:rows][sec]).abs().max())
    margin = _margin(qk, v, first)
    record(f"cross_stored_sim_{pairs}x{m}x{n}", err_second_direction_gfc_attention=err_old,
           err_second_direction_stored=err_new, err_first_direction=err_old_first, stored_vs_gfc_attention=diff,
           margin=margin)
    print(f"{pairs}x{m}x{n}: second direction vs float64: gfc_attention {err_old:.3e}, stored {err_new:.3e} "
          f"(first direction {err_old_first:.3e}); stored vs gfc_attention {diff:.3e}; margin {margin:.3e}")
    assert err_old < 1e-4  # the yardstick itself is sound
    assert err_new <= err_old + margin, (err_new, err_old, margin)  # (b)


# ------------------------------------------------------------------------------------------------ model level
MODEL_SHAPES = [(8, 128, 128), (129, 128, 136)]  # pairs, M, N


def _model_outputs():
    from glue_factory_colon_amd import lightglue

    lib = nat.lib()
    model = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.1, "n_layers": 2,
                                 "matmul_precision": "fp32"}).eval().to(DEV)
    params = model.ensure_packed(DEV)[0]
    outs = []
    for b, m, n in MODEL_SHAPES:
        g = torch.Generator().manual_seed(77 + b)
        rows = b * (m + n)
        kp = (torch.rand((rows, 2), generator=g) * torch.tensor([640.0, 480.0])).to(DEV)
        # side 1 of a pair repeats side 0's descriptors with noise, so that there is something to match
        d0 = F.normalize(torch.randn((b, m, 256), generator=g), dim=-1)
        d1 = F.normalize(torch.randn((b, n, 256), generator=g), dim=-1)
        d1[:, :m] = F.normalize(d0 + 0.05 * torch.randn((b, m, 256), generator=g), dim=-1)
        de = torch.cat([d0.reshape(-1, 256), d1.reshape(-1, 256)]).to(DEV)
        size = torch.tensor([[640.0, 480.0]] * b, device=DEV)
        need = int(lib.gfc_lg_packed_workspace_bytes(b, m, n))
        # the shape passes the gate, 7 pairs do not: the score array of one chunk (at most 128 pairs of this size) is
        # part of the workspace
        sim = int(lib.gfc_attention_cross_stored_workspace_bytes(min(b, 128), m, n, HEADS))
        assert need - int(lib.gfc_lg_packed_workspace_bytes(7, m, n)) >= sim > 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        o = [torch.full((b * m,), -7, dtype=torch.long, device=DEV), torch.full((b * n,), -7, dtype=torch.long, device=DEV),
             torch.zeros((b * m,), device=DEV), torch.zeros((b * n,), device=DEV),
             torch.zeros((b * (m + 1) * (n + 1),), device=DEV)]
        out_rows = torch.zeros((rows, 256), device=DEV)
        nat.check(lib.gfc_lg_forward_packed(ctypes.byref(params), P(kp), P(de), P(size), P(size), None, b, m, n, 0.1,
                                            P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(out_rows), P(ws), need, None,
                                            st()), "gfc_lg_forward_packed")
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in o])
    return outs


def test_model_with_and_without_the_gate():
    """matches0 / matches1 equal, scores within the 1e-4 of test_c2_batch32_matcher_stage_isolated."""
    if os.environ.get(CHILD_OUT):  # the child: the one-launch cross block
        assert os.environ.get("GFC_CROSS_STORED") == "0"
        torch.save(_model_outputs(), os.environ[CHILD_OUT])
        return
    assert os.environ.get("GFC_CROSS_STORED", "1") != "0"
    gots = _model_outputs()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "plain.pt")
        env = dict(os.environ, GFC_CROSS_STORED="0", **{CHILD_OUT: path})
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                            "test_model_with_and_without_the_gate", "-p", "no:cacheprovider"],
                           capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-800:], r.stderr[-400:])
        wants = torch.load(path)
    for (b, m, n), got, want in zip(MODEL_SHAPES, gots, wants):
        n_matches = int((want[0] >= 0).sum())
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        s_err = max(float((got[i] - want[i]).abs().max()) for i in (2, 3))
        la_err = float(((got[4] - want[4]).abs() / (1 + want[4].abs())).max())
        record(f"cross_stored_sim_model_{b}x{m}x{n}", matching_score_diff=s_err, log_assignment_rel_diff=la_err,
               matches=n_matches)
        print(f"{b}x{m}x{n}: stored vs one-launch cross block: {n_matches} matches, matching scores {s_err:.3e}, "
              f"log assignment (relative) {la_err:.3e}")
        assert n_matches > 0  # there are matches to compare
        assert s_err < 1e-4 and la_err < 1e-4, (s_err, la_err)
