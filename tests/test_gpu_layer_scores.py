"""gfc_lg_layer_scores alone against the float64 restatement (tests/layer_loss_reference.py) on the same input bits.

No excuse band: correct0 / correct1 and the four counts are exact.  bce0 / bce1 are held to a bound derived per case
from the kernel's arithmetic: each term max(x,0) - x y + log1p(exp(-|x|)) is evaluated in fp32 -- x y and the
subtraction are exact for y in {0, 1}; expf is within 1 ulp, which moves l = log1p(e) by at most 2^-23 l (l >= e / (1 +
e)); log1pf is within 2 ulp of l; the final addition rounds once (2^-24 of the term) -- so a term is within 4 * 2^-23 of
itself; the sum and the mean are fp64, the result is rounded to fp32 once (2^-24).  Bound: (4 * 2^-23 + 2^-24) * bce.

Shapes: the issue's six, the edges of the kernel's decomposition by one either way (16 rows per row workgroup, 128-row
column chunks of the M + 1 rows, 256-column tiles, the 16-byte vector loop of a row of N + 1 entries), and 2 x 2048 x
2048.  N + 1 odd puts row starts at every 4-byte phase of a 16-byte line.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_loss_reference as lr  # noqa: E402

from glue_factory_colon_amd import _native as nat  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 65, 1), (2, 1, 65), (3, 63, 64), (3, 64, 63), (2, 257, 130),
          (1, 15, 255), (1, 16, 256), (1, 17, 257), (2, 126, 259), (1, 127, 3), (1, 128, 5), (1, 129, 260),
          (2, 2048, 2048)]
BCE_REL = 4 * 2.0 ** -23 + 2.0 ** -24


def run_kernel(la, lf, x0, x1, thr, with_correct=True, ws_bytes=None):
    b, m, n = la.shape[0], la.shape[1] - 1, la.shape[2] - 1
    dev = torch.device("cuda")
    need = nat.call("gfc_lg_layer_scores_workspace_bytes", b, m, n)
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 16), dtype=torch.uint8, device=dev)
    out = torch.full((b, 6), float("nan"), device=dev)
    c0 = torch.full((b, m), 7, dtype=torch.uint8, device=dev) if with_correct else None
    c1 = torch.full((b, n), 7, dtype=torch.uint8, device=dev) if with_correct else None
    nat.call("gfc_lg_layer_scores", la.to(dev), lf.to(dev), x0.to(dev), x1.to(dev), float(thr), b, m, n, out, c0, c1,
             ws, ws.numel() if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    return out.cpu(), None if c0 is None else c0.cpu(), None if c1 is None else c1.cpu()


def restated(la, lf, x0, x1, thr):
    """The restatement on the same bits: arg-max and BCE in float64, the confident predicate on the float32 sigmoid."""
    out, c0, c1 = lr.layer_scores(la.double(), lf.double(), x0.double(), x1.double(), float(thr))
    n0, n1 = lr.confident_counts(x0, x1, torch.tensor(thr, dtype=torch.float32))
    for p in (torch.sigmoid(x0), torch.sigmoid(x1)):  # the inputs keep clear of the threshold, the planted 0.5 aside
        d = (p - thr).abs()
        assert not bool(((d > 0) & (d < 1e-6)).any())
    out[:, 4], out[:, 5] = n0.double(), n1.double()
    return out, c0, c1


def check(tag, got, want):
    (out, c0, c1), (ref, r0, r1) = got, want
    if c0 is not None:
        assert torch.equal(c0.bool(), r0) and torch.equal(c1.bool(), r1), tag
        assert int(c0.max()) <= 1 and int(c1.max()) <= 1, tag
    for k in (0, 1, 4, 5):
        assert torch.equal(out[:, k].double(), ref[:, k]), (tag, k, out[:, k].tolist(), ref[:, k].tolist())
    for k in (2, 3):
        err = (out[:, k].double() - ref[:, k]).abs()
        tol = BCE_REL * ref[:, k].abs()
        print(f"{tag}: bce{k - 2} worst error / bound {float((err / tol.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= tol).all()), (tag, k, err.tolist(), tol.tolist())


def random_case(b, m, n, seed):
    g = torch.Generator().manual_seed(seed)
    la = -8.0 * torch.rand((b, m + 1, n + 1), generator=g)
    # the final assignment: the layer's, disturbed so that roughly half of the arg-maxima move
    lf = la + 0.6 * torch.randn((b, m + 1, n + 1), generator=g) * (torch.rand((b, m + 1, n + 1), generator=g) < 0.5)
    x0, x1 = 3.0 * torch.randn((b, m), generator=g), 3.0 * torch.randn((b, n), generator=g)
    return la, lf, x0, x1


@pytest.fixture(scope="module")
def large():
    """2 x 2048 x 2048 with its float64 restatement, computed once."""
    case = random_case(2, 2048, 2048, 99)
    return case, restated(*case, 0.87)


@pytest.mark.parametrize("shape", SHAPES[:-1], ids=lambda s: "x".join(map(str, s)))
def test_shapes(shape):
    case = random_case(*shape, seed=sum(shape))
    want = restated(*case, 0.87)
    check(str(shape), run_kernel(*case, 0.87), want)
    if shape in ((3, 63, 64), (2, 257, 130)):  # NULL correct pointers: the same out
        out, c0, c1 = run_kernel(*case, 0.87, with_correct=False)
        assert c0 is None and c1 is None
        check(str(shape) + " no correct", (out, None, None), want)
    b, m, n = shape
    both = int(want[1].sum()) + int(want[2].sum())
    assert b * (m + n) < 100 or 0 < both < b * (m + n)  # the case has agreeing and disagreeing points


def test_large(large):
    case, want = large
    check("2x2048x2048", run_kernel(*case, 0.87), want)


def test_planted_cases():
    b, m, n = 2, 70, 67
    la, lf, x0, x1 = random_case(b, m, n, 5)
    inf, nan = float("inf"), float("nan")
    # rows of pair 0 ------------------------------------------------------------------------------------------
    la[0, 0, 3] = la[0, 0, 9] = 50.0; lf[0, 0, 3] = 50.0            # a tie inside a row: the lower index wins -> agree
    la[0, 1, 5] = la[0, 1, n] = 51.0; lf[0, 1, 5] = 51.0            # the dustbin ties with a real column -> the column
    lf[0, 2, 5] = lf[0, 2, n] = 52.0; la[0, 2, n] = 52.0            # ... in the final matrix: it resolves to 5, not n
    la[0, 3, n] = 53.0; lf[0, 3, 7] = 53.0                          # the arg-max in the dustbin on one matrix only
    la[0, 4, 0] = lf[0, 4, 0] = 54.0                                # first column
    la[0, 5, n] = lf[0, 5, n] = 55.0                                # last column (the dustbin)
    la[0, 6, n - 1] = lf[0, 6, n - 1] = 56.0                        # last real column
    la[0, 7, 4] = inf; lf[0, 7, 4] = 1e30; la[0, 7, 10:20] = -inf   # +inf and -inf entries
    la[0, 8, 2] = nan; la[0, 8, 30] = 57.0; lf[0, 8, 30] = 57.0     # a NaN is skipped: the arg-max is 30 in both
    la[0, 9, :] = -inf; lf[0, 9, 0] = 58.0                          # nothing above -inf: index 0, as the final
    la[0, 10, :] = nan; lf[0, 10, 1] = 58.0                         # all NaN: index 0 as well, final 1
    # columns of pair 1 ---------------------------------------------------------------------------------------
    la[1, 2, 3] = la[1, 40, 3] = 60.0; lf[1, 2, 3] = 60.0           # a tie inside a column: the lower row wins
    la[1, 6, 4] = la[1, m, 4] = 61.0; lf[1, 6, 4] = 61.0            # the dustbin row ties with a real row
    la[1, m, 5] = 62.0; lf[1, 11, 5] = 62.0                         # the dustbin row on one matrix only
    la[1, 0, 6] = lf[1, 0, 6] = 63.0                                # first row
    la[1, m, 7] = lf[1, m, 7] = 64.0                                # last row (the dustbin)
    la[1, m - 1, 8] = lf[1, m - 1, 8] = 65.0                        # last real row
    la[1, 12, 9] = inf; lf[1, 12, 9] = inf; la[1, 13:30, 9] = -inf; lf[1, 50, 9] = inf  # +inf twice: the first
    la[1, 14, 10] = nan; lf[1, 14, 10] = nan                        # a NaN in a column of both
    # logits: 0 (probability exactly 0.5 = the threshold: confident), +-88, +-1e4 (the BCE stays finite)
    x0[0, :5] = torch.tensor([0.0, 88.0, -88.0, 1e4, -1e4])
    x1[1, :5] = torch.tensor([0.0, 88.0, -88.0, 1e4, -1e4])
    thr = 0.5
    want = restated(la, lf, x0, x1, thr)
    ref, r0, r1 = want
    # the plants mean what the comments say (read off the restatement)
    assert r0[0, :11].tolist() == [True, True, False, False, True, True, True, True, True, True, False]
    assert r1[1, 3:11].tolist() == [True, True, False, True, True, True, True, r1[1, 10].item()]
    assert lr.argmax_low(la[0, :-1, :].double(), 1)[:3].tolist() == [3, 5, n]
    assert lr.argmax_low(lf[0, :-1, :].double(), 1)[2].item() == 5
    got = run_kernel(la, lf, x0, x1, thr)
    check("planted", got, want)
    assert bool(torch.isfinite(got[0]).all())
    # the logit 0 sits exactly on the threshold and counts as confident; just above it, it would not
    lo = run_kernel(la, lf, torch.zeros_like(x0), torch.zeros_like(x1), 0.5)[0]
    hi = run_kernel(la, lf, torch.zeros_like(x0), torch.zeros_like(x1), 0.5000001)[0]
    assert lo[:, 4].tolist() == [m, m] and lo[:, 5].tolist() == [n, n]
    assert hi[:, 4].tolist() == [0, 0] and hi[:, 5].tolist() == [0, 0]


def test_refused_before_any_launch():
    la, lf, x0, x1 = random_case(1, 20, 9, 3)
    need = nat.call("gfc_lg_layer_scores_workspace_bytes", 1, 20, 9)
    with pytest.raises(nat.NativeError, match="GFC_ERR_WORKSPACE"):
        run_kernel(la, lf, x0, x1, 0.5, ws_bytes=need - 1)
    dev = torch.device("cuda")
    small = torch.zeros(64, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    out = torch.full((1, 6), 3.0, device=dev)
    for b, m, n in ((1, 65536, 1), (1, 1, 65536), (65536, 1, 1), (1, 0, 4), (1, 4, 0), (0, 4, 4)):
        assert nat.call("gfc_lg_layer_scores_workspace_bytes", b, m, n) == 0
        with pytest.raises(nat.NativeError, match="GFC_ERR_INVALID"):
            nat.call("gfc_lg_layer_scores", small, small, small, small, 0.5, b, m, n, out, None, None, ws, ws.numel())
    torch.cuda.synchronize()
    assert out.tolist() == [[3.0] * 6]  # nothing was written
