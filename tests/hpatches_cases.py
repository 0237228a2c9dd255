"""Seeded inputs of the HPatches match-metric and DLT tests, shared by the host test (which shows on the CPU that they
meet the conditions the GPU test leans on) and tests/test_gpu_eval_homography.py.  Key points are float32, as the
kernels receive them; all coordinates stay below 4096 (hpatches_reference.DELTA)."""
import torch

SIZE = torch.tensor([640.0, 480.0])
# |dH_ij| <= 2^-23 |H_ij| + 1e-9 max|H|: the kernel's single float32 rounding of a float64 result (with a factor 2),
# plus the eigen-solver (every case has kappa * 2^-52 <= 1e-11: 100 x room by the reference's own conditioning)
DLT_BOUND_REL, DLT_BOUND_ABS = 2.0**-23, 1e-9
H_SCALE = (torch.tensor([[0.7, 0.1, -5], [-0.1, 0.65, 13], [0, 0, 1.0]]),
           torch.tensor([[1.5, 0.2, 21], [-0.3, 1.6, 33], [0, 0, 1.0]]))


def warp32(kp, H):
    """float32 points [..., K, 2] through H [..., 3, 3], divisor w + 1e-5 (only used to BUILD inputs)."""
    h = torch.cat([kp, torch.ones_like(kp[..., :1])], -1) @ H.transpose(-1, -2)
    return h[..., :2] / (h[..., 2:] + 1e-5)


def metric_case(seed, b, m, n):
    """b pairs of m x n key points, continuous uniform in 640 x 480, a random mild homography per pair,
    kp1[perm[:k]] = warp(kp0[:k]) + 1.2 px noise (k = min(m, n)), every 7th match removed, every 11th shifted to a wrong
    index.  -> {"H" [b,3,3], "kp0" [b,m,2], "kp1" [b,n,2], "m0" [b,m]}"""
    g = torch.Generator().manual_seed(seed)
    k = min(m, n)
    H = torch.eye(3)[None].repeat(b, 1, 1)
    H[:, :2, :2] += 0.1 * torch.randn((b, 2, 2), generator=g)
    H[:, :2, 2] = 20 * torch.randn((b, 2), generator=g)
    H[:, 2, :2] = 1e-4 * torch.randn((b, 2), generator=g)
    kp0 = torch.rand((b, m, 2), generator=g) * SIZE
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(b)])
    kp1 = torch.rand((b, n, 2), generator=g) * SIZE
    proj = warp32(kp0, H) + 1.2 * torch.randn((b, m, 2), generator=g)
    m0 = torch.full((b, m), -1, dtype=torch.long)
    for i in range(b):
        kp1[i, perm[i, :k]] = proj[i, :k]
        m0[i, :k] = perm[i, :k]
    m0[:, ::7] = -1
    m0[:, 1::11] = torch.where(m0[:, 1::11] > -1, (m0[:, 1::11] + 1) % n, m0[:, 1::11])
    return {"H": H, "kp0": kp0, "kp1": kp1, "m0": m0}


def _dlt_item(seed, noise, H=None, n_pts=300, keep=None):
    g = torch.Generator().manual_seed(seed)
    if H is None:
        H = torch.eye(3)
        H[:2, :2] += 0.1 * torch.randn((2, 2), generator=g)
        H[:2, 2] = 20 * torch.randn(2, generator=g)
        H[2, :2] = 1e-4 * torch.randn(2, generator=g)
    kp0 = torch.rand((n_pts, 2), generator=g) * SIZE
    h = torch.cat([kp0, torch.ones(n_pts, 1)], -1).double() @ H.double().T
    kp1_all = (h[:, :2] / h[:, 2:]).float() + noise * torch.randn((n_pts, 2), generator=g)
    perm = torch.randperm(n_pts, generator=g)
    kp1 = kp1_all[perm]          # shuffled: the matches are a real permutation
    m0 = torch.argsort(perm)     # kp1[m0[i]] is the partner of kp0[i]
    if keep is not None:
        m0[keep:] = -1
    scores = torch.rand(n_pts, generator=g) * 0.9 + 0.1
    return {"H": H, "kp0": kp0, "kp1": kp1, "m0": m0, "scores": scores}


def dlt_cases():
    """name -> list of items (one batch per name, B > 1, different data per item), 300 x 300 key points each."""
    cases = {"noise0": [_dlt_item(11, 0.0), _dlt_item(12, 0.0)],
             "noise07": [_dlt_item(13, 0.7), _dlt_item(14, 0.7), _dlt_item(15, 0.7)],
             "noise2": [_dlt_item(16, 2.0), _dlt_item(17, 2.0)],
             "scale": [_dlt_item(18, 0.0, H=H_SCALE[0]), _dlt_item(19, 0.0, H=H_SCALE[1])],
             "four": [_dlt_item(20, 0.0, keep=4), _dlt_item(21, 0.0, keep=4)],
             "three": [_dlt_item(22, 0.0, keep=3), _dlt_item(23, 0.5, keep=3)]}
    out = [_dlt_item(24, 0.7), _dlt_item(25, 0.7)]
    for item in out:  # indices N and N + 5 mixed in: such matches are skipped
        n = item["kp1"].shape[0]
        item["m0"][5::40] = n
        item["m0"][9::50] = n + 5
    cases["out_of_range"] = out
    weighted = [_dlt_item(26, 0.3), _dlt_item(27, 0.3)]
    for s, item in enumerate(weighted):  # 20 % of the matches displaced by 30 px, weight 1e-3; the rest weight near 1
        g = torch.Generator().manual_seed(100 + s)
        n = item["kp0"].shape[0]
        bad = torch.randperm(n, generator=g)[: n // 5]
        ang = torch.rand(len(bad), generator=g) * 6.283185307179586
        item["kp1"][item["m0"][bad]] += 30.0 * torch.stack([ang.cos(), ang.sin()], -1)
        item["scores"] = 0.9 + 0.1 * torch.rand(n, generator=g)
        item["scores"][bad] = 1e-3
    cases["weighted_outliers"] = weighted
    return cases


def degenerate_dlt_batch():
    """All matches at one point (item 0: both images, item 1: image 1 only) and an ordinary item: held to a property."""
    a, b, c = _dlt_item(30, 0.0), _dlt_item(31, 0.0), _dlt_item(32, 0.7)
    a["kp0"][:] = torch.tensor([100.0, 50.0])
    a["kp1"][:] = torch.tensor([120.0, 70.0])
    b["kp1"][:] = torch.tensor([300.0, 200.0])
    return [a, b, c]


def stack(items):
    return {k: torch.stack([it[k] for it in items]) for k in items[0]}
