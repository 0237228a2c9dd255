"""A workspace of exactly the size its `*_workspace_bytes` export names is enough.

Every entry point that carves a caller's workspace runs twice on the same seeded inputs: once with a roomy workspace
(4 x need), once in the first half of a 2 x need buffer filled with 0xA5, told that it has `need` bytes.  The outputs of
the two runs must be equal bit for bit and the second half of the buffer untouched: the guard half is as large as the
workspace itself, so a slot carved from another layout than the one that was sized lands in it and is seen, without a
fault.  Shapes are the smallest that cross the layouts' boundaries: B = 2, M = 65 (two 64-row bands), N = 130, neither
a wave multiple, and a ragged batch with two groups.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from glue_factory_colon_amd import _native as nat  # noqa: E402

DEV = torch.device("cuda", 0)
B, M, N = 2, 65, 130
RAGGED = [(65, 130), (65, 130), (40, 17)]
GUARD = 0xA5


def st():
    return nat.stream_ptr(DEV)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def P(t):
    return nat.ptr(t)


def _exact(need, run):
    """run(ws, ws_bytes) -> output tensors (fresh ones per call).  See the module docstring."""
    need = int(need)
    assert need > 0
    roomy = torch.full((4 * need,), 0x11, dtype=torch.uint8, device=DEV)
    want = run(roomy, roomy.numel())
    buf = torch.full((2 * need,), GUARD, dtype=torch.uint8, device=DEV)
    got = run(buf, need)
    torch.cuda.synchronize()
    assert len(want) == len(got) and len(got) > 0
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"output {i} differs"
    assert bool((buf[need:] == GUARD).all()), "wrote behind the workspace"


# ------------------------------------------------------------------------------------------------ LightGlue
_MODELS = {}


def _lg(prec):
    """(module, gfc_lg_params) of a 2-layer synthetic matcher."""
    if prec not in _MODELS:
        from glue_factory_colon_amd import lightglue

        m = lightglue.LightGlue({"weights": "synthetic", "filter_threshold": 0.1, "n_layers": 2,
                                 "matmul_precision": prec}).eval().to(DEV)
        _MODELS[prec] = (m, m.ensure_packed(DEV)[0])
    return _MODELS[prec]


def _desc(rows, g, dim=256):
    return F.normalize(torch.randn((rows, dim), generator=g), dim=-1)


def _match_outputs(shapes):
    sm, sn = sum(m for m, _ in shapes), sum(n for _, n in shapes)
    return [torch.full((sm,), -7, dtype=torch.long, device=DEV), torch.full((sn,), -7, dtype=torch.long, device=DEV),
            torch.zeros((sm,), device=DEV), torch.zeros((sn,), device=DEV),
            torch.zeros((sum((m + 1) * (n + 1) for m, n in shapes),), device=DEV)]


def _case_lg_layer(prec):
    lib, (_, params) = nat.lib(), _lg(prec)
    g = gen(11)
    rows = B * (M + N)
    x0 = _desc(rows, g).to(DEV)
    ang = torch.randn((rows, 32), generator=g).repeat_interleave(2, 1)
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    r1 = B * M  # rows: side 0 of every pair, then side 1
    self_p = [[b * M, M, b * M, M] for b in range(B)] + [[r1 + b * N, N, r1 + b * N, N] for b in range(B)]
    cross_p = [[b * M, M, r1 + b * N, N] for b in range(B)] + [[r1 + b * N, N, b * M, M] for b in range(B)]
    sp = torch.tensor(self_p, dtype=torch.int32, device=DEV)
    cp = torch.tensor(cross_p, dtype=torch.int32, device=DEV)

    def run(ws, nbytes):
        x = x0.clone()
        for layer in range(2):
            nat.check(lib.gfc_lg_layer(ctypes.byref(params), layer, P(x), P(cos), P(sin), rows, P(sp), P(cp), 2 * B, N,
                                       P(ws), nbytes, st()), "gfc_lg_layer")
        return [x]

    return lib.gfc_lg_layer_workspace_bytes(rows), run


def _case_lg_assign(prec):
    lib, (_, params) = nat.lib(), _lg(prec)
    g = gen(12)
    x0, x1 = _desc(B * M, g).to(DEV), _desc(B * N, g).to(DEV)

    def run(ws, nbytes):
        o = _match_outputs([(M, N)] * B)
        nat.check(lib.gfc_lg_assign(ctypes.byref(params), 1, P(x0), P(x1), B, M, N, 0.1, P(o[0]), P(o[1]), P(o[2]), P(o[3]),
                                    P(o[4]), P(ws), nbytes, st()), "gfc_lg_assign")
        return o

    return lib.gfc_lg_assign_workspace_bytes(B, M, N), run


def _lg_inputs(shapes, seed):
    """Rows group after group (here: in the order given, equal shapes adjacent), side 0 then side 1 inside a group."""
    g = gen(seed)
    groups = []
    for s in shapes:
        if groups and groups[-1][0] == s:
            groups[-1][1] += 1
        else:
            groups.append([s, 1])
    kp, de = [], []
    for (m, n), cnt in groups:
        for k in (m, n):
            kp.append(torch.rand((cnt * k, 2), generator=g) * torch.tensor([640.0, 480.0]))
            de.append(_desc(cnt * k, g))
    size = torch.tensor([[640.0, 480.0]] * len(shapes), device=DEV)
    return torch.cat(kp).to(DEV), torch.cat(de).to(DEV), size


def _case_lg_forward(prec):
    lib, (_, params) = nat.lib(), _lg(prec)
    kp, de, size = _lg_inputs([(M, N)] * B, 13)
    k0, k1 = kp[:B * M].clone(), kp[B * M:].clone()
    d0 = de[:B * M].clone()
    apart = torch.zeros(12345, device=DEV)  # keeps the two descriptor arrays apart in memory
    d1 = de[B * M:].clone()
    assert d1.data_ptr() != d0.data_ptr() + d0.numel() * 4 and apart.numel()

    def run(ws, nbytes):
        o = _match_outputs([(M, N)] * B)
        r0, r1 = torch.zeros((B * M, 256), device=DEV), torch.zeros((B * N, 256), device=DEV)
        nat.check(lib.gfc_lg_forward(ctypes.byref(params), P(k0), P(k1), P(d0), P(d1), P(size), P(size), None, None, B, M,
                                     N, 0.1, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(r0), P(r1), P(ws), nbytes,
                                     st()), "gfc_lg_forward")
        return o + [r0, r1]

    return lib.gfc_lg_workspace_bytes(B, M, N), run


def _case_lg_forward_packed(prec):
    lib, (_, params) = nat.lib(), _lg(prec)
    kp, de, size = _lg_inputs([(M, N)] * B, 14)

    def run(ws, nbytes):
        o = _match_outputs([(M, N)] * B)
        rows = torch.zeros((B * (M + N), 256), device=DEV)
        nat.check(lib.gfc_lg_forward_packed(ctypes.byref(params), P(kp), P(de), P(size), P(size), None, B, M, N, 0.1,
                                            P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(rows), P(ws), nbytes, None,
                                            st()), "gfc_lg_forward_packed")
        return o + [rows]

    return lib.gfc_lg_packed_workspace_bytes(B, M, N), run


def _case_lg_forward_ragged(prec):
    lib, (_, params) = nat.lib(), _lg(prec)
    kp, de, size = _lg_inputs(RAGGED, 15)
    b = len(RAGGED)
    cm, cn = (ctypes.c_int32 * b)(*[m for m, _ in RAGGED]), (ctypes.c_int32 * b)(*[n for _, n in RAGGED])

    def run(ws, nbytes):
        o = _match_outputs(RAGGED)
        rows = torch.zeros((kp.shape[0], 256), device=DEV)
        nat.check(lib.gfc_lg_forward_ragged(ctypes.byref(params), P(kp), P(de), P(size), P(size), None, b, cm, cn, 0.1,
                                            P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(rows), P(ws), nbytes, None,
                                            st()), "gfc_lg_forward_ragged")
        return o + [rows]

    return lib.gfc_lg_ragged_workspace_bytes(b, cm, cn), run


# ------------------------------------------------------------------------------------------------ attention
def _case_attention(prec):
    """2 problems x 70 queries x 4 heads: 8 workgroups of 128 queries, the full 8-way key split."""
    lib = nat.lib()
    g = gen(21)
    nq, heads, probs = 70, 4, 2
    dt = torch.float32 if prec == "fp32" else torch.float16
    q, k, v = (torch.randn((probs * nq, 256), generator=g).to(DEV, dt) for _ in range(3))
    pt = torch.tensor([[p * nq, nq, p * nq, nq] for p in range(probs)], dtype=torch.int32, device=DEV)
    fn = lib.gfc_attention if prec == "fp32" else lib.gfc_attention_f16

    def run(ws, nbytes):
        o = torch.zeros((probs * nq, 256), device=DEV, dtype=dt)
        nat.check(fn(P(q), 256, P(k), 256, P(v), 256, P(o), 256, P(pt), probs, nq, heads, 0.125, P(ws), nbytes, st()),
                  "attention")
        return [o]

    need = lib.gfc_attention_workspace_bytes(probs, nq, heads)
    assert need == (probs * nq * heads * 8 * 66 * 4 + 255) // 256 * 256  # nothing smaller holds the 8-way split
    return need, run


# ------------------------------------------------------------------------------------------------ assignment stages
def _case_nn_match(_):
    lib = nat.lib()
    g = gen(31)
    d = 64
    d0, d1 = _desc(B * M, g, d).to(DEV), _desc(B * N, g, d).to(DEV)

    def run(ws, nbytes):
        o = _match_outputs([(M, N)] * B)
        sim = torch.zeros((B, M, N), device=DEV)
        nat.check(lib.gfc_nn_match(P(d0), P(d1), B, M, N, d, 0.9, 1.2, 1, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(sim), P(o[4]),
                                   P(ws), nbytes, st()), "gfc_nn_match")
        return o + [sim]

    return lib.gfc_nn_workspace_bytes(B, M, N), run


def _case_log_assignment(_):
    lib = nat.lib()
    g = gen(32)
    sim = torch.randn((B, M, N), generator=g).to(DEV)
    z0, z1 = torch.randn((B, M), generator=g).to(DEV), torch.randn((B, N), generator=g).to(DEV)

    def run(ws, nbytes):
        out = torch.zeros((B, M + 1, N + 1), device=DEV)
        nat.check(lib.gfc_lg_log_assignment(P(sim), P(z0), P(z1), B, M, N, P(out), P(ws), nbytes, st()), "log_assignment")
        return [out]

    return 2 * B * (M + N) * 4, run  # include/gfc_amd.h


def _case_filter_matches(_):
    lib = nat.lib()
    g = gen(33)
    scores = (torch.randn((B, M + 1, N + 1), generator=g) - 1.0).to(DEV)

    def run(ws, nbytes):
        o = _match_outputs([(M, N)] * B)[:4]
        nat.check(lib.gfc_lg_filter_matches(P(scores), B, M, N, 0.1, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(ws), nbytes,
                                            st()), "filter_matches")
        return o

    return B * (M + N) * 8, run  # include/gfc_amd.h


def _case_adaptive_step(_):
    """Two pairs, (200, 131) and (77, 260) rows, random heads, stop and prune decisions both on."""
    lib = nat.lib()
    g = gen(34)
    shapes = ((200, 131), (77, 260))
    nb = len(shapes)
    seg, pairs, off, r = [], [], [], 0
    for b, (m, n) in enumerate(shapes):
        seg += [[r, m], [r + m, n]]
        off.append([r, r + m])
        pairs.append([m + n, b])
        r += m + n
    rows = r
    ind = torch.cat([torch.arange(k, dtype=torch.int32) for s in shapes for k in s])
    x = torch.randn((rows, 256), generator=g)
    cos, sin = torch.randn((rows, 64), generator=g), torch.randn((rows, 64), generator=g)
    heads = [torch.randn(256, generator=g) / 16, torch.tensor([0.1]), torch.randn(256, generator=g) / 16,
             torch.tensor([-0.2])]
    keep = [t.to(DEV).contiguous() for t in (x, cos, sin, ind, torch.tensor(seg, dtype=torch.int32),
                                             torch.tensor(pairs, dtype=torch.int32),
                                             torch.tensor(off, dtype=torch.int32), *heads)]
    dx, dcos, dsin, dind, dseg, dpairs, doff, tw, tb, mw, mb = keep
    p = nat.LgParams()
    p.n_layers, layer = 9, 3
    p.token_w[layer], p.token_b[layer] = tw.data_ptr(), tb.data_ptr()
    p.matchability_w[layer], p.matchability_b[layer] = mw.data_ptr(), mb.data_ptr()

    def run(ws, nbytes):
        prune = torch.ones(rows, dtype=torch.int32, device=DEV)
        o = [torch.zeros_like(dx), torch.zeros_like(dcos), torch.zeros_like(dsin), torch.full_like(dind, -7), prune,
             torch.full((2 * nb, 4), -7, dtype=torch.int32, device=DEV),
             torch.full((2 * nb, 4), -7, dtype=torch.int32, device=DEV),
             torch.full((2 * nb, 2), -7, dtype=torch.int32, device=DEV),
             torch.full((nb, 2), -7, dtype=torch.int32, device=DEV), torch.full((nb, 4), -7, dtype=torch.int32, device=DEV)]
        nat.check(lib.gfc_lg_adaptive_step(ctypes.byref(p), layer, P(dx), P(dcos), P(dsin), P(dind), rows, P(dseg), P(dpairs),
                                           P(doff), nb, nb, 260, 0.5, 0.5, 0.95, 1, 1, P(o[0]), P(o[1]), P(o[2]), P(o[3]),
                                           P(prune), rows, P(o[5]), P(o[6]), P(o[7]), P(o[8]), P(o[9]), P(ws), nbytes, st()),
                  "gfc_lg_adaptive_step")
        return o

    return lib.gfc_lg_adaptive_step_workspace_bytes(nb, rows), run


# ------------------------------------------------------------------------------------------------ extractors
def _case_sp_dense(c):
    from glue_factory_colon_amd import superpoint_open, synthetic

    lib = nat.lib()
    m = superpoint_open.SuperPoint({"weights": "synthetic"}).eval().to(DEV)
    packed = m.ensure_packed(DEV)
    b, h, w = 2, 64, 96
    img = synthetic.synthetic_images(b, h, w, seed=41).to(DEV)
    if c == 3:
        img = (img * torch.tensor([0.9, 1.0, 1.1], device=DEV).view(1, 3, 1, 1)).contiguous()
    assert tuple(img.shape) == (b, c, h, w)

    def run(ws, nbytes):
        heat = torch.zeros((b, h, w), device=DEV)
        desc = torch.zeros((b, h // 8, w // 8, packed.desc_dim), device=DEV)
        nat.check(lib.gfc_sp_dense(ctypes.byref(packed.params), P(img), b, c, h, w, P(heat), P(desc), P(ws), nbytes, None,
                                   st()), "gfc_sp_dense")
        return [heat, desc]

    return lib.gfc_sp_workspace_bytes(b, c, h, w), run


def _keypoint_outputs(b, cap):
    return [torch.zeros((b, cap, 2), device=DEV), torch.zeros((b, cap), device=DEV),
            torch.full((b,), -7, dtype=torch.int32, device=DEV)]


def _case_sp_select(fused):
    lib = nat.lib()
    b, h, w, k = 2, 40, 56, 50
    heat = torch.rand((b, h, w), generator=gen(42)).to(DEV)

    def run(ws, nbytes):
        o = _keypoint_outputs(b, k)
        if fused:
            nat.check(lib.gfc_sp_nms_select(P(heat), b, h, w, 3, 0, None, 0.0, k, k, None, P(o[0]), P(o[1]), P(o[2]), P(ws),
                                            nbytes, st()), "gfc_sp_nms_select")
        else:
            nat.check(lib.gfc_sp_select(P(heat), b, h, w, 0.0, k, k, P(o[0]), P(o[1]), P(o[2]), P(ws), nbytes, st()),
                      "gfc_sp_select")
        return o

    need = lib.gfc_sp_nms_select_workspace_bytes(b, h, w) if fused else lib.gfc_sp_select_workspace_bytes(b, h, w)
    return need, run


def _case_disk_nms_select(_):
    lib = nat.lib()
    b, h, w, n = 2, 40, 56, 50
    heat = torch.randn((b, h, w), generator=gen(43)).to(DEV)

    def run(ws, nbytes):
        o = _keypoint_outputs(b, n)
        nat.check(lib.gfc_disk_nms_select(P(heat), b, h, w, 5, 0.0, n, n, P(o[0]), P(o[1]), P(o[2]), P(ws), nbytes, st()),
                  "gfc_disk_nms_select")
        return o

    return lib.gfc_disk_select_workspace_bytes(b, h, w), run


def _case_disk_instnorm(_):
    lib = nat.lib()
    b, h, w, c = 2, 33, 21, 16  # the smallest gated layer of test_conv5x5_vs_torch
    x = (torch.randn((b, h, w, c), generator=gen(44)) * 2 + 0.5).to(DEV)

    def run(ws, nbytes):
        mean, rstd = torch.zeros((b, c), device=DEV), torch.zeros((b, c), device=DEV)
        nat.check(lib.gfc_disk_instnorm_stats(P(x), b, h, w, c, 1e-5, P(mean), P(rstd), P(ws), nbytes, st()), "instnorm")
        return [mean, rstd]

    return lib.gfc_disk_instnorm_workspace_bytes(b, c), run


def _case_ransac(_):
    lib = nat.lib()
    g = gen(45)
    b, m, t, nh = 2, 100, 3, 512
    kp0 = torch.rand((b, m, 2), generator=g) * torch.tensor([640.0, 480.0])
    H = torch.tensor([[1.05, 0.03, 12.0], [-0.02, 0.97, -7.0], [1e-5, -2e-5, 1.0]])
    q = torch.cat([kp0, torch.ones((b, m, 1))], -1) @ H.T
    kp1 = q[..., :2] / q[..., 2:] + 0.3 * torch.randn((b, m, 2), generator=g)
    kp1[:, ::4] = torch.rand((b, (m + 3) // 4, 2), generator=g) * 400  # a quarter of the matches are outliers
    m0 = torch.arange(m).expand(b, m).clone()
    m0[:, 5::17] = -1
    dk0, dk1, dm0 = kp0.to(DEV), kp1.contiguous().to(DEV), m0.to(DEV)
    th = (ctypes.c_float * t)(1.0, 2.0, 4.0)

    def run(ws, nbytes):
        o = [torch.zeros((b, t, 3, 3), device=DEV, dtype=torch.float64), torch.zeros((b, t, m), device=DEV, dtype=torch.uint8),
             torch.zeros((b, t), device=DEV, dtype=torch.int32), torch.zeros((b, t), device=DEV, dtype=torch.uint8),
             torch.zeros((b, t), device=DEV, dtype=torch.int32), torch.zeros((b, t, 3, 3), device=DEV, dtype=torch.float64)]
        nat.check(lib.gfc_eval_homography_ransac(P(dk0), P(dk1), P(dm0), None, None, None, b, m, m, th, t, nh, 3, 7, P(o[0]),
                                                 P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]), None, P(ws), nbytes, st()),
                  "gfc_eval_homography_ransac")
        return o

    return lib.gfc_eval_homography_ransac_workspace_bytes(b, m, t, nh), run


def _case_relpose(_):
    """Two ranges per pair; all six (pair, threshold) blocks succeed, so every block's solve slice of the workspace is
    used (asserted below)."""
    lib = nat.lib()
    g = gen(46)
    b, m, t, nh = 2, 100, 3, 512
    X = torch.rand((b, m, 3), generator=g) * torch.tensor([4.0, 3.0, 4.0]) + torch.tensor([-2.0, -1.5, 4.0])
    ay, ax = torch.tensor(0.12), torch.tensor(-0.05)
    Ry = torch.tensor([[ay.cos(), 0.0, ay.sin()], [0.0, 1.0, 0.0], [-ay.sin(), 0.0, ay.cos()]])
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, ax.cos(), -ax.sin()], [0.0, ax.sin(), ax.cos()]])
    Y = X @ (Ry @ Rx).T + torch.tensor([0.6, 0.1, 0.05])
    f, c = 500.0, torch.tensor([320.0, 240.0])
    kp0 = f * X[..., :2] / X[..., 2:] + c
    kp1 = f * Y[..., :2] / Y[..., 2:] + c + 0.3 * torch.randn((b, m, 2), generator=g)
    kp1[:, ::4] = torch.rand((b, (m + 3) // 4, 2), generator=g) * 400  # a quarter of the matches are outliers
    m0 = torch.arange(m).expand(b, m).clone()
    m0[:, 5::17] = -1
    cam = torch.tensor([[640.0, 480.0, f, f, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0]] * b)  # PINHOLE (model 0)
    dk0, dk1, dm0, dcam = kp0.contiguous().to(DEV), kp1.contiguous().to(DEV), m0.to(DEV), cam.to(DEV)
    th = (ctypes.c_float * t)(1.0, 2.0, 4.0)

    def run(ws, nbytes):
        f64 = lambda *tail: torch.zeros((b, t, *tail), device=DEV, dtype=torch.float64)  # noqa: E731
        i32 = lambda: torch.zeros((b, t), device=DEV, dtype=torch.int32)  # noqa: E731
        o = [f64(3, 3), f64(3), f64(3, 3), f64(3, 3), torch.zeros((b, t, m), device=DEV, dtype=torch.uint8), i32(),
             torch.zeros((b, t), device=DEV, dtype=torch.uint8), i32(), i32()]
        nat.check(lib.gfc_eval_relative_pose_ransac(P(dk0), P(dk1), P(dm0), None, P(dcam), 0, P(dcam), 0, None, b, m, m, th,
                                                    t, nh, 3, 7, 0.0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]),
                                                    P(o[6]), P(o[7]), P(o[8]), None, None, P(ws), nbytes, st()),
                  "gfc_eval_relative_pose_ransac")
        assert bool(o[6].bool().all()), "a block failed: its solve slice is not exercised"
        return o

    return lib.gfc_eval_relative_pose_ransac_workspace_bytes(b, m, t, nh), run


# ------------------------------------------------------------------------------------------------ SuperGlue
def _sg(names):
    """(module, gfc_sg_params) of a synthetic matcher with the GNN layers `names`: none for the encoder alone (weights of
    test_keypoint_encoder_against_float64), two for the whole forward."""
    key = ("sg", names)
    if key not in _MODELS:
        from glue_factory_colon_amd import superglue, weights

        if names:
            m = superglue.SuperGlue({"weights": "synthetic", "GNN_layers": list(names), "num_sinkhorn_iterations": 20})
        else:
            m = superglue.SuperGlue({"weights": None, "GNN_layers": []})
            m.load_state_dict(weights.superglue_state_dict(5, n_layers=0), strict=True)
        m = m.eval().to(DEV)
        _MODELS[key] = (m, m.ensure_packed(DEV)[0])
    return _MODELS[key]


def _sg_points(rows, g):
    """key points of 640 x 480 images, detection scores, unit descriptors"""
    return (torch.rand((rows, 2), generator=g) * torch.tensor([640.0, 480.0])).to(DEV), \
        torch.rand((rows,), generator=g).to(DEV), _desc(rows, g).to(DEV)


def _case_sg_keypoint_encoder(_):
    """The hidden [rows, 256] activations in front of the last encoder layer are the whole workspace."""
    lib, (_, params) = nat.lib(), _sg(())
    kp, sc, de = _sg_points(B * N, gen(51))
    size = torch.tensor([[640.0, 480.0], [300.0, 500.0]], device=DEV)

    def run(ws, nbytes):
        desc = de.clone()  # in: the descriptors, out: descriptors + encoding
        nat.check(lib.gfc_sg_keypoint_encoder(ctypes.byref(params), P(kp), P(sc), P(size), B, N, P(desc), P(ws), nbytes,
                                              st()), "gfc_sg_keypoint_encoder")
        return [desc]

    return lib.gfc_sg_keypoint_encoder_workspace_bytes(B * N), run


def _case_sg_sinkhorn(_):
    """u | v | the column partials of every row block"""
    lib = nat.lib()
    cost = ((torch.rand((B, M, N), generator=gen(52)) * 2 - 1) * 4.0).to(DEV)

    def run(ws, nbytes):
        out = torch.full((B, M + 1, N + 1), float("nan"), device=DEV)
        nat.check(lib.gfc_sg_sinkhorn(P(cost), 0.7, B, M, N, 20, P(out), P(ws), nbytes, st()), "gfc_sg_sinkhorn")
        return [out]

    return lib.gfc_sg_sinkhorn_workspace_bytes(B, M, N), run


def _case_sg_forward(_):
    """Two layers (self, cross).  The qkv slot holds the encoder's hidden rows, then Q | K | V, then the final_proj
    output; the Sinkhorn and filter workspaces are carved from this one; and M != N, so the attention scratch, sized for
    B (M + N) query slots, is smaller than the 8-way split of the 2 B max(M, N) slots the kernel indexes: gfc_att_split
    shrinks the split (asserted below), and the partials of the split it lands on must fit."""
    lib, (_, params) = nat.lib(), _sg(("self", "cross"))
    g = gen(53)
    k0, s0, d0 = _sg_points(B * M, g)
    k1, s1, d1 = _sg_points(B * N, g)
    size = torch.tensor([[640.0, 480.0]] * B, device=DEV)
    rows, slots = B * (M + N), 2 * B * max(M, N)
    assert slots * 2 <= rows * 8 < slots * 8  # room for a split of at least 2, not for all 8: the shrink loop runs

    def run(ws, nbytes):
        i64 = lambda n: torch.full((B, n), -7, dtype=torch.long, device=DEV)  # noqa: E731
        o = [torch.zeros((B, M, N), device=DEV), torch.zeros((B, M + 1, N + 1), device=DEV), i64(M), i64(N),
             torch.zeros((B, M), device=DEV), torch.zeros((B, N), device=DEV)]
        taps = torch.zeros((4, rows, 256), device=DEV)
        nat.check(lib.gfc_sg_forward(ctypes.byref(params), P(k0), P(k1), P(s0), P(s1), P(d0), P(d1), P(size), P(size), B, M,
                                     N, 20, 0.2, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(taps), P(ws),
                                     nbytes, st()), "gfc_sg_forward")
        return o + list(taps)

    return lib.gfc_sg_workspace_bytes(B, M, N), run


CASES = [(fn, arg) for arg in ("fp32", "fp16")
         for fn in (_case_lg_layer, _case_lg_assign, _case_lg_forward, _case_lg_forward_packed, _case_lg_forward_ragged,
                    _case_attention)]
CASES += [(_case_nn_match, None), (_case_log_assignment, None), (_case_filter_matches, None), (_case_adaptive_step, None),
          (_case_sp_dense, 1), (_case_sp_dense, 3), (_case_sp_select, False), (_case_sp_select, True),
          (_case_disk_nms_select, None), (_case_disk_instnorm, None), (_case_ransac, None),
          (_case_relpose, None), (_case_sg_keypoint_encoder, None), (_case_sg_sinkhorn, None), (_case_sg_forward, None)]


@pytest.mark.parametrize("case,arg", CASES, ids=[f"{fn.__name__[6:]}-{arg}" for fn, arg in CASES])
def test_exact_size_workspace_is_enough(case, arg):
    need, run = case(arg)
    _exact(need, run)
