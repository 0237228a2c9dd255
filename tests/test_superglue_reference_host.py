"""SuperGlue, host side (no GPU): the torch restatement (tests/superglue_reference.py) against the vectors the
reference class itself produced (tests/golden/superglue.npz, superglue_1024.npz: make_golden_superglue.py), the
conditions that make the GPU comparison strict, and the module contract of glue_factory_colon_amd.superglue.
"""
import ctypes
import functools

import pytest
import torch

import superglue_reference as sgr
from glue_factory_colon_amd import _native as nat
from glue_factory_colon_amd import registry, superglue, weights

THRESHOLD = 0.2


@functools.lru_cache(maxsize=None)
def restated(shape):
    b, m, n, iters = shape
    inp = sgr.make_inputs(0, b, m, n)
    with torch.no_grad():
        return inp, sgr.forward(weights.superglue_state_dict(0), inp, iters, THRESHOLD)


def close(a, ref, tol=1e-5):
    return bool(((a.double() - ref.double()).abs() <= tol * (1 + ref.double().abs())).all())


@pytest.mark.parametrize("shape", sgr.SHAPES, ids=lambda s: f"{s[1]}x{s[2]}")
def test_restatement_reproduces_the_reference_vectors(golden, shape):
    b, m, n, _ = shape
    fx = golden("superglue_1024" if m >= 1024 else "superglue")
    assert int(fx["seed"]) == 0
    tag = f"{m}x{n}"
    _, out = restated(shape)
    for k in ("matches0", "matches1"):
        assert torch.equal(out[k], fx[f"{tag}/{k}"]), k
    for k in ("matching_scores0", "matching_scores1"):
        assert close(out[k], fx[f"{tag}/{k}"]), k
    la = out["log_assignment"]
    if m >= 1024:
        assert close(la[:, fx[f"{tag}/rows"]], fx[f"{tag}/la_rows"])
        assert close(la[:, :, fx[f"{tag}/cols"]], fx[f"{tag}/la_cols"])
        assert close(la.sum(2), fx[f"{tag}/la_row_sum"])
        assert close(la.abs().sum(2), fx[f"{tag}/la_row_abs_sum"])
    else:
        assert close(la, fx[f"{tag}/log_assignment"])
        assert close(out["sinkhorn_cost"], fx[f"{tag}/sinkhorn_cost"])
        idx = fx[f"{tag}/tap_rows"]
        for i, t in enumerate(out["taps"]):
            assert close(t[idx], fx[f"{tag}/taps"][i]), f"tap {i}"
    assert float(fx[f"{tag}/ref_fp32_error"]) < 1e-5  # the reference's own fp32 error: what the GPU bound leaves room for


@pytest.mark.parametrize("shape", sgr.SHAPES, ids=lambda s: f"{s[1]}x{s[2]}")
def test_fixture_inputs_make_the_gpu_comparison_strict(shape):
    inp, out = restated(shape)
    c = sgr.conditions(out, inp["gt0"], THRESHOLD)
    print(c)
    assert c["found"] == c["planted"] > 0  # every planted correspondence is found
    assert c["false"] == 0  # no outlier is matched
    assert c["min_threshold_distance"] >= 0.05
    assert c["band_rows"] <= 0.01 * c["rows"] and c["band_cols"] <= 0.01 * c["cols"]


def test_float64_restatement_is_within_the_reference_fp32_error_of_the_fixture(golden):
    b, m, n, iters = sgr.SHAPES[1]
    inp, _ = restated(sgr.SHAPES[1])
    with torch.no_grad():
        out = sgr.forward(weights.superglue_state_dict(0), inp, iters, THRESHOLD, dtype=torch.float64)
    assert close(out["log_assignment"], golden("superglue")[f"{m}x{n}/log_assignment"], 2e-5)


def test_state_dict_layout_registry_and_weights_rule():
    model = superglue.SuperGlue({"weights": None})
    sd = weights.superglue_state_dict(0)
    model.load_state_dict(sd, strict=True)
    assert set(model.state_dict()) == set(sd)
    for key in ("kenc.encoder.0.weight", "kenc.encoder.1.running_var", "kenc.encoder.12.bias",
                "gnn.layers.17.attn.proj.2.weight", "gnn.layers.0.attn.merge.bias", "gnn.layers.3.mlp.1.running_mean",
                "gnn.layers.3.mlp.3.weight", "final_proj.weight", "bin_score"):
        assert key in sd, key
    assert sd["kenc.encoder.0.weight"].shape == (32, 3, 1) and sd["gnn.layers.0.mlp.0.weight"].shape == (512, 512, 1)
    for name in ("gluefactory_nonfree.superglue", "superglue"):
        assert registry.get_model(name) is superglue.SuperGlue
    assert superglue.SuperGlue.default_conf["weights"] == "outdoor"
    for w in ("outdoor", "indoor", "/no/such/checkpoint.pth"):
        with pytest.raises(FileNotFoundError, match="no download"):
            superglue.SuperGlue({"weights": w})
    assert superglue.SuperGlue({"weights": "synthetic:3"}).is_initialized()
    two = superglue.SuperGlue({"weights": "synthetic", "use_scores": False, "GNN_layers": ["self", "cross"]})
    assert two.kenc.encoder[0].weight.shape == (32, 2, 1) and len(two.gnn.layers) == 2
    for bad in ({"descriptor_dim": 128}, {"keypoint_encoder": [32, 64, 128]}, {"GNN_layers": ["self", "other"]}):
        with pytest.raises(NotImplementedError):
            superglue.SuperGlue({"weights": None, **bad})
    with pytest.raises(NotImplementedError):
        model.loss({}, {})


def test_head_major_permutation_and_batchnorm_fold():
    """Packed channel h * 64 + d reads the reference's channel d * 4 + h; the fold is y * scale + shift of eval BN."""
    src = superglue.head_major_index()
    assert src[:3].tolist() == [0, 4, 8] and src[64:67].tolist() == [1, 5, 9] and sorted(src.tolist()) == list(range(256))
    x = torch.randn(7, 256, 5, generator=torch.Generator().manual_seed(0))
    assert torch.equal(x.view(7, 64, 4, 5).permute(0, 2, 1, 3).reshape(7, 256, 5), x[:, src])
    bn = torch.nn.BatchNorm1d(16).eval()
    g = torch.Generator().manual_seed(1)
    bn.load_state_dict({"weight": torch.rand(16, generator=g) + 0.5, "bias": torch.randn(16, generator=g),
                        "running_mean": torch.randn(16, generator=g), "running_var": torch.rand(16, generator=g) + 0.3,
                        "num_batches_tracked": torch.tensor(1)})
    y = torch.randn(4, 16, 9, generator=g)
    scale, shift = superglue.fold_bn1d(bn)
    with torch.no_grad():
        assert torch.allclose(bn(y), y * scale[:, None] + shift[:, None], atol=1e-6)


def test_no_keypoints_takes_the_early_return():
    model = superglue.SuperGlue({"weights": "synthetic"}).eval()
    data = sgr.as_data(sgr.make_inputs(0, 1, 5, 7))
    data["keypoints1"] = data["keypoints1"][:, :0]
    out = model(data)
    assert sorted(out) == ["matches0", "matches1", "matching_scores0", "matching_scores1"]
    assert out["matches0"].dtype == torch.int and out["matches1"].dtype == torch.int
    assert out["matches0"].shape == (1, 5) and out["matches1"].shape == (1, 0)
    assert bool((out["matches0"] == -1).all()) and bool((out["matching_scores0"] == 0).all())


def test_cpu_tensors_are_refused():
    model = superglue.SuperGlue({"weights": "synthetic"}).eval()
    with pytest.raises(nat.NativeError, match="no CPU implementation"):
        model(sgr.as_data(sgr.make_inputs(0, 1, 5, 7)))


# ----------------------------------------------------------------------------------- workspaces, host arithmetic only
def f(n):
    """A non-null, 16-byte aligned host address that is never dereferenced."""
    return ctypes.c_void_p(0x1000 * n)


SG_ARRAYS = ["wqkv", "bqkv", "merge_w", "merge_b", "mlp0_w", "mlp0_b", "mlp_scale", "mlp_shift", "mlp1_w", "mlp1_b"]


def _layer_arrays():
    """The per-layer fields of gfc_sg_params: its arrays of GFC_SG_MAX_LAYERS pointers, as the header declares them."""
    return [name for name, t in nat.SgParams._fields_ if issubclass(t, ctypes.Array) and t._type_ is ctypes.c_void_p
            and t._length_ == nat.GFC_SG_MAX_LAYERS]


def _params():
    assert _layer_arrays() == SG_ARRAYS
    p = nat.SgParams()
    p.n_layers, p.use_scores = 2, 1
    p.cross[1] = 1
    for i in range(5):
        p.kenc_w[i] = p.kenc_b[i] = 0x1000
    for i in range(4):
        p.kenc_scale[i] = p.kenc_shift[i] = 0x1000
    for name in _layer_arrays():
        for i in range(2):
            getattr(p, name)[i] = 0x2000
    p.final_proj_w = p.final_proj_b = 0x3000
    return p


def test_one_byte_short_is_refused_before_any_launch():
    lib, p = nat.lib(), _params()
    b, m, n = 2, 65, 130
    calls = {
        "encoder": (lib.gfc_sg_keypoint_encoder_workspace_bytes(b * m), lambda ws: lib.gfc_sg_keypoint_encoder(
            ctypes.byref(p), f(1), f(2), f(3), b, m, f(4), f(5), ws, None)),
        "sinkhorn": (lib.gfc_sg_sinkhorn_workspace_bytes(b, m, n), lambda ws: lib.gfc_sg_sinkhorn(
            f(1), 1.0, b, m, n, 50, f(2), f(3), ws, None)),
        "forward": (lib.gfc_sg_workspace_bytes(b, m, n), lambda ws: lib.gfc_sg_forward(
            ctypes.byref(p), f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), b, m, n, 50, 0.2, f(9), f(10), f(11), f(12),
            f(13), f(14), None, f(15), ws, None)),
    }
    for name, (need, call) in calls.items():
        assert need > 1, name
        assert call(need - 1) == 2 and call(0) == 2, name  # GFC_ERR_WORKSPACE


def test_workspace_sizes_and_refusals():
    lib = nat.lib()
    assert lib.gfc_sg_keypoint_encoder_workspace_bytes(300) == 300 * 1024
    for args in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert lib.gfc_sg_workspace_bytes(*args) == 0 and lib.gfc_sg_sinkhorn_workspace_bytes(*args) == 0
    assert lib.gfc_sg_workspace_bytes(1, 2796202, 1) == 0  # row offsets x 768 columns leave int arithmetic
    # one row of N + 1 floats and v must fit in 160 KB of LDS
    assert lib.gfc_sg_sinkhorn_workspace_bytes(1, 4, 20000) > 0 and lib.gfc_sg_sinkhorn_workspace_bytes(1, 4, 20480) == 0
    assert lib.gfc_sg_sinkhorn(f(1), 1.0, 1, 4, 20480, 1, f(2), f(3), 1 << 30, None) == 3  # GFC_ERR_UNSUPPORTED
    # u [B,M+1] | v [B,N+1] | partials [B, blocks, N+1][max, sum], 256-byte slots; M = 1024: 61 blocks of 17 rows
    def slot(nbytes):
        return (nbytes + 255) // 256 * 256

    for b in (1, 32):  # the block size does not depend on the batch
        need = lib.gfc_sg_sinkhorn_workspace_bytes(b, 1024, 1024)
        assert need == 2 * slot(b * 1025 * 4) + slot(b * 61 * 1025 * 8)
    assert lib.gfc_sg_workspace_bytes(2, 65, 130) > lib.gfc_sg_sinkhorn_workspace_bytes(2, 65, 130) + 390 * 1536 * 4
