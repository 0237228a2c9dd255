"""CPU checks of the sparse-map labels: the restatement tests/sparse_map_reference.py against the reference's vectors
(tests/golden/sparse_map.npz), the wrong rules the fixture rejects, the third header and its binding, the workspace
account, the registry and the refusals of the two matchers."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_map_reference as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((3.0, 5.0, None, False), (None, 10.0, None, True), (3.0, 5.0, 5.0, True), (None, None, None, True),
            (6.0, 5.0, None, True))


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "sparse_map.npz"))


def restate(z, c, s, sparse, rule=None):
    pos, neg, epi, use = SETTINGS[s]
    t = lambda k: torch.from_numpy(z[f"c{c}_{k}"])  # noqa: E731
    tag = f"c{c}_{'s' if sparse else 'd'}{s}_"
    ids = (t("ids0"), t("ids1"), t("v3d0"), t("v3d1")) if (use and sparse) else (None,) * 4
    return tag, sr.sparse_map_labels(
        t("kp0").double(), t("kp1").double(), t("proj_0to1_f64"), t("proj_1to0_f64"), torch.from_numpy(z[tag + "visible0"]),
        torch.from_numpy(z[tag + "visible1"]), t("valid0"), t("valid1"), *ids, F=t("F_f64"), pos_th=pos, neg_th=neg,
        epi_th=epi, rule=rule)


def differs(z, tag, r):
    m, n = r["assignment"].shape
    want = np.unpackbits(z[tag + "assignment"])[:m * n].reshape(m, n).astype(bool)
    keys = ("matches0", "matches1") + tuple(k + q for k in sr.MASK_KEYS for q in "01")
    return any(not np.array_equal(r[k].numpy(), z[tag + k]) for k in keys) or \
        not np.array_equal(r["assignment"].numpy(), want) or \
        not np.array_equal(r["reward"].numpy(), z[tag + "reward"].astype(np.float64))


@pytest.mark.parametrize("c", range(5))
def test_restatement_equals_the_vectors_and_nothing_is_undecided(z, c):
    assert [tuple(v) for v in z["settings"]] == [tuple(-1.0 if v is None else float(v) for v in s) for s in SETTINGS]
    for s in range(len(SETTINGS)):
        for sparse in (True, False):
            tag, r = restate(z, c, s, sparse)
            assert not differs(z, tag, r), tag
            assert not r["undecided0"].any() and not r["undecided1"].any() and not r["undecided_dense"].any(), tag
            assert r["extra_positives"] == r["extra_positives_dense"], tag
            m, n = r["assignment"].shape
            assert z[tag + "matches0"].shape == (m,) and z[f"c{c}_kp1"].shape == (n, 2)
    assert [z[f"c{c}_kp0"].shape[0] for c in range(5)] == [257, 257, 257, 65, 1]
    assert [z[f"c{c}_kp1"].shape[0] for c in range(5)] == [130, 130, 130, 1, 65]


def test_the_fixture_holds_what_the_issue_of_precedence_needs(z):
    """Duplicate ids (several positives in a row), ids without valid_3D, positives that stay under neg_th < pos_th."""
    tag, r = restate(z, 0, 2, True)
    assert int(r["assignment"].sum(1).max()) >= 2 and r["extra_positives"] >= 4
    ids0, ids1 = torch.from_numpy(z["c0_ids0"]), torch.from_numpy(z["c0_ids1"])
    same = ids0[:, None] == ids1[None]
    assert int(same.sum()) > int(torch.from_numpy(z["c0_s2_mask_pos_3d_map0"]).sum())  # some ids are not valid 3D points
    tag, r = restate(z, 0, 4, True)
    assert bool((r["mask_neg_reproj0"] & (r["matches0"] > -1)).any())  # negative AND positive: the positive stays


@pytest.mark.parametrize("rule", sr.WRONG_RULES)
def test_wrong_rules_are_rejected(z, rule):
    rejected = [tag for c in range(3) for s in range(len(SETTINGS)) for tag, r in [restate(z, c, s, True, rule)]
                if differs(z, tag, r)]
    print(rule, "rejected by", rejected)
    if rule == "last_index_ties":  # the geometry has no exact ties: the duplicate ids are what tells the index rule
        assert rejected and all(SETTINGS[int(t.split("_")[1][1:])][3] for t in rejected)
    else:
        assert rejected


def test_header_is_parsed_and_exported():
    from glue_factory_colon_amd import _native as nat

    assert sorted(nat.SPARSE_MAP_FUNCTIONS) == ["gfc_gt_matches_sparse_map", "gfc_gt_matches_sparse_map_workspace_bytes"]
    assert not set(nat.SPARSE_MAP_FUNCTIONS) & (set(nat.FUNCTIONS) | set(nat.VALIDATION_FUNCTIONS))
    with open(nat.SPARSE_MAP_HEADER_PATH) as f:
        funcs, structs, enums, consts = nat.parse_header(f.read())
    assert funcs == nat.SPARSE_MAP_FUNCTIONS and not structs and not enums and not consts
    ret, params = funcs["gfc_gt_matches_sparse_map"]
    assert ret == "int" and len(params) == 30 and params[-1] == ("stream", "void*")
    assert [p for p, _ in params[8:13]] == ["ids0", "ids1", "valid3d0", "valid3d1", "F"]
    assert dict(params)["ids0"] == "const int64_t*" and dict(params)["extra_positives"] == "int32_t*"
    assert funcs["gfc_gt_matches_sparse_map_workspace_bytes"] == ("size_t", [("B", "int"), ("M", "int"), ("N", "int")])
    import ctypes
    res, args = nat.SPARSE_MAP_SIGNATURES["gfc_gt_matches_sparse_map"]
    assert res is ctypes.c_int and args[13:16] == [ctypes.c_int] * 3 and args[16:19] == [ctypes.c_double] * 3
    assert args[-2] is ctypes.c_size_t and args[-1] is ctypes.c_void_p
    lib = nat.lib()
    for name in nat.SPARSE_MAP_FUNCTIONS:
        assert getattr(lib, name).argtypes == nat.SPARSE_MAP_SIGNATURES[name][1]
    with pytest.raises(nat.NativeError, match="takes 29 arguments"):
        nat.convert("gfc_gt_matches_sparse_map", [None] * 5)


def test_workspace_bytes():
    from glue_factory_colon_amd import _native as nat

    f = nat.lib().gfc_gt_matches_sparse_map_workspace_bytes
    assert f(1, 0, 100) == 0 and f(1, 100, 0) == 0 and f(0, 5, 5) == 0 and f(1, -1, 5) == 0 and f(1, 65536, 5) == 0
    last = 0
    for b, m, n in ((1, 1, 1), (1, 16, 17), (1, 257, 130), (1, 2048, 2048), (4, 2048, 2048), (32, 2048, 2048),
                    (32, 4000, 3900), (65535, 65535, 65535)):
        cur = f(b, m, n)
        assert cur >= max(last, 1) and cur >= b * (21 * (m + n) + 4 * m), (b, m, n, cur)  # slots are 256-byte multiples
        last = cur
    assert f(1, 2048, 2048) <= 25 * 4096 + 7 * 256  # about 24 bytes per key point, seven slots rounded up to 256 bytes
    assert f(2, 300, 257) >= f(1, 300, 257) and f(1, 301, 257) >= f(1, 300, 257) and f(1, 300, 258) >= f(1, 300, 257)


def test_registry_conf_and_refusals(caplog):
    from glue_factory_colon_amd import registry
    from glue_factory_colon_amd.sparse_dense_depth_matcher import SparseDenseDepthMatcher
    from glue_factory_colon_amd.sparse_depth_matcher import SparseDepthMatcher

    for name, cls in (("sparse_depth_matcher", SparseDepthMatcher), ("sparse_dense_depth_matcher", SparseDenseDepthMatcher)):
        for alias in ("matchers." + name, name, "gluefactory.models.matchers." + name):
            assert registry.get_model(alias) is cls
    m = SparseDepthMatcher({"use_gt_pos": True, "th_positive": None, "th_negative": 10})  # the Endomapper configuration
    assert m.conf.th_positive is None and m.conf.th_negative == 10 and m.conf.dense_outputs is True
    assert m.conf.th_epi is None and m.conf.save_fig_when_debug is False
    assert {"sparse_depth0", "valid_3D_mask1", "point3D_ids0", "keypoints1", "T_0to1"} <= set(m.required_data_keys)
    d = SparseDenseDepthMatcher({})
    assert d.conf.use_gt_pos_for_plot is False and d.conf.use_gt_pos is False and d.conf.th_positive == 3.0
    assert list(d.required_data_keys) == []
    SparseDepthMatcher({"th_positive": 6.0, "th_negative": 5.0, "dense_outputs": False})  # positives keep precedence
    for cls in (SparseDepthMatcher, SparseDenseDepthMatcher):
        with pytest.raises(NotImplementedError, match="th_consistency"):
            cls({"th_consistency": 3})
        with pytest.raises(ValueError, match="th_epi"):
            cls({"th_epi": -1.0})
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            cls({"save_fig_when_debug": True})
        assert sum("save_fig_when_debug" in r.getMessage() for r in caplog.records) == 1
        with pytest.raises(NotImplementedError):
            cls({}).loss({}, {})
