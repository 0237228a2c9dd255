"""SIFT, host side (no GPU): the float64 restatement of tests/sift_reference.py finds what it must, its restated
post-processing equals what the REFERENCE's own functions produced (tests/golden/sift_post.npz, written by
tests/golden/make_golden_sift.py), the fixtures the GPU tests use keep their decisions away from the rounding noise (the
margin census), and the model is registered with the reference's conf keys.

UNPINNED: nothing here (or anywhere) compares with OpenCV, pycolmap or CudaSift -- they are absent."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_reference as sr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_post.npz")
REFERENCE_KEYS = ["rootsift", "nms_radius", "max_num_keypoints", "backend", "detection_threshold", "edge_threshold",
                  "first_octave", "num_octaves", "init_blur", "filter_kpts_with_wrapper", "filter_with_scale_weighting",
                  "extractor_channel", "filter_with_lowest_scale", "force_num_keypoints", "random_topk",
                  "mask_out_padded_kpts", "filter_specular_keypoints"]


# ------------------------------------------------------------------------------------------------------ registration
def test_the_registry_knows_the_extractor_under_the_reference_names():
    from glue_factory_colon_amd import registry, sift

    for name in ("extractors.sift", "sift", "gluefactory.models.extractors.sift"):
        assert registry.get_model(name) is sift.SIFT
    assert set(REFERENCE_KEYS) <= set(sift.SIFT.default_conf) and sift.SIFT.default_conf["backend"] == "gfc_amd"
    model = sift.SIFT({})
    assert model.conf.max_num_keypoints == 4096 and model.conf.first_octave == -1 and model.conf.rootsift is True


@pytest.mark.parametrize("backend", ["opencv", "pycolmap", "pycolmap_cpu", "pycolmap_cuda", "py_cudasift", "py_CudaSift"])
def test_the_reference_backends_are_refused_by_name(backend):
    from glue_factory_colon_amd import sift

    with pytest.raises(NotImplementedError, match="cv2|pycolmap|cudasift_py"):
        sift.SIFT({"backend": backend})


def test_scoreless_branches_and_unknown_names_are_refused():
    from glue_factory_colon_amd import sift

    with pytest.raises(ValueError, match="Unknown backend"):
        sift.SIFT({"backend": "vlfeat"})
    for key in ("random_topk", "filter_with_lowest_scale"):
        with pytest.raises(NotImplementedError, match="scores"):
            sift.SIFT({key: True})
    with pytest.raises(ValueError, match="extractor_channel"):
        sift.SIFT({"extractor_channel": "alpha"})
    sift.SIFT({"init_blur": 2.0, "filter_kpts_with_wrapper": False})  # accepted and ignored


def test_entry_points_refuse_a_short_workspace_and_unserved_shapes_before_any_launch():
    from glue_factory_colon_amd import _native as nat

    lib = nat.lib()

    def f(n):
        return ctypes.c_void_p(0x1000 * n)  # never dereferenced

    need = lib.gfc_sift_detect_workspace_bytes(2, 100)
    assert need > 0 and lib.gfc_sift_detect(f(1), 2, 64, 80, None, -1, 4, 0.0066667, 10.0, 100, f(2), f(3), f(4), f(5),
                                            need - 1, None) == 2
    need = lib.gfc_sift_orient_workspace_bytes(2, 100)
    assert need > 0 and lib.gfc_sift_orient(f(1), 2, 64, 80, None, -1, 4, f(2), f(3), f(4), 100, 200, f(5), f(6), f(7), f(8),
                                            need - 1, None) == 2
    need = lib.gfc_sift_filter_workspace_bytes(2, 64, 80, 200)
    assert need > 0 and lib.gfc_sift_filter(f(1), f(2), f(3), 2, 200, 64, 80, None, None, 0, 0, 50, 1, 50, f(4), f(5), f(6),
                                            f(7), f(8), f(9), f(10), f(11), need - 1, None) == 2
    assert lib.gfc_sift_filter(f(1), f(2), f(3), 2, 200, 64, 80, None, None, 17, 0, 50, 1, 50, f(4), f(5), f(6), f(7), f(8),
                               f(9), f(10), f(11), need, None) == 3  # nms_radius above 16
    need = lib.gfc_sift_extract_workspace_bytes(2, 64, 80, -1, 4, 100, 200)
    assert need > 0 and lib.gfc_sift_extract(f(1), 2, 64, 80, None, None, -1, 4, 0.0066667, 10.0, 100, 200, 0, 0, 50, 1, 50,
                                             f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), f(10), f(11), need - 1, None) == 2
    assert lib.gfc_sift_extract_workspace_bytes(2, 12, 80, 0, 4, 100, 200) == 0
    out = (ctypes.c_int64 * 35)()
    for h, w, fo, no in ((15, 40, 0, 3), (7, 40, -1, 3), (32, 40, -2, 3), (32, 40, 1, 3), (32, 40, 0, 9), (8193, 40, -1, 3)):
        assert lib.gfc_sift_pyramid_layout(h, w, fo, no, out) == 3, (h, w, fo, no)
        assert lib.gfc_sift_pyramid(f(1), 1, h, w, None, fo, no, f(2), f(3), None) == 3
    assert lib.gfc_sift_pyramid_layout(480, 640, -1, 4, out) == 0
    assert list(out[:5]) == [4, 6 * (960 * 1280 + 480 * 640 + 240 * 320 + 120 * 160),
                             5 * (960 * 1280 + 480 * 640 + 240 * 320 + 120 * 160), 960, 1280]
    assert [(o.h, o.w) for o in __import__("glue_factory_colon_amd.sift", fromlist=["x"]).pyramid_layout(67, 93, -1, 8).octaves] \
        == sr.octave_sizes(67, 93, -1, 8)


# ----------------------------------------------------------------------------------------------------- the algorithm
def test_planted_blobs_are_found_at_their_integer_pixel():
    """Gaussians centred on pixel centres, first_octave 0: octave 0 samples the pixels themselves and the integer
    extremum is exact by symmetry; the refined position is the pixel centre (+ 0.5, corner convention)."""
    blobs = [(20, 30, 2.2, 0.3), (41, 57, 3.0, -0.3), (22, 70, 2.6, 0.25), (47, 18, 2.4, -0.35)]  # (sigma >= 2.2: smaller blobs peak below layer 1 of octave 0)
    out = sr.detect([d.astype(np.float32) for d in sr.pyramid(sr.blob_image(64, 96, blobs), 0, 2)["dog"]], 0)
    found = {(int(i[2]), int(i[3])) for i in out["idx"] if i[0] == 0}
    for y, x, _, _ in blobs:
        assert (y, x) in found, (y, x)
        j = [k for k, i in enumerate(out["idx"]) if i[0] == 0 and (i[2], i[3]) == (y, x)][0]
        assert abs(out["raw"][j][0] - (x + 0.5)) < 1e-3 and abs(out["raw"][j][1] - (y + 0.5)) < 1e-3
        assert 0.8 * blobs[0][2] < out["raw"][j][2] < 1.6 * blobs[1][2]  # sigma of the order of the blob's


def test_a_constant_region_yields_no_key_point():
    assert len(sr.extract(np.full((48, 64), 0.37), -1, 3)["oris"]) == 0
    img = sr.textured_image(120, 160, 3)
    out = sr.extract(img, -1, 4)
    assert len(out["oris"]) > 20
    black = img == 0
    assert black.mean() > 0.02
    for x, y in out["keypoints"]:
        yy, xx = int(round(y - 0.5)), int(round(x - 0.5))
        assert not black[max(yy - 4, 0): yy + 5, max(xx - 4, 0): xx + 5].all()
    # an exactly constant DoG is all ties: no candidate, whatever the threshold
    for value in (0.0, 0.01):
        assert sr.detect([np.full((5, 16, 16), value)], 0, detection_threshold=0.0)["n_candidates"] == 0


def test_orientations_and_descriptor_of_a_ramp():
    """A linear ramp whose gradient points at 5 degrees (the centre of bin 0; a ramp at 0 degrees sits on the border of
    two bins and ties): one orientation, that angle; likewise at 95 degrees.  The descriptor of a ramp along +x is unit
    length and all its mass is in the bin of the ramp's direction."""
    ys, xs = np.mgrid[0:48, 0:64].astype(np.float64)
    for deg in (5.0, 95.0, 185.0):
        a = np.deg2rad(deg)
        angles, _ = sr.orientations(0.01 * (xs * np.cos(a) + ys * np.sin(a)), 30.3, 22.6, 2.0)
        want = a if a <= np.pi else a - 2 * np.pi
        assert len(angles) == 1 and abs(angles[0] - want) < 1e-9, (deg, angles)
    assert sr.orientations(0.01 * xs, 30.3, 22.6, 2.0)[0] == []  # the tie
    d = sr.descriptor(0.01 * xs, 30.3, 22.6, 2.0, 0.0)
    assert abs(np.linalg.norm(d) - 1) < 1e-12 and d.reshape(16, 8)[:, 1:].max() < 1e-12
    d90 = sr.descriptor(0.01 * xs, 30.3, 22.6, 2.0, np.pi / 2)  # the window turned by 90 degrees sees the ramp at -90
    assert d90.reshape(16, 8)[:, 6].sum() > 0.99 * d90.sum()


# --------------------------------------------------------------------------------------------------- post-processing
def test_restated_post_processing_equals_the_reference_vectors():
    z = np.load(GOLDEN)
    pts, sc, scale, ang = z["points"], z["scores"], z["scales"], z["angles"]
    shape = tuple(z["shape"])
    for r in (0, 3):
        assert np.array_equal(np.sort(sr.filter_dog_point(pts, scale, ang, shape, r, sc)), z[f"keep_r{r}"])
        assert np.array_equal(np.sort(sr.filter_dog_point(pts, scale, ang, shape, r, None)), z[f"keep_r{r}_noscores"])
    assert len(z["keep_r3"]) < len(z["keep_r0"]) < len(pts)
    assert np.abs(sr.sift_to_rootsift(z["desc"]) - z["rootsift"]).max() < 1e-6
    keep = sr.specular_keep(pts, z["mask"])
    assert np.array_equal(np.nonzero(keep)[0], z["specular_keep"]) and 0 < keep.sum() < len(pts)
    k0 = z["keep_r0"]
    k = int(z["k"])
    assert np.array_equal(k0[sr.topk_indices(sc[k0], k)], z["topk_score"])
    assert np.array_equal(k0[sr.topk_indices(sc[k0], k, scale[k0])], z["topk_score_scale"])
    assert not np.array_equal(z["topk_score"], z["topk_score_scale"])
    ranked = np.sort(sc[k0])[::-1]
    assert ranked[k - 1] > ranked[k]  # no tie at the boundary
    # padding: zeros behind the k kept rows; RootSIFT of a padded (zero) row is the constant sqrt(1 / 128)
    sel = z["topk_score_order"]
    assert np.array_equal(z["padded_scores"][:k], sc[sel]) and not z["padded_scores"][k:].any()
    assert not z["padded_desc"][k:].any() and z["padded_valid"].sum() == k
    assert np.abs(z["padded_rootsift"][k:] - np.sqrt(1 / 128)).max() < 1e-6
    assert np.abs(sr.sift_to_rootsift(z["padded_desc"]) - z["padded_rootsift"]).max() < 1e-6


# ------------------------------------------------------------------------------------------------- the margin census
def test_margin_census_of_the_stage_isolated_fixtures():
    """Every recorded margin of the detection fixture exceeds 1e-6 relative, and every fate of a candidate occurs; the
    orientation fixture has no peak decision closer than 1e-4 (none is excused on the GPU)."""
    vol, planted = sr.detect_fixture()
    out = sr.detect([vol], 0, sr.DETECT_THR)
    assert out["margin"].min() > 1e-6 and (len(out["near_misses"]) == 0 or out["near_misses"].min() > 1e-6)
    f = out["fates"]
    assert f["moved"] >= 1 and f["left_margin"] >= 1 and f["not_converged"] >= 1 and f["low_contrast"] >= 3 and f["edge"] >= 1
    assert out["n_candidates"] > 100
    ids = {tuple(int(v) for v in i[1:]) for i in out["idx"]}
    for name, want in (("under_0.8_thr", False), ("over_0.8_thr", False), ("under_thr", False), ("over_thr", True),
                       ("negative", True), ("tie", False), ("tie_twin", False), ("ridge", False), ("on_margin", True)):
        assert (planted[name] in ids) == want, name
    levels, rec = sr.stage_fixture()
    assert len(rec) % 4 != 0
    margins = [sr.orientations(levels[int(r[3])][int(r[4])], r[0], r[1], r[2])[1] for r in rec]
    assert min(margins) > 1e-4


def test_margin_census_of_the_end_to_end_fixture():
    """At most 2 % of the key points of the end-to-end fixture have a decision inside twice the pyramid chain bound of the
    sample that decides (the worst-case fp32 bound: the kernels' measured error is a tenth of it)."""
    img, fo, no = sr.e2e_fixture()
    out = sr.extract(img, fo, no)
    n = len(out["det"]["raw"])
    assert n >= 50 and out["det"]["risky"].sum() <= 0.02 * n
    assert (out["ori_margin"] < 1e-4).sum() <= 0.01 * len(out["oris"])
