"""The GPU comparisons of the SIFT kernels with tests/sift_reference.py, as functions that RETURN their figures:
tests/test_gpu_sift.py asserts on them, tools/sift_parity.py records them.  Nothing here asserts a tolerance."""
import numpy as np
import torch

import sift_reference as sr

# "A level narrower than the tap radius" cannot exist: the widest incremental blur has radius 13 (27 taps) and an octave
# exists only while its shorter side is >= 16.  The extreme that does exist is a 16-sample side under 27 taps, where both
# replicate borders fall inside one window: the third case.
PYRAMID_CASES = {
    # name: (H, W, [valid (w, h) per image] or [None])
    "67x93 (no multiple of the 32 x 64 tile)": (67, 93, [None]),
    "2x64x80, differing valid_wh": (64, 80, [(80, 64), (53, 41)]),
    "16x70 (16 samples under 27 taps: both borders inside one window)": (16, 70, [None]),
}


def image(h, w, seed):
    g = np.random.RandomState(seed)
    return (0.6 * sr.textured_image(h, w, seed, n=12, vignette=False) + 0.4 * g.rand(h, w)).astype(np.float32)


def upload(sift, planes, lay, dog):
    """planes: list per octave of (levels, h, w) arrays -> [1, floats] device buffer in the library's layout."""
    buf = torch.zeros(1, lay.dog_floats if dog else lay.gauss_floats)
    for o, p in enumerate(planes):
        for s in range(p.shape[0]):
            sift.level(buf, lay, 0, o, s, dog=dog)[: p.shape[1], : p.shape[2]] = torch.from_numpy(np.asarray(p[s], np.float32))
    return buf.cuda()


def download(sift, buf, lay, b, sizes, dog):
    """The image's own region of every level: list per octave of (levels, h, w) float32 arrays."""
    buf = buf.cpu()
    n = 5 if dog else 6
    return [np.stack([sift.level(buf, lay, b, o, s, dog=dog)[:h, :w].numpy() for s in range(n)]) for o, (h, w) in enumerate(sizes)]


def records(rec, cap):
    raw_f = torch.zeros(1, cap, 8)
    raw_i = torch.zeros(1, cap, 8, dtype=torch.int32)
    n = len(rec)
    raw_f[0, :n, 4:7] = torch.from_numpy(rec[:, :3]).float()
    raw_i[0, :n, 0] = torch.from_numpy(rec[:, 3]).int()
    raw_i[0, :n, 4] = torch.from_numpy(rec[:, 4]).int()
    counts = torch.tensor([[n, n, 0, 0]], dtype=torch.int32)
    return raw_f.cuda(), raw_i.cuda(), counts.cuda()


def pyramid_errors(sift, imgs, valid, first_octave, num_octaves):
    """-> (worst Gaussian error / bound, worst DoG error / bound, octave counts agree) over the images' own regions."""
    b, h, w = imgs.shape
    wh = None if valid == [None] else torch.tensor(valid, dtype=torch.int32)
    gauss, dog, lay = sift.pyramid(torch.from_numpy(imgs).cuda(), wh, first_octave, num_octaves)
    worst_g = worst_d = 0.0
    octaves_ok = True
    for i, v in enumerate(valid):
        vw, vh = v or (w, h)
        ref = sr.pyramid(imgs[i, :vh, :vw], first_octave, num_octaves)
        sizes = [g.shape[1:] for g in ref["gauss"]]
        if (vw, vh) == (w, h):
            octaves_ok = octaves_ok and len(sizes) == len(lay.octaves)
        kg, kd = download(sift, gauss, lay, i, sizes, False), download(sift, dog, lay, i, sizes, True)
        for o in range(len(sizes)):
            for s in range(6):
                worst_g = max(worst_g, np.abs(kg[o][s].astype(np.float64) - ref["gauss"][o][s]).max() / ref["gauss_bound"][o][s])
            worst_d = max(worst_d, (np.abs(kd[o].astype(np.float64) - ref["dog"][o]) / ref["dog_bound"][o]).max())
    return worst_g, worst_d, octaves_ok


def compare_raw(ref, raw_f, raw_i, counts, b=0):
    """-> dict: counts and integer records equal, and the largest relative distance of (x, y, sigma, score, x_oct, y_oct,
    sigma_oct) from the restatement's values ROUNDED TO FP32 (what a correct fp64 result becomes when it is stored)."""
    n = int(counts[b, 0])
    same = n == len(ref["idx"]) and int(counts[b, 1]) == ref["n_candidates"] and int(counts[b, 2]) == 0
    rel = float("inf")
    if same and n:
        got_i = raw_i[b, :n].cpu().numpy()
        same = np.array_equal(got_i[:, :4], ref["idx"]) and np.array_equal(got_i[:, 4:7], ref["pos"])
        want = ref["raw"].astype(np.float32).astype(np.float64)
        rel = float((np.abs(raw_f[b, :n, :7].cpu().double().numpy() - want) / np.abs(want)).max())
    return {"equal": bool(same), "n": n, "rel": rel}


def orientation_and_descriptor(sift, gauss, lay, levels, raw_f, raw_i, counts, h, w, first_octave, num_octaves):
    """Orient and describe on device records against the restatement fed THE SAME fp32 levels and records (the
    descriptor also the kernel's own fp32 angle): the stage tolerances apply as written.  -> figures."""
    n = int(counts[0, 0])
    ori_f, ori_i, ocounts = sift.orient(gauss, h, w, raw_f, raw_i, counts, None, first_octave, num_octaves)
    desc = sift.describe(gauss, h, w, ori_f, ori_i, ocounts, None, first_octave, num_octaves)
    m = int(ocounts[0, 0])
    kr, ki = raw_f[0, :n].cpu().double().numpy(), raw_i[0, :n].cpu().numpy()
    of, oi, dk = ori_f[0, :m].cpu().numpy(), ori_i[0, :m].cpu().numpy(), desc[0, :m].cpu().double().numpy()
    measured_o = kernel_o = measured_d = kernel_d = 0.0
    close_peak, wrong_count, restated = [], [], 0
    for i in range(n):
        lv = levels[int(ki[i, 0])][int(ki[i, 4])]
        a64, margin = sr.orientations(lv, kr[i, 4], kr[i, 5], kr[i, 6])
        a32, _ = sr.orientations(lv, kr[i, 4], kr[i, 5], kr[i, 6], np.float32)
        restated += len(a64)
        rows = np.nonzero(oi[:, 0] == i)[0]
        if margin < 1e-4:
            close_peak.append(i)
        if len(rows) != len(a64):
            wrong_count.append(i)
            continue
        if len(a32) == len(a64):
            measured_o = max([measured_o] + [abs(x - y) for x, y in zip(a64, a32)])
        for j, th in zip(rows, a64):
            d = abs(float(of[j, 7]) - th)
            kernel_o = max(kernel_o, min(d, 2 * np.pi - d))
            ang = np.float32(of[j, 7])
            d64 = sr.descriptor(lv, kr[i, 4], kr[i, 5], kr[i, 6], ang)
            measured_d = max(measured_d, np.abs(d64 - sr.descriptor(lv, kr[i, 4], kr[i, 5], kr[i, 6], ang, np.float32)).max())
            kernel_d = max(kernel_d, np.abs(dk[j] - d64).max())
    return {"key_points": n, "orientations_kernel": m, "orientations_restatement": restated,
            "orientation_overflow": int(ocounts[0, 1]),
            "key_points_with_another_number_of_orientations": len(wrong_count),
            "of_those_without_a_peak_margin_below_1e-4": len([i for i in wrong_count if i not in close_peak]),
            "key_points_with_a_peak_margin_below_1e-4": len(close_peak),
            "orientation_float32_vs_float64_rad": measured_o, "orientation_allowance_rad": 4 * measured_o,
            "orientation_kernel_vs_float64_rad": kernel_o, "orientation_excused": len(wrong_count),
            "descriptor_float32_vs_float64": float(measured_d), "descriptor_allowance": float(4 * measured_d),
            "descriptor_kernel_vs_float64": float(kernel_d), "descriptor_excused": 0,
            "_ori": (ori_f, ori_i, ocounts, desc)}


def stage_fixture_figures(sift):
    levels, rec = sr.stage_fixture()
    h, w = sr.STAGE_SHAPE
    lay = sift.pyramid_layout(h, w, 0, 2)
    gauss = upload(sift, levels, lay, False)
    raw_f, raw_i, counts = records(rec, 64)
    return orientation_and_descriptor(sift, gauss, lay, levels, raw_f, raw_i, counts, h, w, 0, 2)


def whole_extractor_figures(sift, k=48):
    """The `SIFT` module on the end-to-end fixture against the restatement, stage by stage along the module's own chain:
    the pyramid against float64 (its bound); then every later stage of the restatement is fed what the device produced
    before it -- detection the kernel's fp32 DoG levels, orientation the kernel's levels and records, the descriptor also
    the kernel's angle -- so that each is held to its stage tolerance with nothing excused for pyramid rounding; last,
    the module's output against the restated post-processing (filter_dog_point, top-k, RootSIFT) of that list."""
    img, fo, no = sr.e2e_fixture()
    h, w = img.shape
    dev = torch.from_numpy(img)[None].cuda()
    worst_g, worst_d, octaves_ok = pyramid_errors(sift, img[None], [None], fo, no)
    gauss, dog, lay = sift.pyramid(dev, None, fo, no)
    sizes = sr.octave_sizes(h, w, fo, no)
    kg, kd = download(sift, gauss, lay, 0, sizes, False), download(sift, dog, lay, 0, sizes, True)
    det = sr.detect(kd, fo)
    raw_f, raw_i, counts = sift.detect(dog, h, w, None, fo, no, cap=1024)
    fig = {"image": "sift_reference.e2e_fixture (120 x 160)", "first_octave": fo, "num_octaves": no,
           "pyramid_worst_gauss_error_over_bound": worst_g, "pyramid_worst_dog_error_over_bound": float(worst_d),
           "octaves_agree": octaves_ok, "detection": compare_raw(det, raw_f, raw_i, counts),
           "key_points_restatement": len(det["idx"])}
    od = orientation_and_descriptor(sift, gauss, lay, kg, raw_f, raw_i, counts, h, w, fo, no)
    ori_f, ori_i, ocounts, desc = od.pop("_ori")
    fig["orientation_and_descriptor"] = od
    m = int(ocounts[0, 0])
    of, dk = ori_f[0, :m].cpu().numpy(), desc[0, :m].cpu().numpy()
    keep = sr.filter_dog_point(of[:, :2], of[:, 2], of[:, 7], (h, w), 0, of[:, 3])
    order = keep[np.argsort(-of[keep, 3], kind="stable")][:k] if len(keep) > k else keep
    want = {"keypoints": of[order, :2], "scales": of[order, 2], "oris": of[order, 7], "keypoint_scores": of[order, 3],
            "descriptors": dk[order]}
    pred = sift.SIFT({"first_octave": fo, "num_octaves": no, "max_num_keypoints": k, "rootsift": False})({"image": dev[:, None]})
    fig["module_kept"], fig["restated_kept"], fig["after_filter_dog_point"] = int(pred["keypoints"].shape[1]), len(order), len(keep)
    fig["module_equals_restated_post_processing"] = all(
        pred[key].shape[1] == len(order) and np.array_equal(pred[key][0].cpu().numpy(), want[key]) for key in want)
    root = sift.SIFT({"first_octave": fo, "num_octaves": no, "max_num_keypoints": k})({"image": dev[:, None]})
    fig["module_rootsift_vs_restated"] = float(np.abs(root["descriptors"][0].cpu().double().numpy()
                                                      - sr.sift_to_rootsift(dk[order])).max())
    return fig
