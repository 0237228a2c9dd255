"""The random configurations of tests/test_oracle_vs_reference_fuzz.py, shared by the generator of its fixture
(make_golden.py::golden_reference_fuzz, which runs the reference on them -> reference_fuzz.npz) and the test, which
runs the oracle on the same draws.  Every case is drawn from a seeded torch generator in a fixed order: the same
inputs on every machine.  No reference code involved."""
import numpy as np
import torch

SAMPLE_ROWS = 1  # rows of a large array stored in full (the first); every row also gets a weighted checksum


def sample_rows(n):
    """The rows of an n-row array that the fixture stores in full."""
    return np.unique(np.linspace(0, n - 1, min(n, SAMPLE_ROWS)).round().astype(np.int64))


def row_weights(dim):
    """The fixed weight vector (|w| <= 1) of the row checksums: the first of bench_inputs.desc_checksum_weights."""
    from bench_inputs import desc_checksum_weights

    return desc_checksum_weights(dim)[0].double()


def row_checksums(a):
    """[N, D] -> [N] float64: the weighted sum of every row."""
    return torch.as_tensor(a).double() @ row_weights(a.shape[-1])


def _ri(g, lo, hi):
    return int(torch.randint(lo, hi + 1, (1,), generator=g))


def superpoint_open_cases():
    """14 configurations of the open SuperPoint: any image size (not only multiples of 8), batches of 1-2, every NMS
    radius, border widths, thresholds, top-k above / below the candidate count, RGB input every third case.
    Yields (case, image [b,c,h,w], conf)."""
    from glue_factory_colon_amd import synthetic

    g = torch.Generator().manual_seed(501)
    for case in range(14):
        h, w = _ri(g, 40, 150), _ri(g, 40, 170)  # any size: the network floors to multiples of 8 on its way down
        b = _ri(g, 1, 2)
        r, border = _ri(g, 0, 4), (0, 4, 6)[_ri(g, 0, 2)]
        th = (0.0, 0.005, 0.02)[_ri(g, 0, 2)]
        k = (None, 30, 400)[_ri(g, 0, 2)]
        img = synthetic.synthetic_images(b, h, w, seed=700 + case)
        if case % 3 == 0:
            img = torch.cat([img * 0.9, img, img * 0.8], 1).clamp(0, 1)
        yield case, img, dict(nms_radius=r, remove_borders=border, detection_threshold=th, max_num_keypoints=k)


def superpoint_official_cases():
    """10 configurations of the official SuperPoint: legacy / fixed sampling, with and without an image_size crop.
    Yields (case, image [1,1,h,w], image_size [1,2] or None, conf)."""
    from glue_factory_colon_amd import synthetic

    g = torch.Generator().manual_seed(502)
    for case in range(10):
        h, w = 8 * _ri(g, 6, 18), 8 * _ri(g, 6, 20)
        r, border = _ri(g, 1, 4), (2, 4)[_ri(g, 0, 1)]
        th = (0.0, 0.005)[_ri(g, 0, 1)]
        k = (-1, 60, 2000)[_ri(g, 0, 2)]
        legacy = bool(_ri(g, 0, 1))
        img = synthetic.synthetic_images(1, h, w, seed=800 + case)
        size = None
        if case % 2:
            size = torch.tensor([[float(w - _ri(g, 0, 12)), float(h - _ri(g, 0, 10))]])
        yield case, img, size, dict(nms_radius=r, remove_borders=border, detection_threshold=th, max_num_keypoints=k,
                                    legacy_sampling=legacy)


def lightglue_cases():
    """8 LightGlue inputs: tiny (1-6 points) and unequal key-point sets, thresholds, correlated descriptors (real
    matches) every second case.  Yields (case, data dict of the matcher's inputs, filter_threshold)."""
    g = torch.Generator().manual_seed(503)
    for case in range(8):
        b = _ri(g, 1, 2)
        m_, n_ = (_ri(g, 1, 6), _ri(g, 1, 6)) if case < 2 else (_ri(g, 20, 260), _ri(g, 20, 260))
        th = (0.0, 0.1, 0.3)[_ri(g, 0, 2)]
        size = torch.tensor([[float(_ri(g, 200, 700)), float(_ri(g, 150, 500))]] * b)
        kp0, kp1 = torch.rand((b, m_, 2), generator=g) * size[:, None], torch.rand((b, n_, 2), generator=g) * size[:, None]
        d0 = torch.nn.functional.normalize(torch.randn((b, m_, 256), generator=g), dim=-1)
        d1 = torch.nn.functional.normalize(torch.randn((b, n_, 256), generator=g), dim=-1)
        if case % 2:  # correlated descriptors: real matches
            n_common = min(m_, n_)
            d1[:, :n_common] = torch.nn.functional.normalize(d0[:, :n_common] + 0.1 * torch.randn((b, n_common, 256), generator=g), dim=-1)
        yield case, {"keypoints0": kp0, "keypoints1": kp1, "descriptors0": d0, "descriptors1": d1,
                     "view0": {"image_size": size}, "view1": {"image_size": size}}, th


def auc_cases():
    """Error lists for the AUC of the evaluation summaries: (n, errors, thresholds), incl. an infinite error (a pair
    with fewer than four matches, eval/utils.py:289-291) and one exactly on a threshold."""
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 540):
        errors = (rng.gamma(1.5, 2.0, n)).tolist()
        if n == 540:
            errors[5] = float("inf")
            errors[9] = 3.0
        for ths in ([1, 3, 5], [5, 10, 20]):
            yield n, errors, ths
