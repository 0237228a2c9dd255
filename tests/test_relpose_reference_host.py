"""What the GPU comparison of the relative-pose estimator rests on, for the float64 restatement alone (CPU, no GPU):
the minimal solver solves, outlier-free scenes are recovered, the recorded constants of tests/relpose_reference.py
still hold, the classification band around each threshold is thin, the sampler is what the kernels draw, and the new
entry point checks its arguments and its workspace before anything is launched."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import relpose_reference as rr
from glue_factory_colon_amd import _native as nat
from glue_factory_colon_amd.eval_utils import ransac_sample_indices

INVALID, WORKSPACE = 1, 2


@functools.lru_cache(maxsize=None)
def table():
    """Every scene of the table through the restatement once, both reduction orders: (entry, block, serial)."""
    out = []
    for e in rr.table_cases():
        ths = rr.thresholds_for(e)
        blk = rr.ransac(e["case"], ths, e["hypotheses"], 3, 0, e["stream_id"], order="block")
        ser = rr.ransac(e["case"], ths, e["hypotheses"], 3, 0, e["stream_id"], order="serial")
        out.append((e, blk, ser))
    return out


def angle(a, b):
    """angle between two unit 9-vectors up to sign, accurate near 0"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return 2.0 * np.arcsin(min(1.0, 0.5 * min(np.linalg.norm(a - b), np.linalg.norm(a + b))))


def test_winners_solve_their_sample():
    for e, blk, _ in table():
        rec, _ = rr.records(e["case"])
        for r in blk:
            assert r["success"]
            E = r["E_minimal"].reshape(3, 3)
            assert abs(np.linalg.norm(E) - 1.0) < 1e-12
            big = np.argmax(np.abs(E))
            assert E.reshape(-1)[big] > 0
            pts = rec[r["sample"]]
            q0 = np.concatenate([pts[:, :2], np.ones((5, 1))], 1)
            q1 = np.concatenate([pts[:, 2:], np.ones((5, 1))], 1)
            epi = np.abs(np.einsum("ni,ij,nj->n", q1, E, q0))
            trace = 2 * E @ E.T @ E - np.trace(E @ E.T) * E
            print(e["row"], e["scene"], "epipolar", epi.max(), "det", abs(np.linalg.det(E)), "trace", np.abs(trace).max())
            # unit-norm E, bearings below 1: the residual of an exact solve is rounding times the solver's conditioning
            assert epi.max() < 1e-9 and abs(np.linalg.det(E)) < 1e-9 and np.abs(trace).max() < 1e-9


def test_outlier_free_scenes_recover_all_inliers():
    for e, blk, _ in table():
        n, share, sigma, _ = rr.REGIMES[e["regime"]]
        if share == 0 and sigma == 0:
            for r in blk:
                assert (r["inliers"] == (e["case"]["m0"] > -1)).all(), (e["row"], e["scene"])
                assert r["num_inliers"] == int((e["case"]["m0"] > -1).sum())


def test_restatement_on_the_table():
    worst, worst_cam, red = {}, {}, 0.0
    for e, blk, ser in table():
        err = max(max(r["r_err"], r["t_err"]) for r in blk)
        if e["camera"] is None:
            worst[e["regime"]] = max(worst.get(e["regime"], 0.0), err)
        else:
            worst_cam[e["camera"]] = max(worst_cam.get(e["camera"], 0.0), err)
        for a, b in zip(blk, ser):
            assert (a["best_hypothesis"], a["best_solution"]) == (b["best_hypothesis"], b["best_solution"])
            red = max(red, np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max())
    print("MEASURED_MAX_POSE_ERROR", worst)
    print("MEASURED_MAX_POSE_ERROR_CAMERA", worst_cam)
    print("MEASURED_REDUCTION_SPREAD", red)
    for g, v in worst.items():
        assert v <= 1.01 * rr.MEASURED_MAX_POSE_ERROR[g], (g, v)
    for m, v in worst_cam.items():
        assert v <= 1.01 * rr.MEASURED_MAX_POSE_ERROR_CAMERA[m], (m, v)
    assert red <= 1.01 * rr.MEASURED_REDUCTION_SPREAD
    # the constants are not slack either: each is reached within a factor 2
    assert all(v >= 0.5 * rr.MEASURED_MAX_POSE_ERROR[g] for g, v in worst.items())
    assert all(v >= 0.5 * rr.MEASURED_MAX_POSE_ERROR_CAMERA[m] for m, v in worst_cam.items())
    assert red >= 0.5 * rr.MEASURED_REDUCTION_SPREAD


def test_the_two_root_finding_routes_agree():
    spread = 0.0
    for e, blk, _ in table():
        n, share, sigma, _ = rr.REGIMES[e["regime"]]
        if not (share == 0 and sigma == 0):
            continue
        rec, _ = rr.records(e["case"])
        samples = np.unique(np.stack([r["sample"] for r in blk]), axis=0)
        Ea, oka = rr.five_point(rec[samples], "sturm")
        Eb, okb = rr.five_point(rec[samples], "companion")
        for i in range(len(samples)):
            assert oka[i].sum() == okb[i].sum() and oka[i].sum() > 0, (e["row"], e["scene"])
            for k in np.nonzero(oka[i])[0]:
                spread = max(spread, angle(Ea[i, k], Eb[i, k]))
    print("MEASURED_ROUTE_SPREAD", spread)
    assert spread <= 1.01 * rr.MEASURED_ROUTE_SPREAD and spread >= 0.5 * rr.MEASURED_ROUTE_SPREAD


def test_the_band_around_each_threshold_is_thin():
    for e, blk, _ in table():
        rec, _ = rr.records(e["case"])
        delta = rr.delta_for(e)
        for r in blk:
            d = np.sqrt(rr.sampson2(r["E"], rec))
            band = int((np.abs(d - np.sqrt(r["t2"])) < delta).sum())
            assert band <= 0.01 * len(rec), (e["row"], e["scene"], band)


def test_sampler():
    for n in (5, 6, 7, 12, 300):
        s = ransac_sample_indices(3, 41, n, 3000, sample_size=5)
        assert s.shape == (3000, 5) and s.min() >= 0 and s.max() < n
        assert (np.sort(s, 1)[:, 1:] != np.sort(s, 1)[:, :-1]).all()
    assert len(np.unique(ransac_sample_indices(0, 0, 300, 2000, sample_size=5), axis=0)) > 1990
    # sample_size = 4 is the homography estimator's sampler, value for value (recorded from the version without the keyword)
    want = {4: [[1, 2, 0, 3], [2, 0, 3, 1], [0, 1, 3, 2]], 9: [[3, 7, 0, 2], [4, 0, 7, 8], [2, 3, 8, 7]],
            300: [[117, 267, 10, 108], [161, 22, 6, 204], [69, 130, 94, 181]]}
    for n, rows in want.items():
        assert ransac_sample_indices(3, 7, n, 3).tolist() == rows
        assert ransac_sample_indices(3, 7, n, 3, sample_size=4).tolist() == rows
    with pytest.raises(ValueError):
        ransac_sample_indices(0, 0, 4, 10, sample_size=5)


def _host_compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return path
    raise RuntimeError("no host C++ compiler (g++, c++, clang++ or ROCm's clang++)")


def test_solver_header_on_the_host_equals_the_restatement(tmp_path):
    """csrc/relpose_solver.h is plain C++: compiled for the host (tests/cabi/relpose_solver_host.cpp, IEEE arithmetic,
    no contraction) it gives the restatement's numbers -- every model of every hypothesis, the decomposition, one
    Gauss-Newton round and the cheirality test bit for bit; the pose error to 1e-12 degrees (atan2 of two libraries)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = tmp_path / "librelpose_solver_host.so"
    r = subprocess.run([_host_compiler(), "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                        os.path.join(root, "glue-factory-colon_amd", "csrc"),
                        os.path.join(root, "tests", "cabi", "relpose_solver_host.cpp"), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    models = 0
    for e, blk, _ in table()[::3]:
        rec, _ = rr.records(e["case"])
        E, ok, s = rr.hypotheses(rec, 0, e["stream_id"], e["hypotheses"])
        K = len(s)
        flat = np.ascontiguousarray(rec[s].reshape(K, 20))
        Es, okc = np.zeros((K, 10, 9)), np.zeros((K, 10), np.uint8)
        lib.five_point_many(P(flat), K, P(Es), P(okc))
        assert np.array_equal(okc.astype(bool), ok) and np.array_equal(Es, E), (e["row"], e["scene"])
        models += int(ok.sum())
        r = blk[1]
        Rt = np.zeros(48)
        lib.decompose(P(np.ascontiguousarray(r["E_minimal"])), P(Rt))
        cands = rr.decompose(r["E_minimal"])
        for k in range(4):
            assert np.array_equal(Rt[12 * k:12 * k + 9].reshape(3, 3), cands[k][0])
            assert np.array_equal(Rt[12 * k + 9:12 * k + 12], cands[k][1])
        R, t = cands[0]
        recc = np.ascontiguousarray(rec)
        R2, t2 = np.ascontiguousarray(R.copy()), t.copy()
        moved = lib.gn_step(P(recc), len(rec), ctypes.c_double(r["t2"]), P(R2), P(t2))
        Ecur = rr.essential(R, t)
        b3, b4 = rr.tangent(t)
        with np.errstate(all="ignore"):
            inl = rr.sampson2(Ecur, rec) < r["t2"]
            acc = rr.block_sum(np.where(inl[:, None], rr.gn_terms(R, t, Ecur, b3, b4, rec), 0.0), "serial")
        upd = rr.gn_update(acc, b3, b4, R, t)
        assert bool(moved) == (upd is not None)
        if upd is not None:
            # the rotation goes through sin / cos of the step: two libraries, a rounding apart at most
            assert np.abs(upd[0] - R2).max() <= 4e-16 and np.abs(upd[1] - t2).max() <= 4e-16
        ch = np.zeros(len(rec), np.uint8)
        lib.cheiral(P(np.ascontiguousarray(R)), P(t), P(recc), len(rec), P(ch))
        assert np.array_equal(ch.astype(bool), rr.cheiral(R, t, rec))
        out = np.zeros(2)
        Rg, tg = e["case"]["T_gt"][:9].astype(np.float64), e["case"]["T_gt"][9:].astype(np.float64)
        lib.pose_error(P(np.ascontiguousarray(r["R"])), P(np.ascontiguousarray(r["t"])), P(Rg), P(tg), ctypes.c_double(0.0), P(out))
        assert abs(out[0] - r["r_err"]) <= 1e-12 and abs(out[1] - r["t_err"]) <= 1e-12
    assert models > 10000


def f(n):
    """A non-null, 16-byte aligned host address that is never dereferenced."""
    return ctypes.c_void_p(0x1000 * n)


def _call(lib, ws_bytes, B=2, M=100, N=100, T=3, hyp=512, lo=3, th=(1.0, 2.0, 3.0), model0=0, model1=3, ignore=0.0,
          cam0=f(4), gt=None, rerr=None, terr=None):
    ths = (ctypes.c_float * 8)(*(list(th) + [1.0] * (8 - len(th))))
    return lib.gfc_eval_relative_pose_ransac(f(1), f(2), f(3), None, cam0, model0, f(5), model1, gt, B, M, N, ths, T, hyp, lo,
                                             0, ignore, f(6), f(7), f(8), f(9), f(10), f(11), f(12), f(13), f(14), rerr,
                                             terr, f(15), ws_bytes, None)


def test_entry_point_checks_arguments_then_workspace():
    lib = nat.lib()
    need = lib.gfc_eval_relative_pose_ransac_workspace_bytes(2, 100, 3, 512)
    assert need > 1
    assert _call(lib, need - 1) == WORKSPACE and _call(lib, 0) == WORKSPACE
    # argument errors come first: asked with a workspace that is also too small
    assert _call(lib, 0, T=9, th=(1.0,) * 8) == INVALID and _call(lib, 0, T=0) == INVALID
    assert _call(lib, 0, B=0) == INVALID and _call(lib, 0, M=-1) == INVALID and _call(lib, 0, N=-1) == INVALID
    assert _call(lib, 0, hyp=0) == INVALID and _call(lib, 0, lo=-1) == INVALID and _call(lib, 0, hyp=1 << 27) == INVALID
    assert _call(lib, 0, th=(1.0, 0.0, 3.0)) == INVALID and _call(lib, 0, th=(1.0, -2.0, 3.0)) == INVALID
    assert _call(lib, 0, th=(1.0, float("inf"), 3.0)) == INVALID and _call(lib, 0, th=(float("nan"), 1.0, 3.0)) == INVALID
    assert _call(lib, 0, model0=4) == INVALID and _call(lib, 0, model1=-1) == INVALID
    assert _call(lib, 0, cam0=None) == INVALID and _call(lib, 0, ignore=-1.0) == INVALID
    assert _call(lib, 0, gt=f(16)) == INVALID and _call(lib, 0, gt=f(16), rerr=f(17)) == INVALID
    assert _call(lib, 0, gt=f(16), rerr=f(17), terr=f(18)) == WORKSPACE
    for args in ((0, 10, 3, 512), (2, -1, 3, 512), (2, 10, 0, 512), (2, 10, 9, 512), (2, 10, 3, 0)):
        assert lib.gfc_eval_relative_pose_ransac_workspace_bytes(*args) == 0
    # rs_splits' limits, as for the homography estimator: ceil(512 / B) and floor(num_hypotheses / 256) ranges
    sizes = [lib.gfc_eval_relative_pose_ransac_workspace_bytes(20, 100, 8, h) for h in (255, 256, 511, 512)]
    assert sizes[0] == sizes[1] == sizes[2] < sizes[3]
