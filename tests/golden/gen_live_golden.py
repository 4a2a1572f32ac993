#!/usr/bin/env python3
"""Generate tests/golden/live_post.npz: inputs and outputs of the reference live app's own numpy functions
(live_camera/depth_live_dl.py) on 32x48 maps, for tests/test_live_cpu.py and tests/test_gpu_live.py.

Usage (CPU only):  python tests/golden/gen_live_golden.py <reference>/src

The reference module is imported with a stub ``cv2`` in sys.modules (cv2 is not needed for the arithmetic recorded
here); the stub's applyColorMap returns its input, so colorize_scalar_map yields the uint8 codes. Only data (inputs and
recorded results) is written.
"""

import sys
import tempfile
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
OUT = REPO / "tests" / "golden" / "live_post.npz"
H, W = 32, 48
FOCAL_MODEL, BASELINE = 400.0, 0.1  # f32(400 * 0.1) = 40: disparity 80 / k lies exactly on the k-th 0.5 m contour edge
ALPHA = 0.3


class _Cv2Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return 0 if name.isupper() else object

    @staticmethod
    def applyColorMap(codes, colormap):
        return codes


def _import_reference(src: str):
    sys.modules["cv2"] = _Cv2Stub("cv2")
    sys.path.insert(0, src)
    import live_camera.depth_live_dl as ref

    return ref


def _specials(a: np.ndarray, rng, frac=0.06):
    """Scatter NaN, +-inf, 0 and negative values over a copy of `a`."""
    a = a.copy()
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=np.float32)
    idx = rng.choice(a.size, int(frac * a.size), replace=False)
    a.reshape(-1)[idx] = vals[rng.integers(0, vals.size, idx.size)]
    return a


def _center(ref_median_src: np.ndarray, window: int):
    """depth_live_dl.py:542-551 on one map."""
    h, w = ref_median_src.shape
    cx, cy = w // 2, h // 2
    half = max(1, window // 2)
    y0, y1, x0, x1 = max(0, cy - half), min(h, cy + half + 1), max(0, cx - half), min(w, cx + half + 1)
    patch = ref_median_src[y0:y1, x0:x1]
    patch = patch[np.isfinite(patch) & (patch > 0.0)]
    return (float(np.median(patch)) if patch.size > 0 else float("nan")), patch.size


def main() -> None:
    ref = _import_reference(sys.argv[1])
    rng = np.random.default_rng(20260)
    out = {"focal_model": np.float64(FOCAL_MODEL), "baseline": np.float64(BASELINE), "alpha": np.float64(ALPHA)}

    # ---- disparity -> depth -> contours / fixed-range codes
    disp = rng.uniform(0.2, 60.0, (H, W)).astype(np.float32)
    disp = _specials(disp, rng)
    disp[2, 2:14] = np.array([80, 40, 20, 16, 10, 8, 5, 4, 4.0001, 3.9999, 3.2, 2], dtype=np.float32)  # bin edges, 10 m
    disp[3, 2:6] = np.array([1e-6, 2e-6, 1e-7, 1e6], dtype=np.float32)  # exactly the 1e-6 threshold (invalid)
    disp[10:14, 10:30] = np.float32(7.0)  # a flat patch: no contour inside
    disp[14:18, 10:30] = np.float32(8.5)
    depth = ref.disparity_to_depth(disp, FOCAL_MODEL, BASELINE)
    out["disp"], out["depth"] = disp, depth
    out["contour"] = ref.depth_contour_mask(depth, ref.DEPTH_CONTOUR_STEP_M, *ref.DEPTH_VIS_RANGE_M)
    out["depth_code"] = ref.colorize_scalar_map(depth, 0, fixed_range=ref.DEPTH_VIS_RANGE_M)
    logvar = rng.uniform(-6.0, 6.0, (H, W)).astype(np.float32)
    logvar = _specials(logvar, rng, 0.03)
    with np.errstate(all="ignore"):
        conf = ref.confidence_from_logvar(logvar)
    out["logvar"], out["conf"] = logvar, conf
    out["conf_code"] = ref.colorize_scalar_map(conf, 0, fixed_range=ref.CONFIDENCE_VIS_RANGE)
    # an all-invalid depth map: no contour, all codes 0
    bad = np.full((H, W), np.nan, dtype=np.float32)
    bad[::2] = np.float32(-1.0)
    bad[1::4, ::3] = np.inf
    bad[0, :5] = 0.0
    out["invalid"] = bad
    out["invalid_contour"] = ref.depth_contour_mask(bad, ref.DEPTH_CONTOUR_STEP_M, *ref.DEPTH_VIS_RANGE_M)
    out["invalid_code"] = ref.colorize_scalar_map(bad, 0)

    # ---- auto range (np.percentile 2 / 98): the disparity above, a map of heavily duplicated values, 0 / 1 / 2 valid
    dup = (rng.integers(1, 40, (H, W)) / 4.0).astype(np.float32)
    dup = _specials(dup, rng)
    one = bad.copy()
    one[17, 5] = np.float32(3.25)
    two = one.copy()
    two[4, 40] = np.float32(11.5)
    for name, m in (("disp", disp), ("dup", dup), ("invalid", bad), ("one", one), ("two", two)):
        out[f"auto/{name}/in"] = m
        with np.errstate(all="ignore"):
            out[f"auto/{name}/code"] = ref.colorize_scalar_map(m, 0)
        v = m[np.isfinite(m) & (m > 0.0)]
        lohi = [np.percentile(v, 2), np.percentile(v, 98)] if v.size else [np.nan, np.nan]
        out[f"auto/{name}/lohi"] = np.asarray(lohi, dtype=np.float32)

    # ---- EMA over three frames (:531-540)
    frames = [_specials(rng.uniform(0.2, 60.0, (H, W)).astype(np.float32), rng, 0.02) for _ in range(3)]
    smoothed = None
    for i, prediction in enumerate(frames):
        smoothed = prediction if smoothed is None else ALPHA * prediction + (1.0 - ALPHA) * smoothed
        out[f"ema/in{i}"], out[f"ema/out{i}"] = prediction, smoothed

    # ---- centre-window medians (:542-595): odd and even valid counts, a clipped and an empty window
    odd = disp.copy()
    odd[9:24, 17:32] = rng.uniform(1.0, 50.0, (15, 15)).astype(np.float32)
    odd[16, 24] = np.nan  # 224 valid values in the 15 x 15 window
    odd[15, 23] = np.float32(-2.0)  # 223
    even = odd.copy()
    even[17, 25] = np.inf  # 222
    cases = []
    for name, m, window in (("odd", odd, 15), ("even", even, 15), ("small", even, 4), ("zero", odd, 0),
                            ("clipped", disp, 63), ("empty", bad, 15)):
        med, cnt = _center(m, window)
        out[f"center/{name}/in"] = m
        out[f"center/{name}/window_median_count"] = np.array([window, med, cnt], dtype=np.float64)
        cases.append((name, cnt))
    assert dict(cases)["odd"] % 2 == 1 and dict(cases)["even"] % 2 == 0 and dict(cases)["empty"] == 0, cases

    # ---- calibration geometry (:321-368)
    P1 = np.array([[812.5, 0, 322.0, 0], [0, 812.5, 241.0, 0], [0, 0, 1, 0]], dtype=np.float64)
    P2 = P1.copy()
    P2[0, 3] = -97.5  # baseline 0.12 m
    T = np.array([[-0.1], [0.02], [0.005]], dtype=np.float64)
    nan = float("nan")
    for name, args in (("p", (P1, P2, T)), ("t", (None, None, T)), ("none", (None, None, None)),
                       ("p_zero_tx", (P1, P1, T))):
        b = ref.estimate_baseline_m(*args)
        out[f"baseline/{name}"] = np.float64(nan if b is None else b)
    out["calib/P1"], out["calib/P2"], out["calib/T"] = P1, P2, T
    out["calib/image_size"] = np.array([640, 480])
    out["calib/mtx_l"] = np.array([[800.0, 0, 320.0], [0, 800.0, 240.0], [0, 0, 1]])
    with tempfile.TemporaryDirectory() as tmp:
        full = Path(tmp) / "full.npz"
        np.savez(full, P1=P1, P2=P2, T=T, image_size=out["calib/image_size"], mtx_l=out["calib/mtx_l"])
        bare = Path(tmp) / "bare.npz"
        np.savez(bare, mtx_l=out["calib/mtx_l"], T=T)
        for name, path in (("full", full), ("bare", bare)):
            f, b, wpx = ref.load_calibration_geometry(path)
            out[f"calib/{name}/geometry"] = np.array([nan if f is None else f, nan if b is None else b,
                                                       nan if wpx is None else wpx], dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
