"""NumPy restatement of the preview montage (the reference's eval_utils.py:42-73) as include/stereo_hip.h states it for
sd_quantile_select_n and sd_preview_compose_n. tests/golden/gen_preview_golden.py asserts that it reproduces the
reference's own save_preview_montage byte for byte on every fixture sample.

np.percentile on a float32 array forms (n - 1) * q and the interpolation in float32; the statement (and this file) forms
them in fp64 and rounds to float32 once. The two can differ by one float32 step, which moves no code on the fixture."""

from __future__ import annotations

import numpy as np

Q_LO, Q_HI = 0.05, 0.95


def quantile_select(values: np.ndarray, q_lo: float = Q_LO, q_hi: float = Q_HI) -> dict:
    """The `sel` row of one map: n, the four order statistics, lo and hi (NaN when no value is finite)."""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    v = np.sort(v[np.isfinite(v)])
    n = int(v.size)
    if n == 0:
        nan = np.float32(np.nan)
        return {"n": 0, "stats": np.full(4, nan, dtype=np.float32), "lo": nan, "hi": nan}
    stats, out = [], []
    for q in (q_lo, q_hi):
        pos = np.float64(n - 1) * np.float64(q)
        k = int(np.floor(pos))
        k = min(k, n - 1)
        k1 = min(k + 1, n - 1)
        g = pos - np.floor(pos)
        a, b = np.float64(v[k]), np.float64(v[k1])
        stats += [v[k], v[k1]]
        out.append(np.float32(a + (b - a) * g))
    return {"n": n, "stats": np.asarray(stats, dtype=np.float32), "lo": out[0], "hi": out[1]}


def colour_panel(planes: np.ndarray) -> np.ndarray:
    """f32 [3][H][W] -> u8 [H][W][3]: trunc(clip(float32(x * 255), 0, 255)), NaN -> 0."""
    x = np.asarray(planes, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = x * np.float32(255.0)
        v = np.where(np.isnan(v), np.float32(0.0), np.clip(v, np.float32(0.0), np.float32(255.0)))
    return v.astype(np.uint8).transpose(1, 2, 0)


def map_panel(m: np.ndarray, lo=None, hi=None) -> np.ndarray:
    """f32 [H][W] -> u8 [H][W][3] (_normalize_map). lo / hi: the percentiles to use instead of this file's own (the
    device's, when a test checks the composer apart from the select); a map without a finite value is all zeros."""
    m = np.asarray(m, dtype=np.float32)
    sel = quantile_select(m)
    if sel["n"] == 0:
        return np.zeros((*m.shape, 3), dtype=np.uint8)
    vmin = np.float32(sel["lo"] if lo is None else lo)
    vmax = np.float32(sel["hi"] if hi is None else hi)
    scale = np.float32(max(np.float64(vmax) - np.float64(vmin), 1e-6))
    with np.errstate(invalid="ignore", over="ignore"):
        x = (m - vmin) / scale
        x = np.where(np.isnan(x), np.float32(0.0), np.clip(x, np.float32(0.0), np.float32(1.0))).astype(np.float32)
        gray = (x * np.float32(255.0)).astype(np.uint8)
    return np.stack([gray, gray, gray], axis=-1)


def montage(inp: np.ndarray, tgt: np.ndarray, pred: np.ndarray, sel_t=None, sel_p=None) -> np.ndarray:
    """inp f32 [6][H][W], tgt, pred f32 [H][W] -> u8 [H][4W][3]. sel_t / sel_p: optional (lo, hi) pairs."""
    H, W = inp.shape[1:]
    tgt, pred = np.asarray(tgt).reshape(H, W), np.asarray(pred).reshape(H, W)
    lt, ht = (None, None) if sel_t is None else sel_t
    lp, hp = (None, None) if sel_p is None else sel_p
    return np.concatenate([colour_panel(inp[:3]), colour_panel(inp[3:6]), map_panel(tgt, lt, ht),
                           map_panel(pred, lp, hp)], axis=1)
