"""NumPy restatement of sd_disp_export's per-pixel arithmetic (include/stereo_hip.h, INTEGRATION.md "Predict and
evaluate from files"): the RGB24 code of a value, its decode, and the metric rows. Test infrastructure only; builds on
oracle.data_ref (the decode is its depth_uint8_decoding, the resize its resize_bilinear).

Where this departs from oracle.data_ref.encode_disparity_to_rgb, and why:

* the product v * 1000 is formed exactly (float64 holds a float32 times 1000) and rounded once. Rounded to float32
  first, as ``np.round(disparity * scale)`` does on float32 input, 47187 of the codes c in [8192011, 8388607] do not
  decode back to float32(c / 1000) (counted over all 16646656 codes); with the exact product every code does;
* R = c // 65025 reaches 256 for the top 256 codes (c >= 16646400), which a byte cannot hold: the digits saturate
  there (R = min(., 255), G = min(rem // 255, 255), B = the rest), so (255, 255, 255) is the largest code, 16646655,
  the largest value depth_uint8_decoding can return. Below 16646400 the bytes are the oracle's.
"""

from __future__ import annotations

import numpy as np

from oracle import data_ref

MAX_CODE = 16646655  # 255 * 65025 + 255 * 255 + 255


def disp_code(v: np.ndarray) -> np.ndarray:
    """int64 code of float32 values: 0 where not finite, else rint(clip(v * 1000, 0, MAX_CODE)), ties to even."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.clip(v.astype(np.float64) * 1000.0, 0.0, float(MAX_CODE))
        c = np.rint(np.where(np.isfinite(v), p, 0.0))
    return c.astype(np.int64)


def code_to_rgb(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c, dtype=np.int64)
    r = np.minimum(c // 65025, 255)
    rem = c - r * 65025
    g = np.minimum(rem // 255, 255)
    b = rem - g * 255
    assert b.max(initial=0) <= 255 and c.min(initial=0) >= 0
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def rgb_to_code(rgb: np.ndarray) -> np.ndarray:
    a = rgb.astype(np.int64)
    return a[..., 0] * 65025 + a[..., 1] * 255 + a[..., 2]


def encode(v: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] of float32 values."""
    return code_to_rgb(disp_code(v))


def decode(rgb: np.ndarray) -> np.ndarray:
    """float32 values of uint8 [..., 3]: the reference's depth_uint8_decoding."""
    return data_ref.depth_uint8_decoding(rgb)


def upsample(maps: np.ndarray, out_hw: tuple[int, int], mul) -> np.ndarray:
    """[B,H,W] float32 -> [B,Hs,Ws]: data_ref.resize_bilinear times the float32 scalar mul."""
    return (data_ref.resize_bilinear(maps.astype(np.float32), out_hw) * np.float32(mul)).astype(np.float32)


def width_scale(Ws: int, W: int) -> np.float32:
    return np.float32(Ws / float(W))


def sigma_values(logvar_up: np.ndarray, mul) -> np.ndarray:
    """float32 exp(0.5 lv) * mul on the upsampled (mul = 1) log-variance."""
    return (np.exp(np.float32(0.5) * logvar_up.astype(np.float32)).astype(np.float32) * np.float32(mul)).astype(np.float32)


def metric_rows(d: np.ndarray, gt_rgb: np.ndarray) -> np.ndarray:
    """float64 [B,8] rows of upsampled disparities d [B,Hs,Ws] float32 against RGB24 ground truth [B,Hs,Ws,3]:
    n, sum e, sum e^2, #(e > 1), #(e > 2), #(e > 3), #(e > 3 and e > 0.05f * gt), 0; e = |d - gt| in float32."""
    d = np.asarray(d, dtype=np.float32)
    gt = decode(gt_rgb)
    rows = np.zeros((d.shape[0], 8), dtype=np.float64)
    for b in range(d.shape[0]):
        m = (gt[b] > 0) & np.isfinite(d[b])
        e = np.abs(d[b][m] - gt[b][m]).astype(np.float32)
        e64 = e.astype(np.float64)
        rel = (np.float32(0.05) * gt[b][m]).astype(np.float32)
        rows[b] = [m.sum(), e64.sum(), (e64 * e64).sum(), (e > 1).sum(), (e > 2).sum(), (e > 3).sum(),
                   ((e > 3) & (e > rel)).sum(), 0.0]
    return rows
