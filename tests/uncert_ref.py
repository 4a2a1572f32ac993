"""NumPy restatement of sd_uncert_eval (include/stereo_hip.h, INTEGRATION.md "Uncertainty evaluation"), written from
that section: the two bins and q of a pixel, the curves from the integer histograms with Python integers and float64,
AUSE / AURG, the NLL with np.exp in float32 and the coverage counts. Test infrastructure only; the decode and the resize
are predict_ref's (oracle.data_ref's).

``sparsify_sorted`` is the textbook curve (a stable sort, the m_k least uncertain pixels kept): it is here only to show
what the binned definition means, and equals it to the last bit when every pixel has a bin of its own.
"""

from __future__ import annotations

import numpy as np

import predict_ref as R

BINS = 4096
HEAD = 16
Q_MAX = 2 ** 30
Z = (0.5, 1.0, 2.0, 3.0)
NOMINAL = tuple(1.0 - np.exp(-z) for z in Z)  # Laplace with b = exp(logvar)


def quantise(e: np.ndarray) -> np.ndarray:
    """int64 q = min(rint(e * 4096), 2^30) of float32 errors; the product is exact, ties go to even."""
    e = np.asarray(e, dtype=np.float32)
    with np.errstate(over="ignore"):
        return np.minimum(np.rint(e.astype(np.float64) * 4096.0), float(Q_MAX)).astype(np.int64)


def bin_u(lv: np.ndarray) -> np.ndarray:
    """The uncertainty bin of float32 log-variances: t = (lv + 32) * 64 in float32, saturating at 0 and 4095."""
    lv = np.asarray(lv, dtype=np.float32)
    with np.errstate(over="ignore"):
        t = ((lv + np.float32(32.0)).astype(np.float32) * np.float32(64.0)).astype(np.float32)
    inner = np.floor(np.clip(t, 0.0, 4095.0)).astype(np.int64)
    return np.where(t < 0, 0, np.where(t >= 4095, BINS - 1, inner))


def bin_o(e: np.ndarray) -> np.ndarray:
    """The oracle bin of float32 errors >= 0: 256 bins per octave over [2^-8, 2^8), from the bits of e."""
    bits = np.ascontiguousarray(e, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.clip((bits >> 15) - (119 << 8), 0, BINS - 1)


def histogram(bins: np.ndarray, q: np.ndarray) -> tuple[list[int], list[int]]:
    """cnt and sum of q per bin, as Python integers."""
    cnt, sm = [0] * BINS, [0] * BINS
    for j, v in zip(bins.reshape(-1).tolist(), q.reshape(-1).tolist()):
        cnt[j] += 1
        sm[j] += v
    return cnt, sm


def cuts(n: int, steps: int) -> list[int]:
    return [n - (n * k) // steps for k in range(steps)]


def curve(cnt: list[int], sm: list[int], steps: int) -> np.ndarray:
    """float64 [steps]: the mean error (pixels) of the m_k pixels in the lowest bins, the bin of the cut shared."""
    n = sum(cnt)
    out = np.zeros(steps, dtype=np.float64)
    if n == 0:
        return out
    c_inc, s_inc, c, s = [], [], 0, 0
    for a, b in zip(cnt, sm):
        c += a
        s += b
        c_inc.append(c)
        s_inc.append(s)
    for k, m in enumerate(cuts(n, steps)):
        j = next(i for i in range(BINS) if c_inc[i] >= m)
        c_lt, s_lt = (c_inc[j - 1], s_inc[j - 1]) if j else (0, 0)
        assert c_lt < m <= c_inc[j] and cnt[j] > 0
        out[k] = (float(s_lt) + float(m - c_lt) * float(sm[j]) / float(cnt[j])) / float(m) / 4096.0
    return out


def areas(unc: np.ndarray, orc: np.ndarray) -> tuple[float, float]:
    """(AUSE, AURG): each term formed and added in index order in float64; 0, 0 when unc_0 == 0."""
    steps = len(unc)
    u0 = float(unc[0])
    if u0 == 0.0:
        return 0.0, 0.0
    ause = aurg = 0.0
    for k in range(steps):
        ause += (float(unc[k]) - float(orc[k])) / u0
        aurg += 1.0 - float(unc[k]) / u0
    return ause / steps, aurg / steps


def row_from_pixels(e: np.ndarray, lv: np.ndarray, mul, steps: int) -> dict:
    """The row of one sample from its counted pixels (float32 e = |d - gt| and lv, both 1-D), with what the tests need
    beside it: ``row`` float64 [16 + 2 steps], ``cov_lo`` / ``cov_hi`` (the coverage counts with the pixels within 8
    float32 ulps of the threshold left out / counted in), ``nll`` and ``t`` (float64 per pixel: nll_px and its product
    term e_m * exp(-lv))."""
    e = np.asarray(e, dtype=np.float32).reshape(-1)
    lv = np.asarray(lv, dtype=np.float32).reshape(-1)
    mul = np.float32(mul)
    n = e.size
    row = np.zeros(HEAD + 2 * steps, dtype=np.float64)
    res = {"row": row, "cov_lo": np.zeros(4, np.int64), "cov_hi": np.zeros(4, np.int64),
           "nll": np.zeros(0), "t": np.zeros(0)}
    if n == 0:
        return res
    q = quantise(e)
    u, o = bin_u(lv), bin_o(e)
    cnt_u, sum_u = histogram(u, q)
    cnt_o, sum_o = histogram(o, q)
    unc, orc = curve(cnt_u, sum_u, steps), curve(cnt_o, sum_o, steps)
    with np.errstate(over="ignore", invalid="ignore"):
        e_m = (e / mul).astype(np.float32)
        t = (e_m * np.exp(-lv).astype(np.float32)).astype(np.float32)
        nll = (t + lv).astype(np.float32)
        b = np.exp(lv).astype(np.float32)
    row[0] = n
    row[1] = float(sum(q.tolist()))
    row[2] = nll.astype(np.float64).sum()
    for i, z in enumerate(Z):
        with np.errstate(over="ignore", invalid="ignore"):
            thr = (np.float32(z) * b).astype(np.float32)
            near = np.abs(e_m.astype(np.float64) - thr.astype(np.float64)) <= 8.0 * np.spacing(thr).astype(np.float64)
        near &= np.isfinite(thr)
        covered = e_m <= thr
        row[3 + i] = covered.sum()
        res["cov_lo"][i] = (covered & ~near).sum()
        res["cov_hi"][i] = res["cov_lo"][i] + near.sum()
    row[7], row[8] = areas(unc, orc)
    row[9] = cnt_u[0] + cnt_u[BINS - 1]
    row[10] = cnt_o[0] + cnt_o[BINS - 1]
    row[HEAD:HEAD + steps] = unc
    row[HEAD + steps:] = orc
    res.update(nll=nll.astype(np.float64), t=t.astype(np.float64))
    return res


def sample_rows(d_up: np.ndarray, lv_up: np.ndarray, gt_rgb: np.ndarray, mul, steps: int) -> list[dict]:
    """``row_from_pixels`` per sample of upsampled maps d_up, lv_up [B,Hs,Ws] float32 (sd_resize_bilinear's, with mul
    and with 1) against RGB24 ground truth [B,Hs,Ws,3]: a pixel counts when gt > 0 and d and lv are finite."""
    d_up = np.asarray(d_up, dtype=np.float32)
    lv_up = np.asarray(lv_up, dtype=np.float32)
    gt = R.decode(gt_rgb)
    out = []
    for b in range(d_up.shape[0]):
        m = (gt[b] > 0) & np.isfinite(d_up[b]) & np.isfinite(lv_up[b])
        e = np.abs(d_up[b][m] - gt[b][m]).astype(np.float32)
        out.append(row_from_pixels(e, lv_up[b][m], mul, steps))
    return out


def rows(d_up, lv_up, gt_rgb, mul, steps: int) -> np.ndarray:
    return np.stack([r["row"] for r in sample_rows(d_up, lv_up, gt_rgb, mul, steps)])


def sparsify_sorted(key: np.ndarray, e: np.ndarray, steps: int) -> np.ndarray:
    """The textbook sparsification curve: the pixels in ascending order of ``key`` (stable), curve_k = the float64 mean
    of ``e`` over the first m_k = n - floor(n k / steps) of them."""
    key, e = np.asarray(key).reshape(-1), np.asarray(e, dtype=np.float64).reshape(-1)
    order = np.argsort(key, kind="stable")
    csum = np.cumsum(e[order])
    return np.array([csum[m - 1] / m for m in cuts(e.size, steps)], dtype=np.float64)
