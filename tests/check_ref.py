"""NumPy restatement of sd_stereo_check (INTEGRATION.md "sd_stereo_check"; kernels in csrc/check.hip): the visibility
classes and the photometric residual of a disparity map, float32 with every operation rounded on its own. The device
stage is compared with this bit for bit (rows' two sums within the bound of their summation order)."""

from __future__ import annotations

import numpy as np

F = np.float32
COLOURS = {1: (0, 0, 0), 2: (0, 0, 255), 3: (255, 0, 0), 4: (255, 255, 0)}


def check(disp, left=None, right=None, occ_tol=0.5, photo_thr=np.inf) -> dict:
    """disp float32 [H, W]; left, right uint8 [H, W, 3] or both None. Returns cls uint8 [H, W], disp_vis float32 [H, W],
    row float64 [8] and, with frames, resid float32 [H, W] and vis_rgb uint8 [H, W, 3] (None without)."""
    disp = np.asarray(disp, dtype=F)
    H, W = disp.shape
    occ_tol, photo_thr = F(occ_tol), F(photo_thr)
    frames = left is not None
    assert frames == (right is not None)
    with np.errstate(all="ignore"):
        has = np.isfinite(disp) & (disp > 0)
        x = np.broadcast_to(np.arange(W).astype(F), (H, W))
        xr = (x - np.where(has, disp, F(0))).astype(F)
        oov = has & (xr < 0)
        # m(x): the minimum of xr over the values right of x, by a min-scan of the reversed row shifted by one
        cand = np.where(has, xr, F(np.inf)).astype(F)
        incl = np.minimum.accumulate(cand[:, ::-1], axis=1)[:, ::-1]
        m = np.concatenate([incl[:, 1:], np.full((H, 1), np.inf, dtype=F)], axis=1)
        occ = has & ~oov & ((m + occ_tol).astype(F) <= xr)
        vis = has & ~oov & ~occ
        cls = np.full((H, W), 1, dtype=np.uint8)
        cls[oov], cls[occ], cls[vis] = 2, 3, 0
        resid = vis_rgb = None
        row = np.zeros(8, dtype=np.float64)
        row[0], row[1], row[2] = has.sum(), oov.sum(), occ.sum()
        if frames:
            left = np.asarray(left, dtype=np.uint8)
            right = np.asarray(right, dtype=np.uint8)
            xs = np.where(vis, xr, F(0)).astype(F)  # elsewhere any column: the result is masked
            x0 = np.minimum(np.floor(xs).astype(np.int64), W - 1)
            f = (xs - x0.astype(F)).astype(F)
            x1 = np.minimum(x0 + 1, W - 1)
            yy = np.broadcast_to(np.arange(H)[:, None], (H, W))
            a = right[yy, x0].astype(F)
            b = right[yy, x1].astype(F)
            r = (a + (f[..., None] * (b - a).astype(F)).astype(F)).astype(F)
            ad = np.abs((left.astype(F) - r).astype(F))
            e = ((ad[..., 0] + ad[..., 1]).astype(F) + ad[..., 2]).astype(F)
            resid = np.where(vis, e, F(np.nan)).astype(F)
            mis = vis & (e > photo_thr)
            cls[mis] = 4
            e64 = e[vis].astype(np.float64)
            row[3], row[4], row[5], row[6] = vis.sum(), e64.sum(), (e64 * e64).sum(), mis.sum()
            g = np.minimum(255, (np.where(vis, e, F(0)) / F(3.0)).astype(F).astype(np.int32)).astype(np.uint8)
            vis_rgb = np.repeat(g[..., None], 3, axis=2)
            for c, colour in COLOURS.items():
                vis_rgb[cls == c] = colour
        disp_vis = np.where(cls == 0, disp, F(np.nan)).astype(F)
    return {"cls": cls, "resid": resid, "disp_vis": disp_vis, "vis_rgb": vis_rgb, "row": row}


def step_edge_case(H: int = 4, W: int = 80, seed: int = 0):
    """The worked case: a background of disparity 6 and a nearer strip of 15 on columns 40..59; right random, left the
    right frame warped by the disparity. Returns (disp, left, right)."""
    rng = np.random.default_rng(seed)
    disp = np.full((H, W), 6, dtype=F)
    disp[:, 40:60] = 15
    right = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    src = np.clip(np.arange(W)[None, :] - disp.astype(np.int64), 0, W - 1)
    left = right[np.arange(H)[:, None], src]
    return disp, left, right


def random_case(n: int, H: int, W: int, seed: int):
    """The generator of the device tests: piecewise-constant disparity per row (runs of 3..12 pixels, uniform in
    [1, min(24, max(2, W / 3))], plus uniform +-0.2 jitter), 5 % of the pixels from NaN, 0, -3.5, +inf, -inf, -0; random
    frames. Returns (disp [n, H, W], left, right [n, H, W, 3])."""
    rng = np.random.default_rng(seed)
    hi = min(24.0, max(2.0, W / 3))
    disp = np.empty((n, H, W), dtype=F)
    for i in range(n):
        for y in range(H):
            x = 0
            while x < W:
                run = int(rng.integers(3, 13))
                disp[i, y, x:x + run] = rng.uniform(1.0, hi)
                x += run
    disp = (disp + rng.uniform(-0.2, 0.2, disp.shape)).astype(F)
    special = np.array([np.nan, 0.0, -3.5, np.inf, -np.inf, -0.0], dtype=F)
    hole = rng.random(disp.shape) < 0.05
    disp[hole] = special[rng.integers(0, len(special), int(hole.sum()))]
    left = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return disp, left, right
