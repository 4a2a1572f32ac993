"""NumPy restatement of the classical live loop's matcher (the reference's live_camera/depth_live.py:155-178:
cvtColor, StereoSGBM.compute in 3-way mode, reprojectImageTo3D, nanmedian, normalize), written from the statement in
INTEGRATION.md ("The semi-global matcher"), not from the kernels. Everything up to the int16 disparity is integer
arithmetic, so the device path is held to these arrays bit for bit. Vectorised over d (and over the lines that run in
parallel), plain loops along each scan direction.
"""

from __future__ import annotations

from collections import deque

import numpy as np

INF = 1 << 28  # "+infinity" of the d +- 1 neighbours outside [0, D)
DISP2COST_MAX = np.iinfo(np.int32).max


class Params:
    def __init__(self, min_disparity=0, num_disparities=128, block_size=7, P1=None, P2=None, disp12_max_diff=1,
                 uniqueness_ratio=10, speckle_window_size=100, speckle_range=2, pre_filter_cap=31):
        self.minD, self.D, self.bs = int(min_disparity), int(num_disparities), int(block_size)
        self.P1 = 8 * self.bs * self.bs if P1 is None else int(P1)
        self.P2 = 32 * self.bs * self.bs if P2 is None else int(P2)
        self.max_diff, self.uniq = int(disp12_max_diff), int(uniqueness_ratio)
        self.speckle_window, self.speckle_range = int(speckle_window_size), int(speckle_range)
        self.cap = int(pre_filter_cap)
        assert self.minD >= 0 and self.D % 16 == 0 and 16 <= self.D <= 256 and self.bs % 2 == 1 and 3 <= self.bs <= 11
        assert 3 * (self.bs * self.bs * (2 * self.cap + 63) + self.P2) <= 65535

    @property
    def maxD(self):
        return self.minD + self.D

    @property
    def invalid(self):
        return 16 * (self.minD - 1)


# ---------------------------------------------------------------------- stages 1, 2
def gray(bgr: np.ndarray) -> np.ndarray:
    c = bgr.astype(np.int32)
    return ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def prefilter(a: np.ndarray, cap: int) -> np.ndarray:
    A = np.pad(a.astype(np.int32), 1, mode="edge")
    s = 2 * (A[1:-1, 2:] - A[1:-1, :-2]) + (A[:-2, 2:] - A[:-2, :-2]) + (A[2:, 2:] - A[2:, :-2])
    return (np.clip(s, -cap, cap) + cap).astype(np.uint8)


# ---------------------------------------------------------------------- stages 3, 4
def _bt_terms(a):
    A = a.astype(np.int32)
    P = np.pad(A, ((0, 0), (1, 1)), mode="edge")
    lo, hi = (A + P[:, :-2]) >> 1, (A + P[:, 2:]) >> 1
    return A, np.minimum(A, np.minimum(lo, hi)), np.maximum(A, np.maximum(lo, hi))


def _bt(left, right, p: Params) -> np.ndarray:
    """Birchfield-Tomasi cost [H, W - maxD, D] of the columns x >= maxD."""
    H, W = left.shape
    u, u0, u1 = _bt_terms(left)
    v, v0, v1 = _bt_terms(right)
    xs = np.arange(p.maxD, W)
    out = np.zeros((H, len(xs), p.D), dtype=np.int32)
    for d in range(p.D):
        xr = xs - d - p.minD
        U, U0, U1 = u[:, xs], u0[:, xs], u1[:, xs]
        V, V0, V1 = v[:, xr], v0[:, xr], v1[:, xr]
        a = np.maximum(0, np.maximum(U - V1, V0 - U))
        b = np.maximum(0, np.maximum(V - U1, U0 - V))
        out[:, :, d] = np.minimum(a, b)
    return out


def pixel_cost(gray_l, gray_r, pre_l, pre_r, p: Params) -> np.ndarray:
    return _bt(pre_l, pre_r, p) + (_bt(gray_l, gray_r, p) >> 2)


def block_sum(cost: np.ndarray, bs: int) -> np.ndarray:
    r = bs // 2
    c = np.pad(cost, ((r, r), (r, r), (0, 0)), mode="edge")
    H, Wv = cost.shape[:2]
    out = np.zeros_like(cost)
    for dy in range(bs):
        for dx in range(bs):
            out += c[dy:dy + H, dx:dx + Wv]
    return out


def cost_volume(gray_l, gray_r, pre_l, pre_r, p: Params) -> np.ndarray:
    """C uint16 [H, W, D]; the columns x < maxD are zero (never read)."""
    H, W = gray_l.shape
    C = np.zeros((H, W, p.D), dtype=np.uint16)
    if W > p.maxD:
        s = block_sum(pixel_cost(gray_l, gray_r, pre_l, pre_r, p), p.bs)
        assert s.max() <= 65535
        C[:, p.maxD:] = s
    return C


# ---------------------------------------------------------------------- stage 5
def _path_step(Lq, Cp, P1, P2):
    m = Lq.min(axis=-1, keepdims=True)
    pad = np.full(Lq.shape[:-1] + (1,), INF, dtype=np.int64)
    down = np.concatenate([pad, Lq[..., :-1]], axis=-1) + P1
    up = np.concatenate([Lq[..., 1:], pad], axis=-1) + P1
    return Cp + np.minimum(np.minimum(Lq, down), np.minimum(up, m + P2)) - m


def aggregate(C: np.ndarray, p: Params) -> np.ndarray:
    """S uint16 [H, W, D], the sum of the three paths; zero for x < maxD."""
    H, W, D = C.shape
    S = np.zeros((H, W, D), dtype=np.int64)
    if W <= p.maxD:
        return S.astype(np.uint16)
    Cv = C[:, p.maxD:].astype(np.int64)
    Wv = Cv.shape[1]
    Sv = S[:, p.maxD:]
    L = Cv[0]
    Sv[0] += L
    for y in range(1, H):  # top -> down
        L = _path_step(L, Cv[y], p.P1, p.P2)
        Sv[y] += L
    L = Cv[:, 0]
    Sv[:, 0] += L
    for x in range(1, Wv):  # left -> right
        L = _path_step(L, Cv[:, x], p.P1, p.P2)
        Sv[:, x] += L
    L = Cv[:, Wv - 1]
    Sv[:, Wv - 1] += L
    for x in range(Wv - 2, -1, -1):  # right -> left
        L = _path_step(L, Cv[:, x], p.P1, p.P2)
        Sv[:, x] += L
    assert S.max() <= 65535
    return S.astype(np.uint16)


# ---------------------------------------------------------------------- stages 6, 7
def winner(S: np.ndarray, p: Params):
    """(q int16 [H, W] before the left-right check, disp2 int32 [H, W])."""
    H, W, D = S.shape
    q = np.full((H, W), p.invalid, dtype=np.int64)
    disp2 = np.full((H, W), p.minD - 1, dtype=np.int64)
    cost2 = np.full((H, W), DISP2COST_MAX, dtype=np.int64)
    rows = np.arange(H)
    dd = np.arange(D)[None, :]
    for x in range(W - 1, p.maxD - 1, -1):
        s = S[:, x].astype(np.int64)
        best = s.argmin(axis=1)  # the lowest d of the minimum
        mn = s[rows, best]
        far = np.abs(dd - best[:, None]) > 1
        bad = (far & (s * (100 - p.uniq) < mn[:, None] * 100)).any(axis=1)
        ok = ~bad
        x2 = x - best - p.minD
        upd = ok & (cost2[rows, x2] > mn)
        cost2[rows[upd], x2[upd]] = mn[upd]
        disp2[rows[upd], x2[upd]] = best[upd] + p.minD
        inner = (best > 0) & (best < D - 1)
        sm = s[rows, np.clip(best - 1, 0, D - 1)]
        sp = s[rows, np.clip(best + 1, 0, D - 1)]
        den = np.maximum(sm + sp - 2 * mn, 1)
        num = (sm - sp) * 16 + den
        frac = np.sign(num) * (np.abs(num) // (2 * den))  # C integer division
        val = 16 * best + np.where(inner, frac, 0) + 16 * p.minD
        q[ok, x] = val[ok]
    return q.astype(np.int16), disp2


def lr_check(q: np.ndarray, disp2: np.ndarray, p: Params) -> np.ndarray:
    if p.max_diff < 0:
        return q.copy()
    H, W = q.shape
    out = q.astype(np.int64)
    x = np.arange(W)[None, :]
    rows = np.arange(H)[:, None]
    valid = out != p.invalid

    def fails(dv):
        xx = x - dv
        inside = (xx >= 0) & (xx < W)
        d2 = disp2[rows, np.clip(xx, 0, W - 1)]
        return inside & (d2 >= p.minD) & (np.abs(d2 - dv) > p.max_diff)

    bad = valid & fails(out >> 4) & fails((out + 15) >> 4)
    out[bad] = p.invalid
    return out.astype(np.int16)


# ---------------------------------------------------------------------- stage 8
def speckle(q: np.ndarray, invalid: int, window: int, rng: int) -> np.ndarray:
    """Plain flood fill: 4-neighbour edges between valid pixels that differ by <= 16 * rng; components of <= window
    pixels become invalid. window == 0: unchanged."""
    out = q.copy()
    if window <= 0:
        return out
    H, W = q.shape
    seen = np.zeros((H, W), dtype=bool)
    v = q.astype(np.int64)
    lim = 16 * rng
    for y0 in range(H):
        for x0 in range(W):
            if seen[y0, x0] or v[y0, x0] == invalid:
                continue
            comp = [(y0, x0)]
            seen[y0, x0] = True
            todo = deque(comp)
            while todo:
                y, x = todo.popleft()
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and v[yy, xx] != invalid \
                            and abs(v[yy, xx] - v[y, x]) <= lim:
                        seen[yy, xx] = True
                        comp.append((yy, xx))
                        todo.append((yy, xx))
            if len(comp) <= window:
                for y, x in comp:
                    out[y, x] = invalid
    return out


# ---------------------------------------------------------------------- the matcher, every stage boundary
def compute_stages(gray_l: np.ndarray, gray_r: np.ndarray, p: Params) -> dict:
    pre_l, pre_r = prefilter(gray_l, p.cap), prefilter(gray_r, p.cap)
    C = cost_volume(gray_l, gray_r, pre_l, pre_r, p)
    S = aggregate(C, p)
    q_raw, disp2 = winner(S, p)
    q_lr = lr_check(q_raw, disp2, p)
    q = speckle(q_lr, p.invalid, p.speckle_window, p.speckle_range)
    return {"pre_l": pre_l, "pre_r": pre_r, "C": C, "S": S, "q_raw": q_raw, "disp2": disp2, "q_lr": q_lr, "q": q}


def compute(gray_l, gray_r, p: Params) -> np.ndarray:
    return compute_stages(gray_l, gray_r, p)["q"]


# ---------------------------------------------------------------------- stage 9
def post(q: np.ndarray, Q: np.ndarray):
    """(disp f32 with NaN, z f32 with NaN, code u8) of depth_live.py:161-177."""
    H, W = q.shape
    disp = q.astype(np.float32) / np.float32(16.0)
    disp[disp <= 0.0] = np.nan
    d0 = np.nan_to_num(disp, nan=0.0)
    Q = np.asarray(Q, dtype=np.float64)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    d = d0.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        num = ((Q[2, 0] * x + Q[2, 1] * y) + Q[2, 2] * d) + Q[2, 3]
        den = ((Q[3, 0] * x + Q[3, 1] * y) + Q[3, 2] * d) + Q[3, 3]
        z = (num / den).astype(np.float32)
    z[np.isnan(disp)] = np.nan
    lo, hi = float(d0.min()), float(d0.max())
    scale = 255.0 / (hi - lo) if hi != lo else 0.0
    shift = -lo * scale
    code = np.trunc((d0.astype(np.float64) * scale + shift).astype(np.float32)).astype(np.uint8)
    return disp, z, code


def center_distance(z: np.ndarray, window: int) -> np.float32:
    H, W = z.shape
    cx, cy, half = W // 2, H // 2, max(1, window // 2)
    patch = z[max(0, cy - half):cy + half + 1, max(0, cx - half):cx + half + 1]
    if np.isnan(patch).all():
        return np.float32(np.nan)
    return np.float32(np.nanmedian(patch))


# ---------------------------------------------------------------------- scenes
def shifted_scene(rng, H, W, d0):
    """left: i.i.d. uint8 texture; right: the left shifted by d0 (left x <-> right x - d0), fresh columns filling in."""
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if d0 < W:
        right[:, :W - d0] = left[:, d0:]
    return left, right


def shifted_bgr_scene(rng, H, W, d0, noise=0):
    """BGR frames of the shifted-texture scene; noise > 0 adds uniform integer noise in [-noise, noise] to the right
    frame, so that the matching costs are not trivially zero."""
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if d0 < W:
        right[:, :W - d0] = left[:, d0:]
    if noise:
        n = rng.integers(-noise, noise + 1, right.shape)
        right = np.clip(right.astype(np.int64) + n, 0, 255).astype(np.uint8)
    return left, right


def crafted_speckle_map(H, W, invalid, window, rng_range):
    """Hand-placed components on an invalid background (needs H >= 31, 8 <= window <= W - 5):
    a snake of more than `window` pixels (kept), a block spanning the rows below it (kept), components of exactly
    window and window + 1 pixels, pairs that differ by exactly 16 * range (joined) and by one more (split), and two
    squares that touch only diagonally."""
    q = np.full((H, W), invalid, dtype=np.int16)
    lim = 16 * rng_range
    # snake: rows 0, 2, 4 joined at alternating ends
    q[0, :] = 160
    q[1, W - 1] = 160
    q[2, :] = 160
    q[3, 0] = 160
    q[4, :] = 160
    # exactly `window` pixels (removed) and window + 1 (kept), one row run each
    assert window <= W - 5 and H >= 31
    q[6, 1:1 + window] = 400
    q[8, 1:2 + window] = 800
    # exact difference: joined at lim, split at lim + 1 (each side alone is <= window pixels)
    half = window // 2 + 1
    q[11, 1:1 + half] = 1000
    q[12, 1:1 + half] = 1000 + lim       # joined: 2 * half > window, kept
    q[14, 1:1 + half] = 2000
    q[15, 1:1 + half] = 2000 + lim + 1   # split: each <= window, removed
    # diagonal touch: two squares of side s, together > window, each <= window
    s = 2
    while 2 * s * s <= window:
        s += 1
    if s * s <= window:
        q[17:17 + s, 1:1 + s] = 3000
        q[17 + s:17 + 2 * s, 1 + s:1 + 2 * s] = 3000
    # a block over the remaining rows and many columns (several thread blocks of pixels), with a gentle ramp
    y0 = 18 + 2 * s
    if y0 < H:
        ramp = (np.arange(W - 3) % 5).astype(np.int16)
        q[y0:, 3:] = 5000 + ramp[None, :]
    return q
