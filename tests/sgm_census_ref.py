"""NumPy restatement of the matcher's census / Hamming pixel cost, written from the statement in INTEGRATION.md ("The
census cost": steps 2c and 3c), not from the kernels. Only the two steps that differ from tests/sgm_ref.py are restated
here: the block sum, the winner, the left-right check and the speckle filter are sgm_ref's, the aggregation is sgm_ref's
(3way) or sgm_modes_ref's. All of it is integer arithmetic, so the device path is held to these arrays bit for bit.
"""

from __future__ import annotations

import numpy as np

import sgm_modes_ref as M
import sgm_ref as R
from sgm_ref import block_sum, lr_check, speckle, winner

WINDOWS = ((3, 3), (5, 5), (7, 7), (7, 9))  # (rows, columns)
DEFAULT_WINDOW = (7, 9)


def nbits(window) -> int:
    wh, ww = window
    assert (wh, ww) in WINDOWS, window
    return wh * ww - 1


class Params(R.Params):
    """sgm_ref.Params with the census form of the uint16 bound, npaths * (bs^2 * nbits + P2) <= 65535, in place of the
    Birchfield-Tomasi one. pre_filter_cap is checked as there and otherwise unused."""

    def __init__(self, window=DEFAULT_WINDOW, mode="3way", min_disparity=0, num_disparities=128, block_size=7, P1=None,
                 P2=None, disp12_max_diff=1, uniqueness_ratio=10, speckle_window_size=100, speckle_range=2,
                 pre_filter_cap=31):
        self.window, self.mode, self.nbits = tuple(window), mode, nbits(window)
        self.minD, self.D, self.bs = int(min_disparity), int(num_disparities), int(block_size)
        self.P1 = 8 * self.bs * self.bs if P1 is None else int(P1)
        self.P2 = 32 * self.bs * self.bs if P2 is None else int(P2)
        self.max_diff, self.uniq = int(disp12_max_diff), int(uniqueness_ratio)
        self.speckle_window, self.speckle_range = int(speckle_window_size), int(speckle_range)
        self.cap = int(pre_filter_cap)
        assert self.minD >= 0 and self.D % 16 == 0 and 16 <= self.D <= 256 and self.bs % 2 == 1 and 3 <= self.bs <= 11
        assert 1 <= self.cap <= 63 and 0 <= self.P1 <= self.P2
        check_bound(self, mode)


def check_bound(p, mode: str) -> None:
    """Per path L <= C + P2, and C <= bs^2 * nbits: a pixel cost is a popcount of nbits bits."""
    assert M.npaths(mode) * (p.bs * p.bs * p.nbits + p.P2) <= 65535, (mode, p.bs, p.nbits, p.P2)


# ---------------------------------------------------------------------- step 2c
def census(gray: np.ndarray, wh: int, ww: int) -> np.ndarray:
    """uint64 [H, W]: bit k is set where the k-th window position (row-major, dy outer from -wh/2, dx inner from -ww/2,
    the centre skipped) holds a value strictly below the centre's; edge replication inside the image."""
    assert (wh, ww) in WINDOWS and gray.ndim == 2 and gray.dtype == np.uint8
    H, W = gray.shape
    ry, rx = wh // 2, ww // 2
    g = np.pad(gray.astype(np.int32), ((ry, ry), (rx, rx)), mode="edge")
    centre = gray.astype(np.int32)
    out = np.zeros((H, W), dtype=np.uint64)
    k = 0
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dy == 0 and dx == 0:
                continue
            below = g[ry + dy:ry + dy + H, rx + dx:rx + dx + W] < centre
            out |= below.astype(np.uint64) << np.uint64(k)
            k += 1
    assert k == wh * ww - 1
    return out


# ---------------------------------------------------------------------- step 3c
_M1, _M2, _M4 = np.uint64(0x5555555555555555), np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
_H01 = np.uint64(0x0101010101010101)


def popcount(x: np.ndarray) -> np.ndarray:
    """The set bits of every uint64 (the classic bit-parallel sum; the product wraps modulo 2^64 by design)."""
    x = np.asarray(x, dtype=np.uint64)
    x = x - ((x >> np.uint64(1)) & _M1)
    x = (x & _M2) + ((x >> np.uint64(2)) & _M2)
    x = (x + (x >> np.uint64(4))) & _M4
    with np.errstate(over="ignore"):
        x = x * _H01
    return (x >> np.uint64(56)).astype(np.int32)


def pixel_cost(cl: np.ndarray, cr: np.ndarray, p) -> np.ndarray:
    """Hamming cost int32 [H, W - maxD, D] of the columns x >= maxD: popcount(cl[y][x] ^ cr[y][x - d - minD])."""
    H, W = cl.shape
    xs = np.arange(p.maxD, W)
    out = np.zeros((H, len(xs), p.D), dtype=np.int32)
    for d in range(p.D):
        out[:, :, d] = popcount(cl[:, xs] ^ cr[:, xs - d - p.minD])
    return out


def cost_volume(cl: np.ndarray, cr: np.ndarray, p) -> np.ndarray:
    """C uint16 [H, W, D]; the columns x < maxD are zero (never read)."""
    H, W = cl.shape
    C = np.zeros((H, W, p.D), dtype=np.uint16)
    if W > p.maxD:
        s = block_sum(pixel_cost(cl, cr, p), p.bs)
        assert s.max() <= p.bs * p.bs * p.nbits <= 65535
        C[:, p.maxD:] = s
    return C


# ---------------------------------------------------------------------- the matcher, every stage boundary
def aggregate(C: np.ndarray, p, mode: str) -> np.ndarray:
    check_bound(p, mode)
    if mode == "3way":
        return R.aggregate(C, p)
    S = np.zeros(C.shape, dtype=np.int64)  # sgm_modes_ref.aggregate without its Birchfield-Tomasi bound
    for dy, dx in M.MODES[mode][1]:
        S += M.path(C, p, dy, dx)
    assert S.max(initial=0) <= 65535
    return S.astype(np.uint16)


def compute_stages(gl: np.ndarray, gr: np.ndarray, p, window=None, mode: str = "3way") -> dict:
    wh, ww = p.window if window is None else window
    assert nbits((wh, ww)) == p.nbits
    cl, cr = census(gl, wh, ww), census(gr, wh, ww)
    C = cost_volume(cl, cr, p)
    S = aggregate(C, p, mode)
    q_raw, disp2 = winner(S, p)
    q_lr = lr_check(q_raw, disp2, p)
    q = speckle(q_lr, p.invalid, p.speckle_window, p.speckle_range)
    return {"desc_l": cl, "desc_r": cr, "C": C, "S": S, "q_raw": q_raw, "disp2": disp2, "q_lr": q_lr, "q": q}


def compute(gl, gr, p, window=None, mode: str = "3way") -> np.ndarray:
    return compute_stages(gl, gr, p, window, mode)["q"]


# ---------------------------------------------------------------------- scenes
def monotone_tables(rng, levels=86):
    """Two random strictly increasing maps of 0..levels-1 into 0..255."""
    f, h = (np.sort(rng.choice(256, levels, replace=False)).astype(np.uint8) for _ in range(2))
    return f, h


INVARIANCE_KW = dict(min_disparity=3, num_disparities=48, block_size=5, speckle_window_size=12)


def invariance_scene():
    """The scene of the invariance property: sgm_ref.shifted_scene at 17 x 150 with grays limited to 0..85 and its shift
    inside INVARIANCE_KW's disparity range, and two tables (gl, gr, f, h): compute(f[gl], h[gr]) == compute(gl, gr)."""
    rng = np.random.default_rng(42)
    gl, gr = R.shifted_scene(rng, 17, 150, 3 + 16)
    f, h = monotone_tables(rng)
    return gl // 3, gr // 3, f, h


def levels_scene(rng, H, W, d0, values=(40, 90, 91, 200)):
    """Grays drawn from four values, the right view the left shifted by d0: most window positions tie with the centre,
    so the strict comparison decides the descriptors."""
    v = np.asarray(values, dtype=np.uint8)
    left, right = v[rng.integers(0, len(v), (H, W))], v[rng.integers(0, len(v), (H, W))]
    if d0 < W:
        right[:, :W - d0] = left[:, d0:]
    return left, right
