"""NumPy restatement of the matcher's aggregation modes ("The semi-global matcher", step 5), on top of
the unchanged tests/sgm_ref.py: its recurrence step, winner, left-right check and speckle filter. A path is a direction
(dy, dx); the predecessor of p = (y, x) is q = (y - dy, x - dx), and p starts its path (L = C) exactly when q lies
outside [0, H) x [maxD, W). Vectorised over d and over the lines that run in parallel, a plain loop along the scan.
"""

from __future__ import annotations

import numpy as np

import sgm_ref as R

# mode -> (cv2.StereoSGBM constant, paths)
THREE_WAY = ((1, 0), (0, 1), (0, -1))
MODES = {
    "3way": (2, THREE_WAY),
    "hh4": (3, THREE_WAY + ((-1, 0),)),
    "sgbm": (0, THREE_WAY + ((1, 1), (1, -1))),
    "hh": (1, tuple((dy, dx) for dy in (1, -1) for dx in (-1, 0, 1)) + ((0, 1), (0, -1))),
}


def npaths(mode: str) -> int:
    return len(MODES[mode][1])


def check_bound(p: R.Params, mode: str) -> None:
    """npaths * (bs^2 (2 cap + 63) + P2) <= 65535: per path L <= C + P2, and C <= bs^2 (2 cap + 63)."""
    assert npaths(mode) * (p.bs * p.bs * (2 * p.cap + 63) + p.P2) <= 65535, (mode, p.bs, p.cap, p.P2)


def path(C: np.ndarray, p: R.Params, dy: int, dx: int) -> np.ndarray:
    """L int64 [H, W, D] of the one path (dy, dx); zero for x < maxD."""
    assert (abs(dy), abs(dx)) in ((1, 0), (1, 1), (0, 1))
    H, W, D = C.shape
    L = np.zeros((H, W, D), dtype=np.int64)
    if W <= p.maxD:
        return L
    Cv = C[:, p.maxD:].astype(np.int64)
    Lv = L[:, p.maxD:]
    Wv = Cv.shape[1]
    if dy == 0:  # a column loop; every row is a line
        xs = range(Wv) if dx > 0 else range(Wv - 1, -1, -1)
        prev = np.zeros((H, D), dtype=np.int64)  # zero is the path-start state: the general step gives L = C
        for x in xs:
            prev = R._path_step(prev, Cv[:, x], p.P1, p.P2)
            Lv[:, x] = prev
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    prev = np.zeros((Wv, D), dtype=np.int64)
    for y in ys:  # a row loop; L_prev is shifted by dx, zeros entering where the predecessor is outside
        q = np.zeros_like(prev)
        if dx == 0:
            q = prev
        elif dx > 0:
            q[1:] = prev[:-1]
        else:
            q[:-1] = prev[1:]
        prev = R._path_step(q, Cv[y], p.P1, p.P2)
        Lv[y] = prev
    return L


def aggregate(C: np.ndarray, p: R.Params, mode: str) -> np.ndarray:
    """S uint16 [H, W, D], the sum of the mode's paths; zero for x < maxD."""
    check_bound(p, mode)
    S = np.zeros(C.shape, dtype=np.int64)
    for dy, dx in MODES[mode][1]:
        S += path(C, p, dy, dx)
    assert S.max(initial=0) <= 65535
    return S.astype(np.uint16)


def compute_stages(gray_l: np.ndarray, gray_r: np.ndarray, p: R.Params, mode: str) -> dict:
    pre_l, pre_r = R.prefilter(gray_l, p.cap), R.prefilter(gray_r, p.cap)
    C = R.cost_volume(gray_l, gray_r, pre_l, pre_r, p)
    S = aggregate(C, p, mode)
    q_raw, disp2 = R.winner(S, p)
    q_lr = R.lr_check(q_raw, disp2, p)
    q = R.speckle(q_lr, p.invalid, p.speckle_window, p.speckle_range)
    return {"pre_l": pre_l, "pre_r": pre_r, "C": C, "S": S, "q_raw": q_raw, "disp2": disp2, "q_lr": q_lr, "q": q}


def compute(gray_l, gray_r, p: R.Params, mode: str) -> np.ndarray:
    return compute_stages(gray_l, gray_r, p, mode)["q"]
