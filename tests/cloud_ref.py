"""NumPy restatement of sd_cloud_build_n (INTEGRATION.md "sd_cloud_build_n"; kernels in csrc/cloud.hip): the fp64
reprojection with every operation rounded on its own, the float32 casts, the keep predicate, the organised cloud and the
packed records in boolean-mask order. The device stage is compared with this bit for bit."""

from __future__ import annotations

import numpy as np

RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                   ("alpha", "u1")])


def reproject(disp: np.ndarray, Q: np.ndarray):
    """disp float32 [H, W], Q float64 [4, 4] -> (xyz float32 [H, W, 3] with a value at every pixel that has one, has
    bool [H, W])."""
    disp = np.asarray(disp, dtype=np.float32)
    Q = np.asarray(Q, dtype=np.float64)
    H, W = disp.shape
    has = np.isfinite(disp) & (disp > 0)
    d = np.where(has, disp, np.float32(1)).astype(np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(all="ignore"):
        R = [((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] for r in range(4)]
        xyz = np.stack([(R[k] / R[3]).astype(np.float32) for k in range(3)], axis=-1)
    return xyz, has


def kept_mask(xyz: np.ndarray, has: np.ndarray, z_range) -> np.ndarray:
    z_min, z_max = np.float32(z_range[0]), np.float32(z_range[1])
    z = xyz[..., 2]
    with np.errstate(invalid="ignore"):
        return has & np.isfinite(xyz).all(axis=-1) & (z_min <= z) & (z <= z_max)


def organized(disp, Q, z_range=(-np.inf, np.inf)) -> np.ndarray:
    """The organised cloud float32 [H, W, 3]: the point of a kept pixel, NaN elsewhere."""
    xyz, has = reproject(disp, Q)
    keep = kept_mask(xyz, has, z_range)
    return np.where(keep[..., None], xyz, np.float32(np.nan)).astype(np.float32)


def records(disp, Q, color=None, bgr=True, z_range=(-np.inf, np.inf), stride=1) -> np.ndarray:
    """All packed records of one stream (RECORD array), uncapped: kept pixels of the stride lattice in ascending (y, x)
    order."""
    xyz, has = reproject(disp, Q)
    keep = kept_mask(xyz, has, z_range)
    H, W = keep.shape
    lattice = np.zeros((H, W), dtype=bool)
    lattice[::stride, ::stride] = True
    m = keep & lattice
    out = np.zeros(int(m.sum()), dtype=RECORD)
    p = xyz[m]  # boolean-mask indexing: ascending (y, x)
    out["x"], out["y"], out["z"] = p[:, 0], p[:, 1], p[:, 2]
    if color is None:
        out["red"] = out["green"] = out["blue"] = 255
    else:
        c = np.asarray(color, dtype=np.uint8)[m]
        if bgr:
            c = c[:, ::-1]
        out["red"], out["green"], out["blue"] = c[:, 0], c[:, 1], c[:, 2]
    out["alpha"] = 255
    return out


def prototype_disparity(H: int, W: int, seed: int = 0) -> np.ndarray:
    """Disparities uniform in [-4, 140) with 10 % NaN and one inf: with tests/golden/sgm_calib.npz's Q and z_range
    (0.3, 10) both branches of every predicate occur."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-4, 140, (H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.1] = np.nan
    d[H // 2, W // 2] = np.inf
    return d
