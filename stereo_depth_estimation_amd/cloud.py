"""Coloured point clouds on the device: reprojection of disparity maps through the calibration's Q, an ordered stream
compaction of the valid, in-range points, and binary PLY files (the reference's classical loop calls
cv2.reprojectImageTo3D and keeps [:, :, 2] only, live_camera/depth_live.py:164-165).

    builder = PointCloudBuilder(streams=4)
    res = builder.build(disparity, Q, color=rect_left, z_range=(0.3, 10.0))   # launches only, no host sync
    counts = res.counts()                                                      # the only sync: 4 * n bytes
    res.save_ply(["rig0.ply", "rig1.ply", "rig2.ply", "rig3.ply"])

    classic.step(frame_l, frame_r); classic.cloud(z_range=(0.3, 10.0)).save_ply(["frame.ply"])

The arithmetic is ``sd_cloud_build_n``'s (include/stereo_hip.h, INTEGRATION.md "sd_cloud_build_n"); it is pinned bit
for bit to the NumPy restatement tests/cloud_ref.py. Kernels: csrc/cloud.hip; the writer: csrc/ply_io.cpp. There is no
CPU fallback for the device stage; the Q helpers, the writer and the reader are host code.
"""

from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _lib as L
from .sgm import reprojection_rows

MAX_STREAMS = 64
MAX_STRIDE = 64
TILE_PIXELS = 1024  # csrc/cloud.hip CLOUD_TILE: pixels per block of the count and scatter passes
SCAN_WIDTH = 256    # csrc/cloud.hip CLOUD_SCAN: tile counts per step of the scan pass

# one packed point, little-endian, 16 bytes: the vertex element of the PLY files
RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                   ("alpha", "u1")])
assert RECORD.itemsize == 16

PLY_PROPERTIES = ("float x", "float y", "float z", "uchar red", "uchar green", "uchar blue", "uchar alpha")


def ply_header(vertices: int) -> bytes:
    """The header of the files ``sd_write_ply_batch`` writes, byte for byte."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(vertices)}"]
    lines += [f"property {p}" for p in PLY_PROPERTIES] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


# ---------------------------------------------------------------------- Q helpers (host, fp64)
def pinhole_Q(focal_px: float, baseline_m: float, cx: float, cy: float) -> np.ndarray:
    """The reprojection matrix of an ideal rectified rig: X = (x - cx) B / d, Y = (y - cy) B / d, Z = f B / d, the
    ``disparity_to_depth`` of the reference's depth_live_dl.py:371-377."""
    f, B = float(focal_px), float(baseline_m)
    if not (math.isfinite(f) and f > 0 and math.isfinite(B) and B > 0):
        raise ValueError(f"pinhole_Q: focal_px and baseline_m must be finite and > 0, got {focal_px}, {baseline_m}")
    if not (math.isfinite(float(cx)) and math.isfinite(float(cy))):
        raise ValueError("pinhole_Q: cx and cy must be finite")
    return np.array([[1.0, 0.0, 0.0, -float(cx)], [0.0, 1.0, 0.0, -float(cy)], [0.0, 0.0, 0.0, f],
                     [0.0, 0.0, 1.0 / B, 0.0]], dtype=np.float64)


def rescale_Q(Q, sx: float, sy: float) -> np.ndarray:
    """Q for an image resized by sx along x and sy along y (resized size / calibration size) whose disparities are in
    pixels of the resized image: Q @ A, A mapping (x', y', d', 1) of the resized image back to calibration pixels on
    half-pixel centres, x = (x' + 0.5) / sx - 0.5, y = (y' + 0.5) / sy - 0.5, d = d' / sx."""
    Q = reprojection_rows(Q)
    sx, sy = float(sx), float(sy)
    if not (math.isfinite(sx) and sx > 0 and math.isfinite(sy) and sy > 0):
        raise ValueError(f"rescale_Q: scales must be finite and > 0, got {sx}, {sy}")
    A = np.array([[1.0 / sx, 0.0, 0.0, 0.5 / sx - 0.5], [0.0, 1.0 / sy, 0.0, 0.5 / sy - 0.5], [0.0, 0.0, 1.0 / sx, 0.0],
                  [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)
    return Q @ A


def stream_matrices(Q, n: int) -> np.ndarray:
    """[4, 4] (for all streams) or [n, 4, 4] -> contiguous float64 [n, 4, 4], each checked by reprojection_rows."""
    Qa = np.asarray(Q, dtype=np.float64)
    if Qa.ndim == 3:
        if Qa.shape != (n, 4, 4):
            raise ValueError(f"Q must be [4, 4] or [n = {n}, 4, 4], got shape {Qa.shape}")
        return np.ascontiguousarray(np.stack([reprojection_rows(q) for q in Qa]))
    return np.ascontiguousarray(np.stack([reprojection_rows(Qa)] * n))


def z_bounds(z_range) -> tuple[float, float]:
    """(z_min, z_max) as the float32 values the kernel compares with; +-inf for no bound, NaN refused."""
    lo, hi = (float(np.float32(v)) for v in z_range)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError("z_range must not hold NaN (use -inf / inf for no bound)")
    if lo > hi:
        raise ValueError(f"z_range must be (min, max) with min <= max, got {tuple(z_range)}")
    return lo, hi


def lattice_size(H: int, W: int, stride: int) -> int:
    """Pixels with x % stride == 0 and y % stride == 0: the most points a stream can pack."""
    return -(-H // stride) * -(-W // stride)


# ---------------------------------------------------------------------- PLY files (host)
def write_ply_batch(paths, points_host, counts, threads: int = 16) -> None:
    """Native (``sd_write_ply_batch``) write of n clouds. points_host: the records [n, cap] as a contiguous CPU uint8
    tensor or array [n, cap, 16] (or a RECORD array [n, cap]); counts: n unsigned integers, file i holds the first
    min(counts[i], cap) records. Each file appears under its name complete or not at all (temporary file + rename); the
    parent directories must exist. OSError names the first path that failed; the other files are still written."""
    n = len(paths)
    if isinstance(points_host, torch.Tensor):
        if points_host.device.type != "cpu":
            raise ValueError("write_ply_batch: points_host must be in host memory")
        points_host = points_host.numpy()
    a = np.asarray(points_host)
    if a.dtype == RECORD and a.ndim == 2:
        a = a.view(np.uint8).reshape(a.shape[0], a.shape[1], 16)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[0] != n or a.shape[1] < 1 or a.shape[2] != 16 \
            or not a.flags.c_contiguous:
        raise ValueError(f"write_ply_batch: expected contiguous uint8 records [n = {n}, cap >= 1, 16], got {a.dtype} "
                         f"{a.shape}")
    c = np.ascontiguousarray(np.asarray(counts).astype(np.uint32).reshape(-1))
    if c.shape != (n,):
        raise ValueError(f"write_ply_batch: {n} paths but {c.size} counts")
    arr = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(str(p)) for p in paths])
    err = ctypes.create_string_buffer(1024)
    rc = L.load().sd_write_ply_batch(ctypes.cast(arr, ctypes.c_void_p), n, a.ctypes.data, a.shape[1], c.ctypes.data,
                                     int(threads), err, len(err))
    if rc != 0:
        raise OSError(f"PLY file could not be written: {err.value.decode(errors='replace')}")


def read_ply(path) -> np.ndarray:
    """The vertices of a file ``write_ply_batch`` wrote, as a RECORD array. A reader of exactly that header: anything
    else raises ValueError."""
    data = open(path, "rb").read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    head = data[:end + len(b"end_header\n")]
    lines = head.decode("ascii", errors="replace").split("\n")
    try:
        kind, name, num = lines[2].split(" ")
        vertices = int(num)
    except (IndexError, ValueError):
        raise ValueError(f"{path}: not a PLY header of this writer") from None
    if kind != "element" or name != "vertex" or vertices < 0 or head != ply_header(vertices):
        raise ValueError(f"{path}: not a PLY header of this writer")
    body = data[len(head):]
    if len(body) != vertices * RECORD.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes after the header, {vertices} vertices need "
                         f"{vertices * RECORD.itemsize}")
    return np.frombuffer(body, dtype=RECORD).copy()


# ---------------------------------------------------------------------- the device stage
class CloudResult:
    """Device tensors of one ``build`` (views of the builder's buffers: its next build overwrites them).

    points: uint8 [n, cap, 16], RECORD bytes; only the first min(count, cap) records of a stream are defined.
    xyz:    float32 [n, H, W, 3], NaN where a pixel is not kept, or None."""

    __slots__ = ("points", "xyz", "cap", "_count", "_pin", "_device")

    def __init__(self, points, xyz, count, pin, device):
        self.points, self.xyz, self.cap = points, xyz, int(points.shape[1])
        self._count, self._pin, self._device = count, pin, device

    def counts(self) -> np.ndarray:
        """uint32 [n]: the kept lattice points of each stream, whether or not they fit ``cap``. One 4 * n-byte copy
        through a pinned buffer and the only host synchronisation."""
        n = self._count.shape[0]
        self._pin[:n].copy_(self._count, non_blocking=True)
        torch.cuda.current_stream(self._device).synchronize()
        return self._pin[:n].numpy().view(np.uint32).copy()

    def numpy(self, i: int) -> np.ndarray:
        """Stream i's records as a RECORD array of min(count, cap) points."""
        c = self.counts()
        k = min(int(c[i]), self.cap)
        return self.points[i, :k].cpu().numpy().reshape(-1).view(RECORD).copy()

    def save_ply(self, paths, threads: int = 16) -> np.ndarray:
        """One binary PLY file per stream (``write_ply_batch``); returns the counts."""
        if len(paths) != self.points.shape[0]:
            raise ValueError(f"save_ply: {self.points.shape[0]} streams but {len(paths)} paths")
        c = self.counts()
        write_ply_batch(paths, self.points.cpu(), c, threads)
        return c


class PointCloudBuilder:
    """``sd_cloud_build_n`` with its buffers: up to ``streams`` (1..64) maps of one size per call, one launch per pass
    whatever their number. Buffers are made once per size and only grow; ``build`` issues launches only."""

    def __init__(self, streams: int = 1, device="cuda"):
        n = int(streams)
        if not 1 <= n <= MAX_STREAMS:
            raise ValueError(f"streams must be in [1, {MAX_STREAMS}], got {streams}")
        self.streams = n
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PointCloudBuilder runs only on a HIP device (no CPU path), got {device}")
        self._points = self._xyz = self._work = self._count = self._pin = self._Qdev = None
        self._Qhost = None

    def _matrices(self, Q, n: int) -> torch.Tensor:
        """Qdev f64 [n, 16]. A float64 device tensor [n, 16] / [n, 4, 4] is taken as it is (the caller checked it); host
        matrices are checked and uploaded when they differ from the last call's."""
        if isinstance(Q, torch.Tensor) and Q.is_cuda:
            if Q.dtype != torch.float64 or Q.numel() != n * 16 or not Q.is_contiguous() or Q.device != self.device:
                raise ValueError(f"a device Q must be a contiguous float64 [n = {n}, 16] tensor on {self.device}")
            return Q
        if isinstance(Q, torch.Tensor):
            Q = Q.numpy()
        Qh = stream_matrices(Q, n)
        if self._Qhost is None or self._Qhost.shape != Qh.shape or not np.array_equal(self._Qhost, Qh):
            with torch.inference_mode(False):
                self._Qdev = torch.as_tensor(Qh.reshape(n, 16)).to(self.device)
            self._Qhost = Qh
        return self._Qdev

    def build(self, disparity: torch.Tensor, Q, color: torch.Tensor | None = None, bgr: bool = True,
              z_range=(-math.inf, math.inf), stride: int = 1, organized: bool = False, cap: int | None = None
              ) -> CloudResult:
        """disparity: float32 [n, H, W] on the device (n <= streams), NaN / <= 0 / inf where there is no value. Q: the
        4 x 4 reprojection matrix for all streams or [n, 4, 4] (host), or a float64 device tensor [n, 16]. color: uint8
        [n, H, W, 3], BGR when ``bgr`` else RGB; None: white points. z_range: kept depths (float32, inclusive).
        stride: pack every stride-th pixel in x and y. organized: also the [n, H, W, 3] float32 point image. cap:
        records per stream (default: the lattice size, so nothing is dropped)."""
        if not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.float32 or disparity.dim() != 3 \
                or not disparity.is_cuda:
            raise ValueError("build takes a float32 [n, H, W] device tensor")
        if self.device.index is None:
            self.device = torch.device("cuda", disparity.device.index)
        if disparity.device != self.device:
            raise ValueError(f"disparity is on {disparity.device}, the builder on {self.device}")
        n, H, W = (int(v) for v in disparity.shape)
        if not 1 <= n <= self.streams:
            raise ValueError(f"build takes 1..{self.streams} streams, got {n}")
        if H * W >= 2 ** 31 or H < 1 or W < 1:
            raise ValueError(f"bad size {H} x {W}")
        stride = int(stride)
        if not 1 <= stride <= MAX_STRIDE:
            raise ValueError(f"stride must be in [1, {MAX_STRIDE}], got {stride}")
        if color is not None and (not isinstance(color, torch.Tensor) or color.dtype != torch.uint8
                                  or tuple(color.shape) != (n, H, W, 3) or color.device != self.device):
            raise ValueError(f"color must be a uint8 tensor of {(n, H, W, 3)} on {self.device}")
        z_min, z_max = z_bounds(z_range)
        cap = lattice_size(H, W, stride) if cap is None else int(cap)
        if cap < 1:
            raise ValueError(f"cap must be >= 1, got {cap}")
        disparity = disparity.contiguous()
        color = color.contiguous() if color is not None else None
        with torch.cuda.device(self.device):
            Qdev = self._matrices(Q, n)
            points = L.grow(self, "_points", n * cap * 16, torch.uint8)[:n * cap * 16].view(n, cap, 16)
            xyz = L.grow(self, "_xyz", n * H * W * 3, torch.float32)[:n * H * W * 3].view(n, H, W, 3) if organized \
                else None
            work = L.grow(self, "_work", L.call("sd_cloud_ws_bytes", n, H, W, stride) // 4, torch.int32)
            count = L.grow(self, "_count", self.streams, torch.int32)[:n]
            if self._pin is None:
                self._pin = torch.zeros(MAX_STREAMS, dtype=torch.int32).pin_memory()
            L.call("sd_cloud_build_n", n, disparity.data_ptr(), L.ptr(color), int(bool(bgr)), H, W, Qdev.data_ptr(),
                   z_min, z_max, stride, L.ptr(xyz), points.data_ptr(), cap, count.data_ptr(), work.data_ptr(),
                   L.stream_handle(self.device))
        return CloudResult(points, xyz, count, self._pin, self.device)
