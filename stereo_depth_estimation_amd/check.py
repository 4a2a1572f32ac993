"""A label-free check of disparity maps on the device: the visibility class of every pixel (no value, out of view,
occluded, visible) and, with the two rectified frames, the photometric residual after warping the right frame onto the
left (no counterpart in the reference).

    chk = StereoCheck(streams=4)
    res = chk.run(disparity, left=rect_left, right=rect_right, photo_thr=120.0)   # launches only, no host sync
    for s in res.summary():                                                        # the only sync: 64 * n bytes
        print(s["visible"] / max(s["valued"], 1), s["photo_l1"])
    cloud = builder.build(res.disp_vis, Q, color=rect_left)                        # no flying points

    # geometry only (no frames at the map's size, e.g. LiveDepthBatch): classes 0..3, no residual
    cloud = builder.build(StereoCheck(n).run(live_res.disparity).disp_vis, Q)

The arithmetic is ``sd_stereo_check``'s (include/stereo_hip.h, INTEGRATION.md "sd_stereo_check"); it is pinned bit for
bit to the NumPy restatement tests/check_ref.py. Kernels: csrc/check.hip. There is no CPU fallback.

The frames are taken as rectified: a pixel (x, y) of the left frame is looked for at (x - d, y) of the right frame.
The defaults, ``occ_tol`` = 0.5 px and no photometric threshold, are parameters and not measured optima: the tolerance
that separates a slanted surface from an occlusion, and the residual that separates a wrong match from a change of
exposure, depend on the rig and the scene.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

MAX_SAMPLES = 65535
SCAN_PIXELS = 1024  # csrc/check.hip CHECK_SCAN: pixels per step of the right-to-left row walk
ROW = 8             # doubles per sample: values, out of view, occluded, counted, sum e, sum e^2, mismatch, 0
OUTPUTS = ("cls", "resid", "disp_vis", "vis_rgb", "rows")
CLASSES = ("visible", "no_value", "out_of_view", "occluded", "mismatch")  # the codes 0..4 of ``cls``
SUMMARY_KEYS = ("valued", "out_of_view", "occluded", "visible", "mismatch", "photo_l1", "photo_rms")


@dataclass(frozen=True)
class CheckOptions:
    """What ``--self-check`` asks for: the parameters of the stage (as the float32 values the kernel compares with)
    and which of the optional products predict makes from it."""
    occ_tol: float = 0.5
    photo_thr: float = math.inf
    write_check: bool = False
    ply_visible_only: bool = False

    def describe(self) -> dict:
        """The check arguments as ``predict_meta.json`` records them."""
        return {"self_check": True, "check_occ_tol": float(self.occ_tol),
                "check_photo_thr": float(self.photo_thr) if math.isfinite(self.photo_thr) else None,
                "write_check": bool(self.write_check), "ply_visible_only": bool(self.ply_visible_only)}


def check_params(occ_tol, photo_thr) -> tuple[float, float]:
    """(occ_tol, photo_thr) as float32 values: occ_tol finite and >= 0; photo_thr +inf for none, NaN refused."""
    tol, thr = float(np.float32(occ_tol)), float(np.float32(photo_thr))
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f"occ_tol must be finite and >= 0, got {occ_tol}")
    if math.isnan(thr):
        raise ValueError("photo_thr must not be NaN (inf for no mismatch class)")
    return tol, thr


def check_options(self_check: bool = False, output_root=None, write_ply: bool = False, check_occ_tol=None,
                  check_photo_thr=None, write_check: bool = False, ply_visible_only: bool = False
                  ) -> CheckOptions | None:
    """The ``--self-check`` flags checked and gathered; None without the flag (the other flags then must be unset).
    ``--write-check`` needs ``--output-root``, ``--ply-visible-only`` needs ``--write-ply``."""
    given = [k for k, v in (("--check-occ-tol", check_occ_tol is not None), ("--check-photo-thr", check_photo_thr is not None),
                            ("--write-check", bool(write_check)), ("--ply-visible-only", bool(ply_visible_only))) if v]
    if not self_check:
        if given:
            raise ValueError(f"{', '.join(given)}: only with --self-check.")
        return None
    if write_check and output_root is None:
        raise ValueError("--write-check needs --output-root.")
    if ply_visible_only and not write_ply:
        raise ValueError("--ply-visible-only needs --write-ply.")
    try:
        tol, thr = check_params(0.5 if check_occ_tol is None else check_occ_tol,
                                math.inf if check_photo_thr is None else check_photo_thr)
    except ValueError as e:
        raise ValueError(f"--check-occ-tol / --check-photo-thr: {e}") from None
    return CheckOptions(tol, thr, bool(write_check), bool(ply_visible_only))


def summary_from_row(row) -> dict:
    """The figures of one row (or of a sum of rows) in fp64. ``visible`` counts class 0 alone; ``photo_l1`` is the mean
    absolute residual per channel in codes, sum e / (3 * rows[3]), ``photo_rms`` sqrt(sum e^2 / rows[3]) / 3, both over
    classes 0 and 4 and None when nothing counted (no frames, or no pixel survived)."""
    r = [float(v) for v in row]
    counted = r[3]
    out = {"valued": int(r[0]), "out_of_view": int(r[1]), "occluded": int(r[2]),
           "visible": int(r[0] - r[1] - r[2] - r[6]), "mismatch": int(r[6]),
           "photo_l1": None, "photo_rms": None}
    if counted > 0:
        out.update(photo_l1=r[4] / (3.0 * counted), photo_rms=math.sqrt(r[5] / counted) / 3.0)
    return out


def aggregate_rows(rows) -> dict:
    """Pixel-weighted figures over samples: the rows [N][8] summed column-wise in fp64, then ``summary_from_row``."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    return summary_from_row(rows.sum(axis=0))


class CheckResult:
    """Device tensors of one ``run`` (views of the checker's buffers: its next run overwrites them); None for an output
    that was not asked for.

    cls:      uint8 [n, H, W], the codes of ``CLASSES``
    resid:    float32 [n, H, W], the residual e of classes 0 and 4, NaN elsewhere
    disp_vis: float32 [n, H, W], the disparity of class 0, NaN elsewhere (what ``PointCloudBuilder.build`` takes)
    vis_rgb:  uint8 [n, H, W, 3], the picture of the check
    rows:     float64 [n, 8]"""

    __slots__ = ("cls", "resid", "disp_vis", "vis_rgb", "rows", "_pin", "_device")

    def __init__(self, cls, resid, disp_vis, vis_rgb, rows, pin, device):
        self.cls, self.resid, self.disp_vis, self.vis_rgb, self.rows = cls, resid, disp_vis, vis_rgb, rows
        self._pin, self._device = pin, device

    def summary(self) -> list[dict]:
        """Per-sample dicts of ``SUMMARY_KEYS``. One copy of ``rows`` through a pinned buffer and the only host
        synchronisation."""
        if self.rows is None:
            raise ValueError("summary needs the rows output (want=(..., 'rows'))")
        n = self.rows.shape[0]
        self._pin[:n].copy_(self.rows, non_blocking=True)
        torch.cuda.current_stream(self._device).synchronize()
        return [summary_from_row(r) for r in self._pin[:n].numpy().copy()]


class StereoCheck:
    """``sd_stereo_check`` with its buffers: up to ``streams`` (1..65535) maps of one size per call, two launches at most
    whatever their number. Buffers are made once per size and only grow; ``run`` issues launches only."""

    def __init__(self, streams: int = 1, device="cuda"):
        n = int(streams)
        if not 1 <= n <= MAX_SAMPLES:
            raise ValueError(f"streams must be in [1, {MAX_SAMPLES}], got {streams}")
        self.streams = n
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"StereoCheck runs only on a HIP device (no CPU path), got {device}")
        self._cls = self._resid = self._disp_vis = self._vis_rgb = self._rows = self._work = self._pin = None

    def run(self, disp: torch.Tensor, left: torch.Tensor | None = None, right: torch.Tensor | None = None,
            occ_tol: float = 0.5, photo_thr: float = math.inf, want=None) -> CheckResult:
        """disp: float32 [n, H, W] on the device (n <= streams), the left view's disparity in pixels of these frames,
        NaN / <= 0 / inf where there is no value. left, right: uint8 [n, H, W, 3], rectified frames of that size in any
        colour order (the same in both), or both None: classes 0..3 only. occ_tol: pixels by which a nearer pixel must
        overtake before the one behind counts as occluded (0.5 by default, a parameter, not a measured optimum).
        photo_thr: the residual e (codes summed over the three channels, 0..765) above which a visible pixel becomes a
        mismatch; inf (the default): no such class. want: the outputs of ``OUTPUTS`` to make; by default all that the
        inputs allow (``resid`` and ``vis_rgb`` need frames)."""
        if not isinstance(disp, torch.Tensor) or disp.dtype != torch.float32 or disp.dim() != 3 or not disp.is_cuda:
            raise ValueError("run takes a float32 [n, H, W] device tensor")
        if self.device.index is None:
            self.device = torch.device("cuda", disp.device.index)
        if disp.device != self.device:
            raise ValueError(f"disp is on {disp.device}, the checker on {self.device}")
        n, H, W = (int(v) for v in disp.shape)
        if not 1 <= n <= self.streams:
            raise ValueError(f"run takes 1..{self.streams} samples, got {n}")
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"bad size {H} x {W}")
        if (left is None) != (right is None):
            raise ValueError("left and right: give both or neither")
        for name, t in (("left", left), ("right", right)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8
                                  or tuple(t.shape) != (n, H, W, 3) or t.device != self.device):
                raise ValueError(f"{name} must be a uint8 tensor of {(n, H, W, 3)} on {self.device}")
        frames = left is not None
        if want is None:
            want = OUTPUTS if frames else ("cls", "disp_vis", "rows")
        want = tuple(want)
        if not want or any(w not in OUTPUTS for w in want):
            raise ValueError(f"want must name at least one of {OUTPUTS}, got {want}")
        if not frames and ("resid" in want or "vis_rgb" in want):
            raise ValueError("resid and vis_rgb need the frames")
        tol, thr = check_params(occ_tol, photo_thr)
        disp = disp.contiguous()
        left, right = (left.contiguous(), right.contiguous()) if frames else (None, None)
        px = n * H * W
        with torch.cuda.device(self.device):
            cls = L.grow(self, "_cls", px, torch.uint8)[:px].view(n, H, W) if "cls" in want else None
            resid = L.grow(self, "_resid", px, torch.float32)[:px].view(n, H, W) if "resid" in want else None
            dvis = L.grow(self, "_disp_vis", px, torch.float32)[:px].view(n, H, W) if "disp_vis" in want else None
            vis = L.grow(self, "_vis_rgb", px * 3, torch.uint8)[:px * 3].view(n, H, W, 3) if "vis_rgb" in want else None
            rows = work = None
            if "rows" in want:
                rows = L.grow(self, "_rows", self.streams * ROW, torch.float64)[:n * ROW].view(n, ROW)
                work = L.grow(self, "_work", L.call("sd_stereo_check_ws_bytes", n, H, W) // 8, torch.float64)
                if self._pin is None:
                    self._pin = torch.zeros(self.streams, ROW, dtype=torch.float64).pin_memory()
            L.call("sd_stereo_check", n, disp.data_ptr(), L.ptr(left), L.ptr(right), H, W, tol, thr, L.ptr(cls),
                   L.ptr(resid), L.ptr(dvis), L.ptr(vis), L.ptr(rows), L.ptr(work), L.stream_handle(self.device))
        return CheckResult(cls, resid, dvis, vis, rows, self._pin, self.device)
