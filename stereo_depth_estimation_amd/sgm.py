"""The classical live loop on the device (the reference's live_camera/depth_live.py:138-191 without capture, windows
and text): rectification, gray, a semi-global matcher, reprojection, the centre distance and the colour image.

    matcher = StereoSGM(num_disparities=128, block_size=7)
    q = matcher.compute(gray_l, gray_r)        # int16 [H, W], 16 * disparity: the counterpart of matcher.compute

    classic = ClassicDepth(rectification=calib.rectification, Q=Q)
    res = classic.step(frame_l, frame_r)       # no host sync: device tensors, overwritten by the next step
    dist_m = res.readout()                     # the only host sync (4 bytes)

    rigs = ClassicDepthBatch(4, rectification=[r0, r1, r2, r3], Q=Qs)   # n rigs of one size, one launch per stage
    dists = rigs.step(frames_l, frames_r).readout()                      # float32 [4]; StereoSGM.compute_batch alone

The matcher follows OpenCV's StereoSGBM step by step (three paths by default; mode="hh4" / "sgbm" / "hh" add the
bottom-up path, the two downward diagonals or all eight) and is pinned bit for bit to the NumPy restatements
tests/sgm_ref.py and tests/sgm_modes_ref.py, not to cv2's bytes; what is stated rather than taken from OpenCV is
listed in INTEGRATION.md. Kernels: csrc/sgm.hip. There is no CPU fallback.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .live import MAX_CENTER_WINDOW, MAX_STREAMS, colormap_lut

MAX_WIDTH = 4096  # the winner kernel keeps a row's right-view state in LDS

# mode name -> (cv2.StereoSGBM constant = SD_SGM_MODE_*, paths summed into S)
MODES = {"3way": (L.SD_SGM_MODE_3WAY, 3), "hh4": (L.SD_SGM_MODE_HH4, 4), "sgbm": (L.SD_SGM_MODE_SGBM, 5),
         "hh": (L.SD_SGM_MODE_HH, 8)}


def mode_name(mode) -> str:
    """One of MODES' names from a name or from cv2's integer constant (MODE_SGBM 0, MODE_HH 1, MODE_SGBM_3WAY 2,
    MODE_HH4 3)."""
    if isinstance(mode, str) and mode in MODES:
        return mode
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool):
        for name, (const, _) in MODES.items():
            if const == int(mode):
                return name
    raise ValueError(f"mode must be one of {sorted(MODES)} or cv2's constants 0 (sgbm), 1 (hh), 2 (3way), 3 (hh4), "
                     f"got {mode!r}")


def ws_bytes(H: int, W: int, D: int) -> int:
    """sd_sgm_ws_bytes as a formula: two uint16 volumes, two prefiltered planes, the speckle filter's two int32 planes,
    each rounded up to 256 bytes."""
    def a(v):
        return (v + 255) // 256 * 256

    return 2 * a(2 * H * W * D) + 2 * a(H * W) + 2 * a(4 * H * W)


def reprojection_rows(Q) -> np.ndarray:
    """The 4 x 4 disparity-to-depth matrix of cv2.stereoRectify as a contiguous float64 array (rows 2 and 3 give z)."""
    Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
    if Q.shape != (4, 4):
        raise ValueError(f"Q must be the 4 x 4 reprojection matrix, got shape {Q.shape}")
    if not np.isfinite(Q).all():
        raise ValueError("Q must be finite")
    if not Q[3].any():
        raise ValueError("Q's last row is zero: z = row 2 / row 3 would be undefined everywhere")
    return Q


class StereoSGM:
    """cv2.StereoSGBM.create(..., mode=MODE_SGBM_3WAY) of depth_live.py:67-83, parameters by the same names. mode: "3way"
    (the application's), "hh4", "sgbm" or "hh", or cv2's integer constant."""

    def __init__(self, min_disparity=0, num_disparities=128, block_size=7, P1=None, P2=None, disp12_max_diff=1,
                 uniqueness_ratio=10, speckle_window_size=100, speckle_range=2, pre_filter_cap=31, mode="3way"):
        self.mode = mode_name(mode)
        self.mode_id, npaths = MODES[self.mode]
        minD, D, bs = int(min_disparity), int(num_disparities), int(block_size)
        if D % 16 != 0:
            raise ValueError("--num-disparities must be a multiple of 16.")
        if bs % 2 == 0 or bs < 3:
            raise ValueError("--block-size must be odd and >= 3.")
        if not 16 <= D <= 256:
            raise ValueError("num_disparities must be in [16, 256]")
        if bs > 11:
            raise ValueError("block_size must be <= 11")
        if minD < 0:
            raise ValueError("min_disparity must be >= 0")
        P1 = 8 * bs * bs if P1 is None else int(P1)
        P2 = 32 * bs * bs if P2 is None else int(P2)
        cap = int(pre_filter_cap)
        if not 1 <= cap <= 63:
            raise ValueError("pre_filter_cap must be in [1, 63]")
        if P1 < 0 or P2 < P1:
            raise ValueError("0 <= P1 <= P2 required")
        if npaths * (bs * bs * (2 * cap + 63) + P2) > 65535:
            raise ValueError(f"{npaths} * (block_size^2 * (2 * pre_filter_cap + 63) + P2) = "
                             f"{npaths * (bs * bs * (2 * cap + 63) + P2)} exceeds 65535: the cost sums of the "
                             f"{npaths} paths of mode {self.mode!r} would not fit uint16")
        if not 0 <= int(uniqueness_ratio) <= 100:
            raise ValueError("uniqueness_ratio must be in [0, 100]")
        if int(speckle_window_size) < 0 or not 0 <= int(speckle_range) <= 1024:
            raise ValueError("speckle_window_size >= 0 and speckle_range in [0, 1024] required")
        self.min_disparity, self.num_disparities, self.block_size = minD, D, bs
        self.P1, self.P2, self.pre_filter_cap = P1, P2, cap
        self.disp12_max_diff, self.uniqueness_ratio = int(disp12_max_diff), int(uniqueness_ratio)
        self.speckle_window_size, self.speckle_range = int(speckle_window_size), int(speckle_range)
        self._ws = None
        self._ws_key = None
        self._ws_n = None
        self._ws_n_key = None

    @property
    def invalid_value(self) -> int:
        return 16 * (self.min_disparity - 1)

    def params(self) -> tuple:
        """The integer arguments of sd_sgm_compute, in its order (sd_sgm_compute_mode takes mode_id after them)."""
        return (self.min_disparity, self.num_disparities, self.block_size, self.P1, self.P2, self.disp12_max_diff,
                self.uniqueness_ratio, self.speckle_window_size, self.speckle_range, self.pre_filter_cap)

    def workspace(self, device, H: int, W: int) -> torch.Tensor:
        key = (device, H, W)
        if self._ws_key != key:
            n = L.call("sd_sgm_ws_bytes", H, W, self.num_disparities)
            with torch.inference_mode(False):
                self._ws = torch.empty(n, dtype=torch.uint8, device=device)
            self._ws_key = key
        return self._ws

    def compute(self, gray_l: torch.Tensor, gray_r: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 [H, W] device tensors -> int16 [H, W] (16 * disparity; invalid_value where there is none). Launches
        only; the workspace is allocated once per (device, size)."""
        for g in (gray_l, gray_r):
            if not isinstance(g, torch.Tensor) or g.dtype != torch.uint8 or g.dim() != 2 or not g.is_cuda:
                raise ValueError("compute takes two uint8 [H, W] device tensors")
        if gray_l.shape != gray_r.shape or gray_l.device != gray_r.device:
            raise ValueError("both images must have one size and one device")
        H, W = int(gray_l.shape[0]), int(gray_l.shape[1])
        if W > MAX_WIDTH:
            raise ValueError(f"width {W} exceeds {MAX_WIDTH}")
        gray_l, gray_r = gray_l.contiguous(), gray_r.contiguous()
        if out is None:
            out = torch.empty((H, W), dtype=torch.int16, device=gray_l.device)
        elif out.dtype != torch.int16 or tuple(out.shape) != (H, W) or not out.is_contiguous() \
                or out.device != gray_l.device:
            raise ValueError("out must be a contiguous int16 [H, W] tensor on the images' device")
        ws = self.workspace(gray_l.device, H, W)
        with torch.cuda.device(gray_l.device):
            if self.mode == "3way":
                L.call("sd_sgm_compute", gray_l.data_ptr(), gray_r.data_ptr(), H, W, *self.params(), ws.data_ptr(),
                       out.data_ptr(), L.stream_handle(gray_l.device))
            else:
                L.call("sd_sgm_compute_mode", gray_l.data_ptr(), gray_r.data_ptr(), H, W, *self.params(), self.mode_id,
                       ws.data_ptr(), out.data_ptr(), L.stream_handle(gray_l.device))
        return out

    def workspace_batch(self, device, n: int, H: int, W: int) -> torch.Tensor:
        """n slices of the single-stream workspace (sd_sgm_ws_bytes_n: n x 160 MB at 640 x 480, D = 128)."""
        key = (device, n, H, W)
        if self._ws_n_key != key:
            size = L.call("sd_sgm_ws_bytes_n", n, H, W, self.num_disparities)
            if size < 0:
                raise ValueError(f"streams must be in [1, {MAX_STREAMS}], got {n}")
            with torch.inference_mode(False):
                self._ws_n = torch.empty(size, dtype=torch.uint8, device=device)
            self._ws_n_key = key
        return self._ws_n

    def compute_batch(self, gray_l: torch.Tensor, gray_r: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 [n, H, W] device tensors (n stereo pairs of one size) -> int16 [n, H, W]: compute() for every pair,
        byte for byte, in one launch per stage whatever n is. Launches only; the workspace is allocated once per
        (device, n, size)."""
        for g in (gray_l, gray_r):
            if not isinstance(g, torch.Tensor) or g.dtype != torch.uint8 or g.dim() != 3 or not g.is_cuda:
                raise ValueError("compute_batch takes two uint8 [n, H, W] device tensors")
        if gray_l.shape != gray_r.shape or gray_l.device != gray_r.device:
            raise ValueError("both image sets must have one shape and one device")
        n, H, W = (int(v) for v in gray_l.shape)
        if not 1 <= n <= MAX_STREAMS:
            raise ValueError(f"streams must be in [1, {MAX_STREAMS}], got {n}")
        if W > MAX_WIDTH:
            raise ValueError(f"width {W} exceeds {MAX_WIDTH}")
        gray_l, gray_r = gray_l.contiguous(), gray_r.contiguous()
        if out is None:
            out = torch.empty((n, H, W), dtype=torch.int16, device=gray_l.device)
        elif out.dtype != torch.int16 or tuple(out.shape) != (n, H, W) or not out.is_contiguous() \
                or out.device != gray_l.device:
            raise ValueError("out must be a contiguous int16 [n, H, W] tensor on the images' device")
        ws = self.workspace_batch(gray_l.device, n, H, W)
        with torch.cuda.device(gray_l.device):
            L.call("sd_sgm_compute_n", n, gray_l.data_ptr(), gray_r.data_ptr(), H, W, *self.params(), self.mode_id,
                   ws.data_ptr(), out.data_ptr(), L.stream_handle(gray_l.device))
        return out


class ClassicResult:
    """Device tensors of one step (views of ClassicDepth's buffers: the next step overwrites them)."""

    __slots__ = ("disparity_q4", "disparity", "depth_m", "rect_left", "rect_right", "disp_vis", "_owner")

    def __init__(self, owner, **kw):
        self._owner = owner
        for k, v in kw.items():
            setattr(self, k, v)

    def readout(self) -> float:
        """The centre distance in metres (np.nanmedian of the centre patch of depth_m; NaN when it has no value): one
        4-byte copy and the only host synchronisation of the frame path."""
        return self._owner._readout()


class ClassicDepth:
    def __init__(self, rectification=None, Q=None, center_window=15, colormap="turbo", device="cuda", **matcher_kw):
        """rectification: an object with the reference's map attributes (map_l_1, map_l_2, map_r_1, map_r_2,
        image_size), e.g. load_calibration(path).rectification, or None (frames are taken as rectified). Q: the
        4 x 4 reprojection matrix of the calibration file. colormap: a name of live.COLORMAP_NAMES or a [256, 3]
        uint8 BGR table. matcher_kw: StereoSGM's parameters."""
        if Q is None:
            raise ValueError("ClassicDepth needs the calibration's reprojection matrix Q")
        self.Q = reprojection_rows(Q)
        if not 0 <= int(center_window) <= MAX_CENTER_WINDOW:
            raise ValueError(f"center_window must be in [0, {MAX_CENTER_WINDOW}]")
        self.center_window = int(center_window)
        self.matcher = StereoSGM(**matcher_kw)
        self.rectification = rectification
        lut = colormap_lut(colormap) if isinstance(colormap, str) else np.asarray(colormap)
        if lut.shape != (256, 3) or lut.dtype != np.uint8:
            raise ValueError("colormap: a name or a [256, 3] uint8 BGR table")
        self._lut_host = np.ascontiguousarray(lut)
        self.device = torch.device(device)
        self._buf = None
        self._key = None
        self._stage_i = 0

    # ------------------------------------------------------------------ buffers
    def _alloc(self, H: int, W: int):
        device = self.device
        with torch.inference_mode(False):
            def dev(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=device)

            b = {
                "rect": dev((2, H, W, 3), torch.uint8), "gray": dev((2, H, W), torch.uint8),
                "q": dev((H, W), torch.int16), "disp": dev((H, W), torch.float32), "z": dev((H, W), torch.float32),
                "code": dev((H, W), torch.uint8), "vis": dev((H, W, 3), torch.uint8),
                "minmax": torch.zeros(2, dtype=torch.int32, device=device), "center": dev((1,), torch.float32),
                "lut": torch.as_tensor(self._lut_host).to(device),
                "pin": [torch.empty((2, H, W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(3)],
                "pin_ev": [None, None, None],
                "frames": [dev((2, H, W, 3), torch.uint8) for _ in range(3)],
                "center_host": torch.full((1,), float("nan"), dtype=torch.float32, pin_memory=True),
            }
            r = self.rectification
            if r is not None:
                for side in ("l", "r"):
                    m1 = np.ascontiguousarray(getattr(r, f"map_{side}_1"))
                    m2 = np.ascontiguousarray(getattr(r, f"map_{side}_2"))
                    if m1.shape != (H, W, 2) or m1.dtype != np.int16 or m2.shape != (H, W) or m2.dtype != np.uint16:
                        raise ValueError("rectification maps: map1 int16 [H, W, 2] and map2 uint16 [H, W] "
                                         "(cv2.initUndistortRectifyMap(..., cv2.CV_16SC2) or live.rectify_maps)")
                    b[f"m1{side}"] = torch.as_tensor(m1).to(device)
                    b[f"m2{side}"] = torch.as_tensor(m2.view(np.int16)).to(device)
        self.matcher.workspace(device, H, W)
        self._buf, self._key = b, (H, W)

    def _frames(self, frame_l, frame_r):
        """Both frames on the device, uint8 [H, W, 3]. numpy frames: pinned staging, non_blocking copies."""
        if isinstance(frame_l, torch.Tensor) != isinstance(frame_r, torch.Tensor):
            raise TypeError("both frames must be numpy arrays or both device tensors")
        shape = tuple(frame_l.shape)
        if len(shape) != 3 or shape[2] != 3 or tuple(frame_r.shape) != shape:
            raise ValueError(f"frames must be uint8 [H, W, 3] of one size, got {shape} and {tuple(frame_r.shape)}")
        if shape[1] > MAX_WIDTH:
            raise ValueError(f"width {shape[1]} exceeds {MAX_WIDTH}")
        r = self.rectification
        if r is not None and (shape[1], shape[0]) != tuple(r.image_size):
            raise RuntimeError(f"Capture size mismatch. Expected calibration size={tuple(r.image_size)}, "
                               f"got={(shape[1], shape[0])}.")
        if self._key != (shape[0], shape[1]):
            self._alloc(shape[0], shape[1])
        if isinstance(frame_l, torch.Tensor):
            if frame_l.dtype != torch.uint8 or frame_r.dtype != torch.uint8 or frame_l.device != self.device \
                    or frame_r.device != self.device:
                raise ValueError(f"device frames must be uint8 tensors on {self.device}")
            return frame_l.contiguous(), frame_r.contiguous()
        if frame_l.dtype != np.uint8 or frame_r.dtype != np.uint8:
            raise ValueError("frames must be uint8")
        b = self._buf
        i = self._stage_i
        self._stage_i = (i + 1) % 3
        if b["pin_ev"][i] is not None:
            b["pin_ev"][i].synchronize()  # the upload of three steps ago: long complete unless frames queue up
        else:
            b["pin_ev"][i] = torch.cuda.Event()
        pin = b["pin"][i].numpy()
        pin[0] = frame_l
        pin[1] = frame_r
        b["frames"][i].copy_(b["pin"][i], non_blocking=True)
        b["pin_ev"][i].record(torch.cuda.current_stream(self.device))
        return b["frames"][i][0], b["frames"][i][1]

    # ------------------------------------------------------------------ one frame
    def step(self, frame_l, frame_r) -> ClassicResult:
        """One frame pair (uint8 BGR [H, W, 3], numpy or device tensors) through depth_live.py:155-178. Launches only:
        no host synchronisation, and no allocation after the first call at a size."""
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            fl, fr = self._frames(frame_l, frame_r)
            b = self._buf
            H, W = self._key
            s = L.stream_handle(self.device)
            rect_l, rect_r = fl, fr
            if self.rectification is not None:
                rect_l, rect_r = b["rect"][0], b["rect"][1]
                L.call("sd_live_rectify", fl.data_ptr(), H, W, b["m1l"].data_ptr(), b["m2l"].data_ptr(),
                       rect_l.data_ptr(), s)
                L.call("sd_live_rectify", fr.data_ptr(), H, W, b["m1r"].data_ptr(), b["m2r"].data_ptr(),
                       rect_r.data_ptr(), s)
            gl, gr = b["gray"][0], b["gray"][1]
            L.call("sd_sgm_gray", rect_l.data_ptr(), H, W, gl.data_ptr(), s)
            L.call("sd_sgm_gray", rect_r.data_ptr(), H, W, gr.data_ptr(), s)
            self.matcher.compute(gl, gr, out=b["q"])
            L.call("sd_sgm_post", b["q"].data_ptr(), H, W, self.Q.ctypes.data, b["disp"].data_ptr(), b["z"].data_ptr(),
                   b["code"].data_ptr(), b["minmax"].data_ptr(), s)
            L.call("sd_sgm_center", b["z"].data_ptr(), H, W, self.center_window, b["center"].data_ptr(), s)
            L.call("sd_live_compose", b["code"].data_ptr(), b["lut"].data_ptr(), b["vis"].data_ptr(), None, None, None,
                   None, None, None, H, W, H, W, s)
        return ClassicResult(self, disparity_q4=b["q"], disparity=b["disp"], depth_m=b["z"], rect_left=rect_l,
                             rect_right=rect_r, disp_vis=b["vis"])

    def _readout(self) -> float:
        b = self._buf
        if b is None:
            raise RuntimeError("readout() before the first step")
        b["center_host"].copy_(b["center"], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return float(b["center_host"][0])


class ClassicBatchResult(ClassicResult):
    """Device tensors of one step of all streams, [n, ...] views of ClassicDepthBatch's buffers (the next step
    overwrites them)."""

    __slots__ = ()

    def readout(self) -> np.ndarray:
        """The centre distances in metres, float32 [n] (NaN for a stream whose centre patch has no value): one
        4 * n-byte copy and the only host synchronisation of the frame path."""
        return self._owner._readout()


class ClassicDepthBatch:
    """The classical frame path for n stereo rigs of one capture size and one matcher configuration: one launch per
    stage and step, whatever n is, and every stream's results are the bytes a ClassicDepth stepped on that stream's
    pair gives.

        classic = ClassicDepthBatch(4, rectification=[rect0, rect1, rect2, rect3], Q=Qs)   # Qs: [4, 4, 4]
        res = classic.step(frames_l, frames_r)     # uint8 [4, H, W, 3] per side; device tensors, no host sync
        dist_m = res.readout()                     # float32 [4], the only host sync

    The matcher keeps no state between frames, so there is no hold or fresh mask: a rig without a new frame resubmits
    its last one. The workspace is n x sd_sgm_ws_bytes (n x 160 MB at 640 x 480, D = 128)."""

    def __init__(self, n, rectification=None, Q=None, center_window=15, colormap="turbo", device="cuda", **matcher_kw):
        """n: 1..64 streams. rectification: None (frames are taken as rectified), one object with the reference's map
        attributes shared by all streams, or a list of one per stream (all of one image_size). Q: the 4 x 4
        reprojection matrix for all streams, or [n, 4, 4]. center_window, colormap, matcher_kw: as ClassicDepth."""
        n = int(n)
        if not 1 <= n <= MAX_STREAMS:
            raise ValueError(f"streams must be in [1, {MAX_STREAMS}], got {n}")
        self.streams = n
        if Q is None:
            raise ValueError("ClassicDepthBatch needs the calibration's reprojection matrix Q ([4, 4] or [n, 4, 4])")
        Qa = np.asarray(Q, dtype=np.float64)
        if Qa.ndim == 3:
            if Qa.shape != (n, 4, 4):
                raise ValueError(f"Q must be [4, 4] or [n = {n}, 4, 4], got shape {Qa.shape}")
            self.Q = np.ascontiguousarray(np.stack([reprojection_rows(q) for q in Qa]))
        else:
            self.Q = np.ascontiguousarray(np.stack([reprojection_rows(Qa)] * n))
        if not 0 <= int(center_window) <= MAX_CENTER_WINDOW:
            raise ValueError(f"center_window must be in [0, {MAX_CENTER_WINDOW}]")
        self.center_window = int(center_window)
        self.matcher = StereoSGM(**matcher_kw)
        self.shared_maps = not isinstance(rectification, (list, tuple))
        if not self.shared_maps:
            if len(rectification) != n:
                raise ValueError(f"rectification: a list must have one entry per stream ({n}), got {len(rectification)}")
            if any(r is None for r in rectification):
                raise ValueError("rectification: a list must hold one object per stream (no None entries)")
            sizes = {tuple(r.image_size) for r in rectification}
            if len(sizes) > 1:
                raise ValueError(f"rectification: all streams must have one image_size, got {sorted(sizes)}")
            self.rectification = list(rectification)
        else:
            self.rectification = None if rectification is None else [rectification]
        self.image_size = None if self.rectification is None else tuple(self.rectification[0].image_size)
        lut = colormap_lut(colormap) if isinstance(colormap, str) else np.asarray(colormap)
        if lut.shape != (256, 3) or lut.dtype != np.uint8:
            raise ValueError("colormap: a name or a [256, 3] uint8 BGR table")
        self._lut_host = np.ascontiguousarray(lut)
        self.device = torch.device(device)
        self._buf = None
        self._key = None
        self._stage_i = 0

    # ------------------------------------------------------------------ buffers
    def _alloc(self, H: int, W: int):
        n, device = self.streams, self.device
        with torch.inference_mode(False):
            def dev(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=device)

            u8, f32 = torch.uint8, torch.float32
            b = {
                "rect": dev((2, n, H, W, 3), u8), "gray": dev((2, n, H, W), u8), "q": dev((n, H, W), torch.int16),
                "disp": dev((n, H, W), f32), "z": dev((n, H, W), f32), "code": dev((n, H, W), u8),
                "vis": dev((n, H, W, 3), u8), "minmax": torch.zeros((n, 2), dtype=torch.int32, device=device),
                "center": dev((n,), f32), "lut": torch.as_tensor(self._lut_host).to(device),
                "Q": torch.as_tensor(self.Q.reshape(n, 16)).to(device),
                "pin": [torch.empty((2, n, H, W, 3), dtype=u8, pin_memory=True) for _ in range(3)],
                "pin_ev": [None, None, None],
                "frames": [dev((2, n, H, W, 3), u8) for _ in range(3)],
                "center_host": torch.full((n,), float("nan"), dtype=f32, pin_memory=True),
            }
            if self.rectification is not None:
                for side in ("l", "r"):
                    m1s, m2s = [], []
                    for r in self.rectification:
                        m1 = np.ascontiguousarray(getattr(r, f"map_{side}_1"))
                        m2 = np.ascontiguousarray(getattr(r, f"map_{side}_2"))
                        if m1.shape != (H, W, 2) or m1.dtype != np.int16 or m2.shape != (H, W) or m2.dtype != np.uint16:
                            raise ValueError("rectification maps: map1 int16 [H, W, 2] and map2 uint16 [H, W] "
                                             "(cv2.initUndistortRectifyMap(..., cv2.CV_16SC2) or live.rectify_maps)")
                        m1s.append(m1)
                        m2s.append(m2.view(np.int16))
                    b[f"m1{side}"] = torch.as_tensor(np.stack(m1s)).to(device)
                    b[f"m2{side}"] = torch.as_tensor(np.stack(m2s)).to(device)
        self.matcher.workspace_batch(device, n, H, W)
        self._buf, self._key = b, (H, W)

    def _frames(self, frames_l, frames_r):
        """Both sides on the device, uint8 [n, H, W, 3]. numpy frames: pinned staging, one non_blocking copy."""
        n = self.streams
        if isinstance(frames_l, torch.Tensor) != isinstance(frames_r, torch.Tensor):
            raise TypeError("both frame sets must be numpy arrays or both device tensors")
        shape = tuple(frames_l.shape)
        if len(shape) != 4 or shape[0] != n or shape[3] != 3 or tuple(frames_r.shape) != shape:
            raise ValueError(f"frames must be uint8 [n = {n}, H, W, 3] of one size, got {shape} and "
                             f"{tuple(frames_r.shape)}")
        if shape[2] > MAX_WIDTH:
            raise ValueError(f"width {shape[2]} exceeds {MAX_WIDTH}")
        if self.image_size is not None and (shape[2], shape[1]) != self.image_size:
            raise RuntimeError(f"Capture size mismatch. Expected calibration size={self.image_size}, "
                               f"got={(shape[2], shape[1])}.")
        if self._key != (shape[1], shape[2]):
            self._alloc(shape[1], shape[2])
        if isinstance(frames_l, torch.Tensor):
            if frames_l.dtype != torch.uint8 or frames_r.dtype != torch.uint8 or frames_l.device != self.device \
                    or frames_r.device != self.device:
                raise ValueError(f"device frames must be uint8 tensors on {self.device}")
            return frames_l.contiguous(), frames_r.contiguous()
        if frames_l.dtype != np.uint8 or frames_r.dtype != np.uint8:
            raise ValueError("frames must be uint8")
        b = self._buf
        i = self._stage_i
        self._stage_i = (i + 1) % 3
        if b["pin_ev"][i] is not None:
            b["pin_ev"][i].synchronize()  # the upload of three steps ago: long complete unless frames queue up
        else:
            b["pin_ev"][i] = torch.cuda.Event()
        pin = b["pin"][i].numpy()
        pin[0] = frames_l
        pin[1] = frames_r
        b["frames"][i].copy_(b["pin"][i], non_blocking=True)
        b["pin_ev"][i].record(torch.cuda.current_stream(self.device))
        return b["frames"][i][0], b["frames"][i][1]

    # ------------------------------------------------------------------ one step of all streams
    def step(self, frames_l, frames_r) -> ClassicBatchResult:
        """One frame pair per stream (uint8 BGR [n, H, W, 3] per side, numpy or device tensors) through
        depth_live.py:155-178. Launches only, as many as ClassicDepth.step issues for one pair: no host
        synchronisation, and no allocation after the first call at a size."""
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        n = self.streams
        with torch.cuda.device(self.device):
            fl, fr = self._frames(frames_l, frames_r)
            b = self._buf
            H, W = self._key
            s = L.stream_handle(self.device)
            rect_l, rect_r = fl, fr
            if self.rectification is not None:
                rect_l, rect_r = b["rect"][0], b["rect"][1]
                map_stride = 0 if self.shared_maps else H * W
                L.call("sd_live_rectify_n", n, fl.data_ptr(), H, W, b["m1l"].data_ptr(), b["m2l"].data_ptr(), map_stride,
                       rect_l.data_ptr(), s)
                L.call("sd_live_rectify_n", n, fr.data_ptr(), H, W, b["m1r"].data_ptr(), b["m2r"].data_ptr(), map_stride,
                       rect_r.data_ptr(), s)
            gl, gr = b["gray"][0], b["gray"][1]
            # [n][H][W][3] is an image of n * H rows to the gray kernel
            L.call("sd_sgm_gray", rect_l.data_ptr(), n * H, W, gl.data_ptr(), s)
            L.call("sd_sgm_gray", rect_r.data_ptr(), n * H, W, gr.data_ptr(), s)
            self.matcher.compute_batch(gl, gr, out=b["q"])
            L.call("sd_sgm_post_n", n, b["q"].data_ptr(), H, W, b["Q"].data_ptr(), b["disp"].data_ptr(),
                   b["z"].data_ptr(), b["code"].data_ptr(), b["minmax"].data_ptr(), s)
            L.call("sd_sgm_center_n", n, b["z"].data_ptr(), H, W, self.center_window, b["center"].data_ptr(), s)
            L.call("sd_live_compose_n", n, b["code"].data_ptr(), b["lut"].data_ptr(), b["vis"].data_ptr(), None, None,
                   None, None, None, None, H, W, H, W, 0, s)
        return ClassicBatchResult(self, disparity_q4=b["q"], disparity=b["disp"], depth_m=b["z"], rect_left=rect_l,
                                  rect_right=rect_r, disp_vis=b["vis"])

    def _readout(self) -> np.ndarray:
        b = self._buf
        if b is None:
            raise RuntimeError("readout() before the first step")
        b["center_host"].copy_(b["center"], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return b["center_host"].numpy().copy()
