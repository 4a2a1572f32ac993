"""The classical live loop on the device (the reference's live_camera/depth_live.py:138-191 without capture, windows
and text): rectification, gray, a semi-global matcher, reprojection, the centre distance and the colour image.

    matcher = StereoSGM(num_disparities=128, block_size=7)
    q = matcher.compute(gray_l, gray_r)        # int16 [H, W], 16 * disparity: the counterpart of matcher.compute

    classic = ClassicDepth(rectification=calib.rectification, Q=Q)
    res = classic.step(frame_l, frame_r)       # no host sync: device tensors, overwritten by the next step
    dist_m = res.readout()                     # the only host sync (4 bytes)

    rigs = ClassicDepthBatch(4, rectification=[r0, r1, r2, r3], Q=Qs)   # n rigs of one size, one launch per stage
    dists = rigs.step(frames_l, frames_r).readout()                      # float32 [4]; StereoSGM.compute_batch alone

ClassicDepthBatch and StereoSGM.compute_batch are the implementation; ClassicDepth and StereoSGM.compute are their
one-stream case.

The matcher follows OpenCV's StereoSGBM step by step (three paths by default; mode="hh4" / "sgbm" / "hh" add the
bottom-up path, the two downward diagonals or all eight) and is pinned bit for bit to the NumPy restatements
tests/sgm_ref.py and tests/sgm_modes_ref.py, not to cv2's bytes; what is stated rather than taken from OpenCV is
listed in INTEGRATION.md. Kernels: csrc/sgm.hip. There is no CPU fallback.

    matcher = StereoSGM(num_disparities=128, block_size=7, cost="census", census_window=(7, 9))

replaces OpenCV's Birchfield-Tomasi pixel cost by the Hamming distance of census descriptors ("The census
cost"; restated in tests/sgm_census_ref.py): the result does not change under a strictly increasing intensity map of
either camera. ClassicDepth, ClassicDepthBatch and proxy.ProxyLoss pass ``cost`` and ``census_window`` on to it.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .live import (MAX_CENTER_WINDOW, MAX_STREAMS, PinnedRing, _of_batch, colormap_table, stream_rectification,
                   upload_maps)

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


# pixel cost name -> SD_SGM_COST_*; the census windows (rows, columns), their descriptor bits being rows * columns - 1
COSTS = {"bt": L.SD_SGM_COST_BT, "census": L.SD_SGM_COST_CENSUS}
CENSUS_WINDOWS = ((3, 3), (5, 5), (7, 7), (7, 9))
DEFAULT_CENSUS_WINDOW = (7, 9)


def parse_census_window(window) -> tuple:
    """One of CENSUS_WINDOWS as (rows, columns), from a pair or from "HxW" (the tools' spelling, e.g. "7x9")."""
    w = window
    try:
        if isinstance(w, str):
            w = w.lower().split("x")
        w = tuple(int(v) for v in w)
    except (TypeError, ValueError):
        w = None
    if w not in CENSUS_WINDOWS:
        raise ValueError(f"census_window must be one of {', '.join(f'{a}x{b}' for a, b in CENSUS_WINDOWS)} "
                         f"(rows x columns), got {window!r}")
    return w


def ws_bytes(H: int, W: int, D: int, cost: str = "bt") -> int:
    """sd_sgm_ws_bytes as a formula: two uint16 volumes, two prefiltered planes, the speckle filter's two int32 planes,
    each rounded up to 256 bytes; cost="census" appends the two uint64 descriptor planes (sd_sgm_ws_bytes_cost_n)."""
    def a(v):
        return (v + 255) // 256 * 256

    return 2 * a(2 * H * W * D) + 2 * a(H * W) + 2 * a(4 * H * W) + (2 * a(8 * H * W) if cost == "census" else 0)


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
    (the application's), "hh4", "sgbm" or "hh", or cv2's integer constant.

    cost: the pixel cost. "bt" (the default, OpenCV's) is Birchfield-Tomasi on the prefiltered and the gray planes.
    "census" is the Hamming distance of census descriptors over ``census_window`` = (rows, columns), one of
    CENSUS_WINDOWS, default (7, 9): it depends only on the order of the intensities inside each image, so any strictly
    increasing intensity map of either camera (gain, offset, gamma) leaves the result unchanged byte for byte
    ("The census cost"). P1 and P2 keep their defaults 8 and 32 block_size^2 there: parameters, not
    measured optima. ``pre_filter_cap`` is then checked and otherwise unused."""

    def __init__(self, min_disparity=0, num_disparities=128, block_size=7, P1=None, P2=None, disp12_max_diff=1,
                 uniqueness_ratio=10, speckle_window_size=100, speckle_range=2, pre_filter_cap=31, mode="3way",
                 cost="bt", census_window=None):
        self.mode = mode_name(mode)
        self.mode_id, npaths = MODES[self.mode]
        if not isinstance(cost, str) or cost not in COSTS:
            raise ValueError(f"cost must be one of {sorted(COSTS)}, got {cost!r}")
        if cost == "bt" and census_window is not None:
            raise ValueError("census_window is the census cost's: give it with cost='census'")
        self.cost, self.cost_id = cost, COSTS[cost]
        if cost == "census":
            self.census_window = parse_census_window(DEFAULT_CENSUS_WINDOW if census_window is None else census_window)
            self.nbits = self.census_window[0] * self.census_window[1] - 1
        else:
            self.census_window, self.nbits = None, None
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
        if cost == "census":
            if npaths * (bs * bs * self.nbits + P2) > 65535:
                raise ValueError(f"{npaths} * (block_size^2 * nbits + P2) = {npaths * (bs * bs * self.nbits + P2)} "
                                 f"exceeds 65535 (nbits = {self.nbits}, the {self.census_window[0]}x"
                                 f"{self.census_window[1]} census window): the cost sums of the {npaths} paths of mode "
                                 f"{self.mode!r} would not fit uint16")
        elif npaths * (bs * bs * (2 * cap + 63) + P2) > 65535:
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

    @property
    def invalid_value(self) -> int:
        return 16 * (self.min_disparity - 1)

    def params(self) -> tuple:
        """The integer arguments of the matcher's C entry points, in their order (mode_id follows them where the entry
        point takes one)."""
        return (self.min_disparity, self.num_disparities, self.block_size, self.P1, self.P2, self.disp12_max_diff,
                self.uniqueness_ratio, self.speckle_window_size, self.speckle_range, self.pre_filter_cap)

    def workspace(self, device, H: int, W: int, n: int = 1) -> torch.Tensor:
        """The matcher's scratch memory for n pairs of H x W (sd_sgm_ws_bytes_cost_n: n x 160 MB at 640 x 480, D = 128,
        and n x 5 MB of descriptors more with the census cost).
        Nothing is kept in it between calls, so the one buffer serves every size it is large enough for: it is
        replaced only to grow or to change device."""
        key = (device, H, W, n)
        if self._ws_key == key:  # the size of the last call: nothing to ask or to compare
            return self._ws
        size = L.call("sd_sgm_ws_bytes_cost_n", n, H, W, self.num_disparities, self.cost_id)
        if size < 0:
            raise ValueError(f"streams must be in [1, {MAX_STREAMS}], got {n}")
        if self._ws is None or self._ws_key[0] != device or self._ws.numel() < size:
            self._ws = None  # released before the larger one is made
            with torch.inference_mode(False):
                self._ws = torch.empty(size, dtype=torch.uint8, device=device)
        self._ws_key = key
        return self._ws

    def compute(self, gray_l: torch.Tensor, gray_r: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 [H, W] device tensors -> int16 [H, W] (16 * disparity; invalid_value where there is none):
        compute_batch on one pair."""
        for g in (gray_l, gray_r):
            if not isinstance(g, torch.Tensor) or g.dtype != torch.uint8 or g.dim() != 2 or not g.is_cuda:
                raise ValueError("compute takes two uint8 [H, W] device tensors")
        if out is None:
            return self.compute_batch(gray_l[None], gray_r[None])[0]
        if out.dtype != torch.int16 or out.shape != gray_l.shape or not out.is_contiguous() \
                or out.device != gray_l.device:
            raise ValueError("out must be a contiguous int16 [H, W] tensor on the images' device")
        self.compute_batch(gray_l[None], gray_r[None], out[None])
        return out

    def compute_batch(self, gray_l: torch.Tensor, gray_r: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 [n, H, W] device tensors (n stereo pairs of one size) -> int16 [n, H, W]: every pair's map is the same
        bytes whatever n is, in one launch per stage. Launches only; the workspace is allocated at the first call and
        again only when a call needs a larger one."""
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
        ws = self.workspace(gray_l.device, H, W, n)
        with torch.cuda.device(gray_l.device):
            if self.cost == "bt":  # the entry point the step has always called (sd_sgm_compute_cost_n with
                # SD_SGM_COST_BT is the same host function and the same launches)
                L.call("sd_sgm_compute_n", n, gray_l.data_ptr(), gray_r.data_ptr(), H, W, *self.params(), self.mode_id,
                       ws.data_ptr(), out.data_ptr(), L.stream_handle(gray_l.device))
            else:
                L.call("sd_sgm_compute_cost_n", n, gray_l.data_ptr(), gray_r.data_ptr(), H, W, *self.params(),
                       self.mode_id, self.cost_id, *self.census_window, ws.data_ptr(), out.data_ptr(),
                       L.stream_handle(gray_l.device))
        return out


# ClassicDepthBatch is the implementation, for n rigs per step; ClassicDepth (at the end) is its n = 1 case for one rig.
class ClassicResult:
    """Device tensors of one step (views of the classic object's buffers: the next step overwrites them): stream-major
    [n, ...] from ClassicDepthBatch, stream 0's from ClassicDepth."""

    __slots__ = ("disparity_q4", "disparity", "depth_m", "rect_left", "rect_right", "disp_vis", "_owner")

    def __init__(self, owner, **kw):
        self._owner = owner
        for k, v in kw.items():
            setattr(self, k, v)

    def readout(self):
        """The centre distance in metres (np.nanmedian of the centre patch of depth_m; NaN when it has no value):
        float32 [n] from ClassicDepthBatch, a float from ClassicDepth. One 4 * n-byte copy and the only host
        synchronisation of the frame path."""
        return self._owner._readout()


ClassicBatchResult = ClassicResult


class ClassicDepthBatch:
    """The classical frame path for n stereo rigs of one capture size and one matcher configuration: one launch per
    stage and step, whatever n is, and a stream's results are the same bytes whatever n is and whichever streams run
    beside it.

        classic = ClassicDepthBatch(4, rectification=[rect0, rect1, rect2, rect3], Q=Qs)   # Qs: [4, 4, 4]
        res = classic.step(frames_l, frames_r)     # uint8 [4, H, W, 3] per side; device tensors, no host sync
        dist_m = res.readout()                     # float32 [4], the only host sync

    The matcher keeps no state between frames, so there is no hold or fresh mask: a rig without a new frame resubmits
    its last one. The workspace is n x sd_sgm_ws_bytes (n x 160 MB at 640 x 480, D = 128)."""

    def __init__(self, n, rectification=None, Q=None, center_window=15, colormap="turbo", device="cuda", **matcher_kw):
        """n: 1..64 streams. rectification: None (frames are taken as rectified), one object with the reference's map
        attributes (map_l_1, map_l_2, map_r_1, map_r_2, image_size), e.g. load_calibration(path).rectification, shared
        by all streams, or a list of one per stream (all of one image_size). Q: the 4 x 4 reprojection matrix of the
        calibration file for all streams, or [n, 4, 4]. colormap: a name of live.COLORMAP_NAMES or a [256, 3] uint8
        BGR table. matcher_kw: StereoSGM's parameters, ``cost="census"`` and ``census_window=(rows, columns)`` among
        them (the census / Hamming pixel cost in place of Birchfield-Tomasi)."""
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
        self.rectification, self.shared_maps, self.image_size = stream_rectification(rectification, n)
        self._lut_host = colormap_table(colormap)
        self.device = torch.device(device)
        self._buf = None
        self._key = None
        self._last_rect_left = None  # the last step's rectified left frames: the colours of cloud()
        self._last_rect_right = None  # with rect_left: the frames of check()
        self._cloud_builder = None
        self._checker = None

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
                # numpy frames: pinned staging buffers [side][stream], each with a device copy of its own
                "ring": PinnedRing((2, n, H, W, 3)),
                "frames": [dev((2, n, H, W, 3), u8) for _ in range(3)],
                "center_host": torch.full((n,), float("nan"), dtype=f32, pin_memory=True),
            }
            if self.rectification is not None:
                rects = self.rectification[:1] if self.shared_maps else self.rectification
                for side in ("l", "r"):
                    b[f"m1{side}"], b[f"m2{side}"] = upload_maps(rects, side, H, W, device)
        self.matcher.workspace(device, H, W, n)
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
        i, pin = b["ring"].take()
        pin[0] = frames_l
        pin[1] = frames_r
        b["frames"][i].copy_(b["ring"].pin[i], non_blocking=True)
        b["ring"].record(self.device)
        return b["frames"][i][0], b["frames"][i][1]

    # ------------------------------------------------------------------ one step of all streams
    def step(self, frames_l, frames_r) -> ClassicResult:
        """One frame pair per stream (uint8 BGR [n, H, W, 3] per side, numpy or device tensors) through
        depth_live.py:155-178. Launches only, the same list whatever n is: no host synchronisation, and no allocation
        after the first call at a size."""
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
        self._last_rect_left, self._last_rect_right = rect_l, rect_r
        return ClassicResult(self, disparity_q4=b["q"], disparity=b["disp"], depth_m=b["z"], rect_left=rect_l,
                             rect_right=rect_r, disp_vis=b["vis"])

    def _readout(self) -> np.ndarray:
        b = self._buf
        if b is None:
            raise RuntimeError("readout() before the first step")
        b["center_host"].copy_(b["center"], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return b["center_host"].numpy().copy()

    def cloud(self, z_range=(-float("inf"), float("inf")), stride: int = 1, organized: bool = False):
        """The coloured point clouds of the last step (cloud.PointCloudBuilder.build on its disparity, rect_left as BGR
        colours and the object's Q): a cloud.CloudResult of n streams. Launches only; the builder and its buffers are
        made at the first call. step() itself runs nothing of this."""
        if self._buf is None or self._last_rect_left is None:
            raise RuntimeError("cloud() before the first step")
        if self._cloud_builder is None:
            from .cloud import PointCloudBuilder

            self._cloud_builder = PointCloudBuilder(self.streams, self.device)
        b = self._buf
        return self._cloud_builder.build(b["disp"], b["Q"], color=self._last_rect_left, bgr=True, z_range=z_range,
                                         stride=stride, organized=organized)

    def check(self, occ_tol: float = 0.5, photo_thr: float = float("inf")):
        """The label-free check of the last step (check.StereoCheck.run on its disparity, rect_left and rect_right; the
        NaN holes of the disparity are class 1): a check.CheckResult of n streams. Launches only; the checker and its
        buffers are made at the first call. step() itself runs nothing of this."""
        if self._buf is None or self._last_rect_left is None:
            raise RuntimeError("check() before the first step")
        if self._checker is None:
            from .check import StereoCheck

            self._checker = StereoCheck(self.streams, self.device)
        return self._checker.run(self._buf["disp"], self._last_rect_left, self._last_rect_right, occ_tol=occ_tol,
                                 photo_thr=photo_thr)


# ---------------------------------------------------------------------- one rig
class ClassicDepth:
    """One stereo rig: ClassicDepthBatch with one stream, taking [H, W, 3] frames and handing out stream 0's tensors
    and the centre distance as a float (see the module docstring)."""

    def __init__(self, rectification=None, Q=None, center_window=15, colormap="turbo", device="cuda", **matcher_kw):
        """As ClassicDepthBatch, with one rectification object (or None) and the 4 x 4 Q."""
        if Q is None:
            raise ValueError("ClassicDepth needs the calibration's reprojection matrix Q")
        self._batch = ClassicDepthBatch(1, rectification, reprojection_rows(Q), center_window, colormap, device,
                                        **matcher_kw)
        self.rectification = rectification

    matcher, center_window, device = _of_batch("matcher"), _of_batch("center_window"), _of_batch("device")
    Q = property(lambda self: self._batch.Q[0])

    def step(self, frame_l, frame_r) -> ClassicResult:
        """One frame pair (uint8 BGR [H, W, 3], numpy or device tensors) through depth_live.py:155-178. Launches only:
        no host synchronisation, and no allocation after the first call at a size."""
        fl, fr = frame_l[None], frame_r[None]
        res = self._batch.step(fl, fr)
        out = ClassicResult(self, **{k: getattr(res, k)[0] for k in ClassicResult.__slots__[:-1]})
        if res.rect_left is fl:  # device frames taken as rectified: the caller's own tensors
            out.rect_left = frame_l
        if res.rect_right is fr:
            out.rect_right = frame_r
        return out

    def _readout(self) -> float:
        return float(self._batch._readout()[0])

    def cloud(self, z_range=(-float("inf"), float("inf")), stride: int = 1, organized: bool = False):
        """The coloured point cloud of the last step: ClassicDepthBatch.cloud with one stream (a cloud.CloudResult whose
        stream 0 is this rig: ``.numpy(0)``, ``.save_ply([path])``)."""
        return self._batch.cloud(z_range=z_range, stride=stride, organized=organized)

    def check(self, occ_tol: float = 0.5, photo_thr: float = float("inf")):
        """The label-free check of the last step: ClassicDepthBatch.check with one stream (a check.CheckResult whose
        sample 0 is this rig)."""
        return self._batch.check(occ_tol=occ_tol, photo_thr=photo_thr)
