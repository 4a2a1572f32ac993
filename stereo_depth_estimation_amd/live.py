"""The live depth loop's frame path on the device (the reference's live_camera/depth_live_dl.py:468-617 around
``model(x)``): raw uint8 BGR camera frames in, display-ready uint8 images and three centre scalars out.

    live = LiveDepth(model, model_size=(960, 720), rectification=rect)
    res = live.step(frame_l, frame_r)        # no host sync: device tensors, overwritten by the next step
    center_disp, center_depth_m, center_conf = res.readout()   # the only host sync

Rectification (cv2.remap with OpenCV's fixed-point maps), BGR->RGB, resize, /255 and the engine's input pack are one
HIP pass that writes the engine's input; EMA, depth, confidence, colour codes, contours, the auto range, the centre
medians and the colour images run after the heads (csrc/live.hip). Camera capture, windows and text overlays stay with
the host application. Not reproduced: OpenCV's intermediate uint8 rounding and fixed-point interpolation tables, and
the bytes of its colormap tables.

Several rigs of one capture size run through one step with LiveDepthBatch (below): one front end, one batch-N forward,
one display stage and one read-out for N camera pairs.
"""

from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import _lib as L

COLORMAP_NAMES = ("turbo", "inferno", "magma", "viridis")
COLORMAP_FILE = Path(__file__).resolve().parent / "colormaps.json"
DEPTH_VIS_RANGE_M = (0.0, 10.0)
DEPTH_CONTOUR_STEP_M = 0.5
CONFIDENCE_COLORMAP = "viridis"
CONFIDENCE_VIS_RANGE = (0.0, 5.0)
MAX_CENTER_WINDOW = 63


# ---------------------------------------------------------------------- host helpers (numpy, float64)
def colormap_lut(name: str) -> np.ndarray:
    """[256, 3] uint8 BGR table of one of COLORMAP_NAMES (generated from matplotlib's listed colormaps by
    tools/gen_colormap_luts.py; OpenCV took its tables from the same source, byte equality with cv2 is not pinned)."""
    if name not in COLORMAP_NAMES:
        raise ValueError(f"unknown colormap {name!r}: one of {COLORMAP_NAMES}")
    return load_colormaps()[COLORMAP_NAMES.index(name)]


_colormaps = None


def load_colormaps() -> np.ndarray:
    """The committed tables (colormaps.json: {"names": [...], "bgr": [4][256][3]}) as one [4, 256, 3] uint8 array, in
    the order of COLORMAP_NAMES."""
    global _colormaps
    if _colormaps is None:
        data = json.loads(COLORMAP_FILE.read_text())
        luts = np.asarray(data["bgr"], dtype=np.uint8)
        if tuple(data["names"]) != COLORMAP_NAMES or luts.shape != (len(COLORMAP_NAMES), 256, 3):
            raise ValueError(f"{COLORMAP_FILE}: expected the tables of {COLORMAP_NAMES}, [4][256][3]")
        _colormaps = luts
    return _colormaps


def rectify_maps(mtx, dist, R, P, image_size) -> tuple[np.ndarray, np.ndarray]:
    """Undistort-rectify maps in OpenCV's CV_16SC2 fixed-point format for image_size = (width, height):
    map1 int16 [h, w, 2] (integer x, y) and map2 uint16 [h, w] (fy5 << 5 | fx5, fractions in 1/32 px).

    For every destination pixel (u, v): the ray (P[:, :3] @ R)^-1 [u, v, 1], normalised by its z, distorted with the
    radial (k1..k6, rational) and tangential (p1, p2) model, projected through `mtx`; the source coordinate is
    quantised as round_half_even(32 * coord)."""
    mtx = np.asarray(mtx, dtype=np.float64)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    d = np.zeros(8, dtype=np.float64)
    dv = np.asarray(dist if dist is not None else [], dtype=np.float64).reshape(-1)[:8]
    d[:dv.size] = dv
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    w, h = int(image_size[0]), int(image_size[1])
    inv = np.linalg.inv(P[:3, :3] @ R)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = inv[0, 0] * u + inv[0, 1] * v + inv[0, 2]
    Y = inv[1, 0] * u + inv[1, 1] * v + inv[1, 2]
    Z = inv[2, 0] * u + inv[2, 1] * v + inv[2, 2]
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    radial = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    sx = mtx[0, 0] * xd + mtx[0, 2]
    sy = mtx[1, 1] * yd + mtx[1, 2]
    return quantize_maps(sx, sy)


def quantize_maps(sx: np.ndarray, sy: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Float source coordinates -> (map1 int16 [h, w, 2], map2 uint16 [h, w]), round_half_even(32 * coord), the
    integer part saturated to int16."""
    qx = np.rint(32.0 * np.asarray(sx, dtype=np.float64)).astype(np.int64)
    qy = np.rint(32.0 * np.asarray(sy, dtype=np.float64)).astype(np.int64)
    map1 = np.stack([np.clip(qx >> 5, -32768, 32767), np.clip(qy >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    map2 = (((qy & 31) << 5) | (qx & 31)).astype(np.uint16)
    return map1, map2


def estimate_baseline_m(P1=None, P2=None, T=None) -> float | None:
    """Stereo baseline in metres: |P2[0, 3] / P1[0, 0]| when both projections are given and that is finite and
    positive, else the norm of T (>= 3 values), else None."""
    if P1 is not None and P2 is not None:
        f = float(np.asarray(P1)[0, 0])
        if np.isfinite(f) and abs(f) > 1e-9:
            b = abs(-float(np.asarray(P2)[0, 3]) / f)
            if np.isfinite(b) and b > 0.0:
                return b
    if T is not None:
        t = np.asarray(T, dtype=np.float64).reshape(-1)
        if t.size >= 3:
            b = float(np.linalg.norm(t))
            if np.isfinite(b) and b > 0.0:
                return b
    return None


@dataclass
class Rectification:
    """The reference's RectificationData: fixed-point maps of both sides and the rectified geometry."""

    map_l_1: np.ndarray
    map_l_2: np.ndarray
    map_r_1: np.ndarray
    map_r_2: np.ndarray
    image_size: tuple[int, int]  # (width, height)
    focal_length_px: float
    baseline_m: float | None


@dataclass
class Calibration:
    focal_length_px: float | None
    baseline_m: float | None
    calibration_width_px: int | None
    rectification: Rectification | None


def load_calibration(path, rectify: bool = True) -> Calibration:
    """Read the reference's stereo calibration .npz (keys mtx_l, dist_l, mtx_r, dist_r, R1, R2, P1, P2, image_size,
    optionally T). The geometry needs only P1 / P2 / T / image_size (mtx_l's focal length when P1 is absent); the
    rectification maps are built when all of their keys are present and `rectify` is set, and then define the focal
    length, baseline and calibration width, as in the reference's main()."""
    with np.load(path) as data:
        d = {k: data[k] for k in data.files}
    P1, P2, T = d.get("P1"), d.get("P2"), d.get("T")
    if P1 is not None:
        focal = float(P1[0, 0])
    elif "mtx_l" in d:
        focal = float(d["mtx_l"][0, 0])
    else:
        focal = None
    if focal is not None and (not np.isfinite(focal) or focal <= 0.0):
        focal = None
    baseline = estimate_baseline_m(P1, P2, T)
    width = int(np.asarray(d["image_size"]).reshape(-1)[0]) if "image_size" in d else None
    rect = None
    need = ("mtx_l", "dist_l", "mtx_r", "dist_r", "R1", "R2", "P1", "P2", "image_size")
    if rectify and all(k in d for k in need):
        size = tuple(int(v) for v in np.asarray(d["image_size"]).reshape(-1)[:2])
        ml1, ml2 = rectify_maps(d["mtx_l"], d["dist_l"], d["R1"], P1, size)
        mr1, mr2 = rectify_maps(d["mtx_r"], d["dist_r"], d["R2"], P2, size)
        rect = Rectification(ml1, ml2, mr1, mr2, size, float(P1[0, 0]), baseline)
        focal, width = rect.focal_length_px, size[0]
    return Calibration(focal, baseline, width, rect)


# ---------------------------------------------------------------------- the device path
# LiveDepthBatch is the implementation, for N rigs per step; LiveDepth (at the end) is its N = 1 case for one rig.
MAX_STREAMS = 64


class LiveResult:
    """Device tensors of one step (views of the live object's buffers: the next step overwrites them, except the
    slices of streams it holds): stream-major [N, ...] from LiveDepthBatch, stream 0's from LiveDepth. depth_m,
    confidence and confidence_vis are None when depth / uncertainty is off."""

    __slots__ = ("disparity", "logvar", "depth_m", "confidence", "depth_vis", "confidence_vis", "left_view", "_live")

    def __init__(self, live, **kw):
        self._live = live
        for k, v in kw.items():
            setattr(self, k, v)

    def readout(self):
        """(center_disparity, center_depth_m, center_confidence) of the latest step: float32 [N, 3] from LiveDepthBatch
        (a held stream's row is its last fresh frame's), a tuple of three floats from LiveDepth. One 12 * N-byte copy
        and the only host synchronisation of the frame path."""
        return self._live._readout()


LiveBatchResult = LiveResult


def _per_stream(value, streams: int, name: str) -> list:
    """A scalar (or None) for all streams, or a sequence of one value per stream."""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != streams:
            raise ValueError(f"{name}: a sequence must have one entry per stream ({streams}), got {len(value)}")
        return list(value)
    return [value] * streams


def stream_rectification(rectification, streams: int):
    """None, one rectification object shared by all streams, or a list of one per stream (all of one image_size) ->
    (one object per stream or None, shared_maps, image_size or None)."""
    shared = not isinstance(rectification, (list, tuple))
    if rectification is None:
        return None, shared, None
    rects = _per_stream(rectification, streams, "rectification")
    if any(r is None for r in rects):
        raise ValueError("rectification: a sequence must hold one object per stream (no None entries)")
    sizes = {tuple(r.image_size) for r in rects}
    if len(sizes) > 1:
        raise ValueError(f"rectification: all streams must have one image_size, got {sorted(sizes)}")
    return rects, shared, sizes.pop()


def upload_maps(rects, side: str, H: int, W: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """Side "l" or "r" of the objects' fixed-point maps, checked and stacked on the device: map1 int16
    [len(rects), H, W, 2] and map2 as int16 [len(rects), H, W] (the uint16's bits)."""
    m1s, m2s = [], []
    for r in rects:
        m1 = np.ascontiguousarray(getattr(r, f"map_{side}_1"))
        m2 = np.ascontiguousarray(getattr(r, f"map_{side}_2"))
        if m1.shape != (H, W, 2) or m1.dtype != np.int16 or m2.shape != (H, W) or m2.dtype != np.uint16:
            raise ValueError("rectification maps: map1 int16 [H, W, 2] and map2 uint16 [H, W] "
                             "(cv2.initUndistortRectifyMap(..., cv2.CV_16SC2) or live.rectify_maps)")
        m1s.append(m1)
        m2s.append(m2.view(np.int16))
    return torch.as_tensor(np.stack(m1s)).to(device), torch.as_tensor(np.stack(m2s)).to(device)


def colormap_table(colormap) -> np.ndarray:
    """A name of COLORMAP_NAMES or a [256, 3] uint8 BGR table -> the table, contiguous."""
    lut = colormap_lut(colormap) if isinstance(colormap, str) else np.asarray(colormap)
    if lut.shape != (256, 3) or lut.dtype != np.uint8:
        raise ValueError("colormap: a name or a [256, 3] uint8 BGR table")
    return np.ascontiguousarray(lut)


class PinnedRing:
    """Three pinned uint8 staging buffers of one shape for numpy frames, filled in turn: a slot is written again only
    after its upload of three steps ago has completed, so a step never waits unless frames queue up."""

    def __init__(self, shape):
        self.pin = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(3)]
        self._events = [torch.cuda.Event() for _ in range(3)]
        self._slot = -1

    def take(self) -> tuple[int, np.ndarray]:
        """The next slot and the numpy view of pin[slot], once the slot's last upload is complete."""
        self._slot = (self._slot + 1) % 3
        self._events[self._slot].synchronize()  # returns at once for a slot that has not been uploaded yet
        return self._slot, self.pin[self._slot].numpy()

    def record(self, device) -> None:
        """After the caller's non_blocking copies out of the slot taken last."""
        self._events[self._slot].record(torch.cuda.current_stream(device))


class LiveDepthBatch:
    """The frame path for `streams` camera pairs of one capture size and one model: one front-end launch, one batch-N
    forward and one launch sequence of the display stage per step, whatever N is.

        live = LiveDepthBatch(model, streams=4, model_size=(960, 720), rectification=[rect0, rect1, rect2, rect3])
        res = live.step(frames_l, frames_r, fresh=[True, True, False, True])   # stream 2 had no new frame
        centers = res.readout()                                                # [4, 3], the only host sync

    A stream that is not fresh is held: its EMA state, depth, confidence, images and centre row stay as its last
    fresh frame left them. The forward still runs over all N input slots, and res.logvar (the heads' raw output, like
    the raw disparity before the EMA) is overwritten for held streams too."""

    def __init__(self, model, streams, model_size=(320, 240), rectification=None, focal_length_px=None, baseline_m=None,
                 calibration_width_px=None, uncertainty=True, colormap="turbo", ema_alpha=0.0, center_window=15):
        """model: an eval-mode StereoUNet (in_channels 6) on a HIP device. streams: 1..64. model_size = (width,
        height). rectification: None, one object with the reference's RectificationData attributes (map_l_1, map_l_2,
        map_r_1, map_r_2, image_size, focal_length_px, baseline_m) shared by all streams, or a sequence of one per
        stream (all of one image_size); when given it defines the geometry (depth_live_dl.py:407-410).
        focal_length_px, baseline_m, calibration_width_px: scalars or sequences of one per stream. Depth is on for a
        stream when a baseline and a focal length scaled to the model width exist (:412-423), and must be on for all
        streams or for none. colormap: a name of COLORMAP_NAMES or a [256, 3] uint8 BGR table."""
        n = int(streams)
        if not 1 <= n <= MAX_STREAMS:
            raise ValueError(f"streams must be in [1, {MAX_STREAMS}]")
        if not 0.0 <= float(ema_alpha) <= 1.0:
            raise ValueError("ema_alpha must be in [0, 1]")
        if not 0 <= int(center_window) <= MAX_CENTER_WINDOW:
            raise ValueError(f"center_window must be in [0, {MAX_CENTER_WINDOW}]")
        if model.in_channels != 6:
            raise ValueError("LiveDepth / LiveDepthBatch need a stereo model (in_channels 6)")
        self.model = model
        self.streams = n
        self.W, self.H = int(model_size[0]), int(model_size[1])
        if self.H % 16 or self.W % 16 or self.H <= 0 or self.W <= 0:
            raise ValueError("model_size must be positive multiples of 16 (four 2x2 pools)")
        self.rectification, self.shared_maps, self.image_size = stream_rectification(rectification, n)
        focal = _per_stream(focal_length_px, n, "focal_length_px")
        base = _per_stream(baseline_m, n, "baseline_m")
        width = _per_stream(calibration_width_px, n, "calibration_width_px")
        self.focal_length_px_model, self.baseline_m = [], []
        for i, r in enumerate(self.rectification or [None] * n):
            f, b, w = (r.focal_length_px, r.baseline_m, r.image_size[0]) if r is not None else (focal[i], base[i], width[i])
            fm = f * (self.W / float(w)) if f is not None and w is not None and w > 0 else None
            self.focal_length_px_model.append(fm)
            self.baseline_m.append(b)
        enabled = [fm is not None and b is not None for fm, b in zip(self.focal_length_px_model, self.baseline_m)]
        if any(enabled) != all(enabled):
            raise ValueError("depth is enabled for some streams and not for others (a baseline and a focal length with "
                             f"its calibration width per stream): enabled = {enabled}; it must be all or none")
        self.depth_enabled = all(enabled)
        self.uncertainty = bool(uncertainty)
        self.ema_alpha = float(ema_alpha)
        self.center_window = int(center_window)
        self._lut_host = (colormap_table(colormap), colormap_lut(CONFIDENCE_COLORMAP))
        self._first = [True] * n  # the stream's next fresh frame is copied into the EMA state
        self._seen = [False] * n  # the stream has had a fresh frame since the buffers were made
        self._buf = None
        self._key = None

    def reset(self, stream=None) -> None:
        """Forget the EMA state of one stream, or of all: its next fresh frame's prediction is taken as is."""
        if stream is None:
            self._first = [True] * self.streams
            return
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream must be in [0, {self.streams})")
        self._first[int(stream)] = True

    # ------------------------------------------------------------------ buffers
    def _alloc(self, device, Hc: int, Wc: int):
        n, H, W = self.streams, self.H, self.W
        with torch.inference_mode(False):  # written in place by later steps, in or out of inference mode
            def dev(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=device)

            f32, u8 = torch.float32, torch.uint8
            fb = [float(f) * float(b) for f, b in zip(self.focal_length_px_model, self.baseline_m)] \
                if self.depth_enabled else [0.0] * n
            b = {
                "disp": dev((n, 1, H, W), f32), "logvar": dev((n, 1, H, W), f32), "state": dev((n, H, W), f32),
                "depth": dev((n, H, W), f32), "conf": dev((n, H, W), f32), "dcode": dev((n, H, W), u8),
                "ccode": dev((n, H, W), u8), "edge": dev((n, H, W), u8), "depth_vis": dev((n, Hc, Wc, 3), u8),
                "conf_vis": dev((n, Hc, Wc, 3), u8), "left_view": dev((n, Hc, Wc, 3), u8),
                "view": dev((n, Hc, Wc, 3), u8), "center": dev((n, 3), f32),
                "fb": torch.as_tensor(np.asarray(fb, dtype=np.float32)).to(device),
                "sel": torch.zeros((n, 8), dtype=f32, device=device),
                "sel_ws": torch.zeros(L.call("sd_live_select_n_ws_bytes", n) // 4, dtype=torch.int32, device=device),
                "lut_a": torch.as_tensor(self._lut_host[0]).to(device), "lut_b": torch.as_tensor(self._lut_host[1]).to(device),
                # numpy frames: pinned staging buffers [side][stream] and ONE device copy, in which a held stream's
                # slices keep its previous frame
                "ring": PinnedRing((2, n, Hc, Wc, 3)),
                "frames": dev((2, n, Hc, Wc, 3), u8),
                "center_host": torch.full((n, 3), float("nan"), dtype=f32, pin_memory=True),
            }
            if self.rectification is not None:
                rects = self.rectification[:1] if self.shared_maps else self.rectification
                for side in ("l", "r"):
                    b[f"m1{side}"], b[f"m2{side}"] = upload_maps(rects, side, Hc, Wc, device)
        self._buf, self._key = b, (device, Hc, Wc)
        self._first = [True] * n
        self._seen = [False] * n

    def _frames(self, frames_l, frames_r, fresh, device):
        """Both sides on the device, uint8 [N, Hc, Wc, 3]. numpy frames: the fresh streams' frames go through pinned
        staging into the device copy (non_blocking, one copy per side and run of fresh streams)."""
        n = self.streams
        if isinstance(frames_l, torch.Tensor) != isinstance(frames_r, torch.Tensor):
            raise TypeError("both frame sets must be numpy (an array or a sequence of frames) or both device tensors")
        is_dev = isinstance(frames_l, torch.Tensor)
        if not is_dev and not isinstance(frames_l, np.ndarray):  # a sequence of N frames
            if len(frames_l) != n or len(frames_r) != n:
                raise ValueError(f"expected {n} frames per side, got {len(frames_l)} and {len(frames_r)}")
            shapes = {tuple(np.shape(f)) for f in list(frames_l) + list(frames_r)}
            if len(shapes) != 1:
                raise ValueError(f"frames must be uint8 [Hc, Wc, 3] of one size, got {sorted(shapes)}")
            shape = (n,) + shapes.pop()
        else:
            shape = tuple(frames_l.shape)
            if tuple(frames_r.shape) != shape:
                raise ValueError(f"frames must be uint8 [N, Hc, Wc, 3] of one size, got {shape} and "
                                 f"{tuple(frames_r.shape)}")
        if len(shape) != 4 or shape[0] != n or shape[3] != 3:
            raise ValueError(f"frames must be uint8 [N = {n}, Hc, Wc, 3], got {shape}")
        if self.image_size is not None and (shape[2], shape[1]) != self.image_size:
            raise RuntimeError(f"Capture size mismatch. Expected calibration size={self.image_size}, "
                               f"got={(shape[2], shape[1])}.")
        if self._key != (device, shape[1], shape[2]):
            self._alloc(device, shape[1], shape[2])
        held_unseen = [i for i in range(n) if not fresh[i] and not self._seen[i]]
        if held_unseen:
            raise ValueError(f"streams {held_unseen} are held (fresh = False) before their first frame: a stream's "
                             "first step must be fresh")
        if is_dev:
            if frames_l.dtype != torch.uint8 or frames_r.dtype != torch.uint8 or frames_l.device != device \
                    or frames_r.device != device:
                raise ValueError("device frames must be uint8 tensors on the model's device")
            return frames_l.contiguous(), frames_r.contiguous()
        for side in (frames_l, frames_r):
            if any(f.dtype != np.uint8 for f in ([side] if isinstance(side, np.ndarray) else side)):
                raise ValueError("frames must be uint8")
        b = self._buf
        i, pin = b["ring"].take()
        runs, k = [], 0  # [k0, k1) runs of fresh streams
        while k < n:
            if not fresh[k]:
                k += 1
                continue
            k0 = k
            while k < n and fresh[k]:
                pin[0, k] = frames_l[k]
                pin[1, k] = frames_r[k]
                k += 1
            runs.append((k0, k))
        if runs == [(0, n)]:
            b["frames"].copy_(b["ring"].pin[i], non_blocking=True)
        else:
            for k0, k1 in runs:
                for side in (0, 1):
                    b["frames"][side, k0:k1].copy_(b["ring"].pin[i][side, k0:k1], non_blocking=True)
        b["ring"].record(device)
        return b["frames"][0], b["frames"][1]

    # ------------------------------------------------------------------ one step of all streams
    def step(self, frames_l, frames_r, fresh=None) -> LiveResult:
        """One frame pair per stream (uint8 BGR [N, Hc, Wc, 3]: numpy arrays, sequences of N numpy [Hc, Wc, 3]
        frames, or device tensors) through rectification, one batch-N forward and the display stage. fresh: N bools
        (default: all); a stream that is not fresh is held: with numpy frames its input slot keeps its previous frame
        (the entry passed for it is ignored), with device tensors the forward reads whatever its slice holds, and in
        both cases nothing of its results changes. Launches only: no host synchronisation, and no allocation after
        the first call at a size. Like the results, the device copy of numpy frames is overwritten by the next step
        (stream-ordered after this step's kernels)."""
        model = self.model
        if model.training:
            raise RuntimeError("LiveDepth / LiveDepthBatch run the inference forward: call model.eval()")
        n = self.streams
        fresh = [True] * n if fresh is None else [bool(f) for f in fresh]
        if len(fresh) != n:
            raise ValueError(f"fresh: one flag per stream ({n}), got {len(fresh)}")
        eng = model.engine()
        with torch.cuda.device(eng.device):
            return self._step(eng, frames_l, frames_r, fresh)

    def _step(self, eng, frames_l, frames_r, fresh) -> LiveResult:
        n, H, W = self.streams, self.H, self.W
        fl, fr = self._frames(frames_l, frames_r, fresh, eng.device)
        b = self._buf
        Hc, Wc = self._key[1], self._key[2]
        maps = [L.ptr(b.get(k)) for k in ("m1l", "m2l", "m1r", "m2r")]
        map_stride = 0 if self.shared_maps else Hc * Wc

        def pack(xin, amax, slot, clear, stream):
            L.call("sd_live_frontend_n", n, eng.sd_dtype, fl.data_ptr(), fr.data_ptr(), Hc, Wc, *maps, map_stride, H, W,
                   xin, None, amax, slot, clear, stream)

        eng.pack_weights(cached=True, train=False)
        eng.forward_packed(H, W, pack, batch=n)
        unc, on = self.uncertainty, self.depth_enabled
        logvar = b["logvar"] if unc else None
        eng.heads(L.SD_HEADS_INFER, disp=b["disp"], logvar=logvar)
        s = L.stream_handle(eng.device)
        view = fl
        if maps[0] is not None:
            L.call("sd_live_rectify_n", n, fl.data_ptr(), Hc, Wc, maps[0], maps[1], map_stride, b["view"].data_ptr(), s)
            view = b["view"]
        a = self.ema_alpha
        copy = hold = 0
        for i in range(n):
            if not fresh[i]:
                hold |= 1 << i
                continue
            if self._first[i] or a <= 0.0:
                copy |= 1 << i
            self._first[i] = False
            self._seen[i] = True
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        dlo, dhi = DEPTH_VIS_RANGE_M
        clo, chi = CONFIDENCE_VIS_RANGE
        L.call("sd_live_post_n", n, b["disp"].data_ptr(), L.ptr(logvar), H, W, b["state"].data_ptr(), copy, hold, f32(a),
               f32(1.0 - a), int(on), b["fb"].data_ptr() if on else None, b["depth"].data_ptr() if on else None,
               b["conf"].data_ptr() if unc else None, b["dcode"].data_ptr() if on else None, f32(dlo),
               f32(max(dhi - dlo, 1e-6)), b["ccode"].data_ptr() if unc else None, f32(clo), f32(max(chi - clo, 1e-6)), s)
        if on:
            L.call("sd_live_contours_n", n, b["depth"].data_ptr(), H, W, f32(dlo), f32(dhi), f32(DEPTH_CONTOUR_STEP_M),
                   b["edge"].data_ptr(), hold, s)
        else:  # each stream's disparity in its own 2nd..98th percentile range
            L.call("sd_live_select_n", n, b["state"].data_ptr(), H, W, b["sel_ws"].data_ptr(), b["sel"].data_ptr(),
                   b["dcode"].data_ptr(), hold, s)
        L.call("sd_live_center_n", n, b["state"].data_ptr(), b["depth"].data_ptr() if on else None,
               b["conf"].data_ptr() if unc else None, H, W, self.center_window, b["center"].data_ptr(), hold, s)
        L.call("sd_live_compose_n", n, b["dcode"].data_ptr(), b["lut_a"].data_ptr(), b["depth_vis"].data_ptr(),
               b["ccode"].data_ptr() if unc else None, b["lut_b"].data_ptr() if unc else None,
               b["conf_vis"].data_ptr() if unc else None, b["edge"].data_ptr() if on else None,
               view.data_ptr() if on else None, b["left_view"].data_ptr() if on else None, H, W, Hc, Wc, hold, s)
        return LiveResult(self, disparity=b["state"], logvar=None if logvar is None else logvar[:, 0],
                          depth_m=b["depth"] if on else None, confidence=b["conf"] if unc else None,
                          depth_vis=b["depth_vis"], confidence_vis=b["conf_vis"] if unc else None,
                          left_view=b["left_view"] if on else view)

    def _readout(self) -> np.ndarray:
        b = self._buf
        if b is None:
            raise RuntimeError("readout() before the first step")
        b["center_host"].copy_(b["center"], non_blocking=True)
        torch.cuda.current_stream(self._key[0]).synchronize()
        return b["center_host"].numpy().copy()


# ---------------------------------------------------------------------- one rig
def _of_batch(name):
    return property(lambda self: getattr(self._batch, name), lambda self, value: setattr(self._batch, name, value))


class LiveDepth:
    """One camera pair: LiveDepthBatch with one stream, taking [Hc, Wc, 3] frames and handing out stream 0's tensors
    and a tuple of three floats (see the module docstring)."""

    def __init__(self, model, model_size=(320, 240), rectification=None, focal_length_px=None, baseline_m=None,
                 calibration_width_px=None, uncertainty=True, colormap="turbo", ema_alpha=0.0, center_window=15):
        """As LiveDepthBatch, with one rectification object (or None) and scalar geometry."""
        self._batch = LiveDepthBatch(model, 1, model_size, rectification, focal_length_px, baseline_m,
                                     calibration_width_px, uncertainty, colormap, ema_alpha, center_window)
        self.rectification = rectification

    model, W, H = _of_batch("model"), _of_batch("W"), _of_batch("H")
    depth_enabled, uncertainty = _of_batch("depth_enabled"), _of_batch("uncertainty")
    ema_alpha, center_window = _of_batch("ema_alpha"), _of_batch("center_window")
    focal_length_px_model = property(lambda self: self._batch.focal_length_px_model[0])
    baseline_m = property(lambda self: self._batch.baseline_m[0])

    def reset(self) -> None:
        """Forget the EMA state: the next frame's prediction is taken as is."""
        self._batch.reset()

    def step(self, frame_l, frame_r) -> LiveResult:
        """One frame pair (uint8 BGR [Hc, Wc, 3], numpy or device tensors) through rectification, the model and the
        display stage. Launches only: no host synchronisation, and no allocation after the first call at a size.
        The next step overwrites the results and the device copy of numpy frames."""
        fl, fr = frame_l[None], frame_r[None]
        res = self._batch.step(fl, fr)
        out = LiveResult(self)
        for k in LiveResult.__slots__[:-1]:
            v = getattr(res, k)
            setattr(out, k, None if v is None else v[0])
        if res.left_view is fl:  # device frames shown as they came: the caller's own tensor
            out.left_view = frame_l
        return out

    def _readout(self) -> tuple[float, float, float]:
        c = self._batch._readout()[0]
        return float(c[0]), float(c[1]), float(c[2])
