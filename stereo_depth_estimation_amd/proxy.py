"""Proxy-label adaptation on the device: the semi-global matcher labels the pixels it is sure of, and the heads are
trained on those labels beside (or instead of) the label-free loss (no counterpart in the reference, whose labels come
from the dataset).

    loss = SelfSupLoss(streams=16)
    proxy = ProxyLoss(streams=16)                       # w_proxy=1, num_disparities=64, block_size=5, mode="3way"
    for batch in loader:                                # {"input": float32 [n, 6, H, W]}: left RGB / 255, then right
        adapt_step(model, opt, batch["input"], loss, proxy=proxy)   # launches only, no host sync
    print(loss.means(), proxy.means())                  # one pinned copy of eight doubles each

    adapt_step(model, opt, inputs, None, proxy=proxy)   # the labels-only step: no check stage, no photometric stage

The photometric term of ``selfsup.py`` is weak where texture is low or repeats, and where the right-view match lies
outside the half-pixel cell the warp's gradient sees. The standard remedy is proxy supervision: ``StereoSGM`` (sgm.py)
already is a device matcher with uniqueness, left-right and speckle filtering, so what it keeps is a filtered, sparse,
reliable map, and the heads already train in the reference's heteroscedastic L1 form against a sparse target
(``|d - t| exp(-lv) + lv``, reference train.py:329-340; ``uncertainty=False``: plain ``|d - t|``).

``labels`` turns the model's own input batch back into the matcher's two gray images (``sd_proxy_gray``) and runs
``StereoSGM.compute_batch`` into a buffer of the object; ``run`` is ``sd_proxy_loss`` on those labels: the gradient
maps for the heads' GRADS mode, written (labels only) or added onto a ``SelfSupResult``'s maps (``into=``). The
arithmetic is stated in include/stereo_hip.h and INTEGRATION.md ("sd_proxy_gray", "sd_proxy_loss") and held to the
NumPy restatement tests/proxy_ref.py. Kernels: csrc/proxy.hip. There is no CPU fallback.

The frames are taken as rectified, as in selfsup.py. The defaults (64 disparities, block 5, ``w_proxy`` = 1, the
matcher's own filters) are parameters and not measured optima: the disparity range is the rig's and the scene's, and
how much a matcher's label should weigh beside the photometric term depends on both.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .live import MAX_STREAMS
from .selfsup import SelfSupResult
from .sgm import MAX_WIDTH, StereoSGM

ROW = 8  # doubles per sample: labelled, sum l, sum a, sum a^2, sum |g_d|, labels on a non-finite disparity, 0, 0
SUMMARY_KEYS = ("proxy_loss", "proxy_mae", "proxy_rmse", "proxy_fraction", "grad_l1")
# totals: the columns of ``rows`` summed over every sample of every step, then [6] steps and [7] pixels
TOTAL_STEPS, TOTAL_PIXELS = 6, 7


def proxy_param(w_proxy=1.0) -> float:
    """The weight as the float32 value the kernel computes with (``selfsup_params``' rule): finite and >= 0."""
    with np.errstate(over="ignore"):  # a value past float32's range rounds to inf and is refused below
        f = float(np.float32(w_proxy))
    if not math.isfinite(f) or f < 0:
        raise ValueError(f"w_proxy must be finite and >= 0, got {w_proxy}")
    return f


def check_width(W: int, min_disparity: int, num_disparities: int):
    """No pixel of a frame that is not wider than the disparity range can carry a label (the matcher labels columns
    x >= min_disparity + num_disparities only)."""
    bound = int(min_disparity) + int(num_disparities)
    if int(W) <= bound:
        raise ValueError(f"width {W} is not above min_disparity + num_disparities = {bound}: no pixel could carry a label")


def summary_from_rows(rows, pixels: int, w_proxy: float) -> dict:
    """The figures of rows [k][8] (one step's samples, or the totals of many steps) over ``pixels`` pixels, in fp64:
    ``proxy_loss`` = w_proxy * sum l / max(1, labelled) (what the gradient maps are the gradient of), ``proxy_mae`` and
    ``proxy_rmse`` the mean and the root mean square of |disp - label| over the labelled pixels (None without one),
    ``proxy_fraction`` labelled / pixels, ``grad_l1`` sum |g_d|."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, ROW).sum(axis=0)
    lab, px = float(r[0]), max(float(pixels), 1.0)
    return {"proxy_loss": w_proxy * float(r[1]) / max(lab, 1.0),
            "proxy_mae": float(r[2]) / lab if lab > 0 else None,
            "proxy_rmse": math.sqrt(float(r[3]) / lab) if lab > 0 else None,
            "proxy_fraction": lab / px, "grad_l1": float(r[4])}


class ProxyResult:
    """Device tensors of one ``ProxyLoss.run`` (views of the proxy object's buffers, or of the ``into`` result's maps:
    the next run overwrites them).

    gdisp:   float32 [n, H, W], d loss / d disparity (with ``into``: the sum of both losses' maps)
    glogvar: float32 [n, H, W], d loss / d logvar; None without uncertainty
    rows:    float64 [n, 8]
    count:   int32 [1], the labelled pixels of the batch (with ``into``: plus the counted pixels of the other loss;
             the AdamW gate reads it)
    labels:  int16 [n, H, W], the matcher's 16 * disparity"""

    __slots__ = ("gdisp", "glogvar", "rows", "count", "labels", "_pin", "_device", "_w")

    def __init__(self, gdisp, glogvar, rows, count, labels, pin, device, w):
        self.gdisp, self.glogvar, self.rows, self.count, self.labels = gdisp, glogvar, rows, count, labels
        self._pin, self._device, self._w = pin, device, w

    def summary(self) -> dict:
        """The dict of ``SUMMARY_KEYS`` over the batch. One copy of ``rows`` through a pinned buffer and the only host
        synchronisation."""
        n = self.rows.shape[0]
        self._pin[:n].copy_(self.rows, non_blocking=True)
        torch.cuda.current_stream(self._device).synchronize()
        return summary_from_rows(self._pin[:n].numpy().copy(), self.labels.numel(), self._w)


class ProxyLoss:
    """A ``StereoSGM``, ``sd_proxy_gray`` and ``sd_proxy_loss`` with their buffers: up to ``streams`` (1..64, the
    matcher's ``MAX_STREAMS``) samples of one size per call. Buffers are made once per size and only grow, and the next
    call overwrites them; ``run`` issues launches only. ``totals`` accumulates the rows of every run on the device;
    ``means()`` reads them. ``matcher_kw`` are ``StereoSGM``'s other parameters, among them ``cost="census"`` and
    ``census_window=(rows, columns)``: labels from the census / Hamming cost, which a difference in gain, exposure or
    gamma between the two sensors does not move. The defaults are parameters, not measured optima."""

    def __init__(self, streams: int = 16, w_proxy=1.0, uncertainty: bool = True, device="cuda", num_disparities=64,
                 block_size=5, mode="3way", **matcher_kw):
        n = int(streams)
        if not 1 <= n <= MAX_STREAMS:
            raise ValueError(f"streams must be in [1, {MAX_STREAMS}], got {streams}")
        self.streams = n
        self.w_proxy = proxy_param(w_proxy)
        self.uncertainty = bool(uncertainty)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"ProxyLoss runs only on a HIP device (no CPU path), got {device}")
        self.matcher = StereoSGM(num_disparities=num_disparities, block_size=block_size, mode=mode, **matcher_kw)
        self._gray = self._q4 = self._disp = self._logvar = self._gdisp = self._glogvar = None
        self._rows = self._work = self._count = self._pin = self._totals = self._inc = self._tpin = None
        self.last = None  # the ProxyResult of the last adapt_step

    def describe(self) -> dict:
        m = self.matcher
        return {"w_proxy": self.w_proxy, "uncertainty": self.uncertainty, "min_disparity": m.min_disparity,
                "num_disparities": m.num_disparities, "block_size": m.block_size, "mode": m.mode, "P1": m.P1, "P2": m.P2,
                "disp12_max_diff": m.disp12_max_diff, "uniqueness_ratio": m.uniqueness_ratio,
                "speckle_window_size": m.speckle_window_size, "speckle_range": m.speckle_range,
                "pre_filter_cap": m.pre_filter_cap, "cost": m.cost,
                "census_window": None if m.census_window is None else list(m.census_window)}

    def _bind_device(self, t: torch.Tensor):
        if self.device.index is None:
            self.device = torch.device("cuda", t.device.index)
        if t.device != self.device:
            raise ValueError(f"the tensor is on {t.device}, the proxy loss on {self.device}")

    def _check_inputs(self, inputs, n=None, H=None, W=None):
        if not isinstance(inputs, torch.Tensor) or inputs.dtype != torch.float32 or not inputs.is_cuda \
                or inputs.dim() != 4 or inputs.shape[1] != 6:
            raise ValueError("inputs must be a float32 device tensor [n, 6, H, W]")
        self._bind_device(inputs)
        shape = (int(inputs.shape[0]), int(inputs.shape[2]), int(inputs.shape[3]))
        if n is not None and shape != (n, H, W):
            raise ValueError(f"inputs must be a float32 tensor of {(n, 6, H, W)} on {self.device}")
        if not 1 <= shape[0] <= self.streams:
            raise ValueError(f"1..{self.streams} samples, got {shape[0]}")
        check_width(shape[2], self.matcher.min_disparity, self.matcher.num_disparities)
        if shape[2] > MAX_WIDTH:
            raise ValueError(f"width {shape[2]} exceeds {MAX_WIDTH}")
        return shape

    def maps(self, n: int, H: int, W: int):
        """The proxy object's own (disp, logvar) float32 [n, 1, H, W] for the heads to write into in the labels-only
        step (logvar None without uncertainty)."""
        if not 1 <= n <= self.streams:
            raise ValueError(f"1..{self.streams} samples, got {n}")
        px = n * H * W
        with torch.cuda.device(self.device):
            disp = L.grow(self, "_disp", px, torch.float32)[:px].view(n, 1, H, W)
            logvar = L.grow(self, "_logvar", px, torch.float32)[:px].view(n, 1, H, W) if self.uncertainty else None
        return disp, logvar

    def labels(self, inputs: torch.Tensor) -> torch.Tensor:
        """inputs: float32 [n, 6, H, W] on the device, the model's input batch. Returns int16 [n, H, W], the matcher's
        16 * disparity of every pair (``matcher.invalid_value`` where it keeps none), a view of the object's buffer:
        ``sd_proxy_gray``, then ``StereoSGM.compute_batch``. Launches only."""
        n, H, W = self._check_inputs(inputs)
        inputs = inputs.contiguous()
        px = n * H * W
        with torch.cuda.device(self.device):
            gray = L.grow(self, "_gray", 2 * px, torch.uint8)
            gl, gr = gray[:px].view(n, H, W), gray[px:2 * px].view(n, H, W)
            q4 = L.grow(self, "_q4", px, torch.int16)[:px].view(n, H, W)
            L.call("sd_proxy_gray", n, inputs.data_ptr(), H, W, gl.data_ptr(), gr.data_ptr(),
                   L.stream_handle(self.device))
            self.matcher.compute_batch(gl, gr, out=q4)
        return q4

    @property
    def totals(self) -> torch.Tensor:
        """float64 [8] on the device: the columns of ``rows`` summed over every sample of every ``run`` since
        ``reset()``, then the number of runs and of pixels."""
        if self._totals is None:
            with torch.inference_mode(False):
                self._totals = torch.zeros(ROW, dtype=torch.float64, device=self.device)
                self._inc = torch.zeros(ROW, dtype=torch.float64, device=self.device)
        return self._totals

    def reset(self):
        self.totals.zero_()

    def means(self, since=None) -> dict | None:
        """``summary_from_rows`` of the totals (minus ``since``, an earlier host copy of them), pixel-weighted over the
        runs, plus ``steps``; None when nothing ran. One pinned copy, one synchronisation. ``last_totals`` is the host
        copy to hand back as ``since``."""
        if self._tpin is None:
            self._tpin = torch.zeros(ROW, dtype=torch.float64).pin_memory()
        self._tpin.copy_(self.totals, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        t = self._tpin.numpy().copy()
        self.last_totals = t.copy()
        if since is not None:
            t -= np.asarray(since, dtype=np.float64)
        if t[TOTAL_STEPS] <= 0:
            return None
        rows = t.copy()
        rows[TOTAL_STEPS:] = 0.0
        out = summary_from_rows(rows, int(t[TOTAL_PIXELS]), self.w_proxy)
        out["steps"] = int(t[TOTAL_STEPS])
        return out

    def run(self, disp: torch.Tensor, logvar: torch.Tensor | None, inputs: torch.Tensor,
            into: SelfSupResult | None = None, count: torch.Tensor | None = None,
            labels: torch.Tensor | None = None) -> ProxyResult:
        """disp: float32 [n, H, W] or [n, 1, H, W] on the device, the heads' disparity in pixels of the input frames.
        logvar: the same shape, or None (required with ``uncertainty``, ignored without). inputs: float32 [n, 6, H, W],
        the model's input batch, which ``labels`` is run on. into: a ``SelfSupResult`` of the same outputs whose maps
        the gradient is added onto (its count must then be ``count``, or its own); by default the maps are the
        object's own and every pixel is written. count: an int32 device tensor of one element that receives the
        labelled pixels (with ``into``: added onto what it holds); by default ``into``'s, else the object's own.
        labels: an int16 [n, H, W] map to use instead of running the matcher (labels made elsewhere; ``inputs`` is then
        not read). Every error is raised before a launch; launches only."""
        if not isinstance(disp, torch.Tensor) or disp.dtype != torch.float32 or not disp.is_cuda:
            raise ValueError("run takes a float32 device tensor [n, H, W] or [n, 1, H, W]")
        if disp.dim() == 4 and disp.shape[1] == 1:
            disp = disp[:, 0]
        if disp.dim() != 3:
            raise ValueError("run takes a float32 device tensor [n, H, W] or [n, 1, H, W]")
        self._bind_device(disp)
        n, H, W = (int(v) for v in disp.shape)
        if not 1 <= n <= self.streams:
            raise ValueError(f"run takes 1..{self.streams} samples, got {n}")
        if not self.uncertainty:
            logvar = None
        elif logvar is None:
            raise ValueError("uncertainty=True needs the logvar map")
        if logvar is not None:
            if logvar.dim() == 4 and logvar.shape[1] == 1:
                logvar = logvar[:, 0]
            if logvar.dtype != torch.float32 or tuple(logvar.shape) != (n, H, W) or logvar.device != self.device:
                raise ValueError(f"logvar must be a float32 tensor of {(n, H, W)} on {self.device}")
            logvar = logvar.contiguous()
        if labels is None:
            self._check_inputs(inputs, n, H, W)
        elif (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int16 or tuple(labels.shape) != (n, H, W)
                or labels.device != self.device):
            raise ValueError(f"labels must be an int16 tensor of {(n, H, W)} on {self.device}")
        if into is not None:
            if tuple(into.gdisp.shape) != (n, H, W) or into.gdisp.device != self.device \
                    or not into.gdisp.is_contiguous():
                raise ValueError(f"into must hold contiguous maps of {(n, H, W)} on {self.device}")
            if (into.glogvar is None) != (logvar is None):
                raise ValueError("into and the proxy loss must agree on uncertainty (a glogvar map or none)")
            if count is None:
                count = into.count
        if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or count.device != self.device):
            raise ValueError("count must be an int32 device tensor of one element")
        disp = disp.contiguous()
        px = n * H * W
        q4 = self.labels(inputs) if labels is None else labels.contiguous()
        with torch.cuda.device(self.device):
            if into is None:
                gdisp = L.grow(self, "_gdisp", px, torch.float32)[:px].view(n, H, W)
                glogvar = L.grow(self, "_glogvar", px, torch.float32)[:px].view(n, H, W) if logvar is not None else None
            else:
                gdisp, glogvar = into.gdisp, into.glogvar
            rows = L.grow(self, "_rows", self.streams * ROW, torch.float64)[:n * ROW].view(n, ROW)
            work = L.grow(self, "_work", L.call("sd_proxy_ws_bytes", n, H, W) // 8, torch.float64)
            if count is None:
                count = L.grow(self, "_count", 1, torch.int32)
            if self._pin is None:
                self._pin = torch.zeros(self.streams, ROW, dtype=torch.float64).pin_memory()
            totals = self.totals
            L.call("sd_proxy_loss", n, disp.data_ptr(), L.ptr(logvar), q4.data_ptr(), H, W, self.w_proxy,
                   int(into is not None), gdisp.data_ptr(), L.ptr(glogvar), rows.data_ptr(), count.data_ptr(),
                   work.data_ptr(), L.stream_handle(self.device))
            # rows[6..7] are 0, so the steps and pixels ride in those two slots of the totals
            with torch.no_grad():
                totals.add_(rows.sum(dim=0))
                if getattr(self, "_inc_px", None) != px:
                    self._inc.zero_()
                    self._inc[TOTAL_STEPS] = 1.0
                    self._inc[TOTAL_PIXELS] = float(px)
                    self._inc_px = px
                totals.add_(self._inc)
        return ProxyResult(gdisp, glogvar, rows, count, q4, self._pin, self.device, self.w_proxy)
