"""Label-free adaptation on the device: a photometric + smoothness loss from the two frames alone, and the training step
built on it (no counterpart in the reference, whose only objective is the masked NLL against a label).

    loss = SelfSupLoss(streams=16)                       # w_photo=1, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10
    opt = FusedAdamW(model.parameters(), lr=1e-5, weight_decay=0.0)
    for batch in loader:                                 # {"input": float32 [n, 6, H, W]}: left RGB / 255, then right
        adapt_step(model, opt, batch["input"], loss)     # launches only, no host sync
    print(loss.means())                                  # the only sync: one pinned copy of eight doubles

The objective is the standard self-supervised stereo one: the left view is reconstructed from the right one through the
predicted disparity (``sd_stereo_check``'s warp, on floats), the Charbonnier error of the reconstruction is averaged over
the pixels the geometry-only check calls visible (class 0: a value, in view, not occluded), weighted by the predicted
uncertainty in the reference's NLL form (``e * exp(-lv) + lv``; ``uncertainty=False``: plain ``e``), and an edge-aware
first-order smoothness term runs over every pixel pair. The arithmetic is ``sd_selfsup_loss``'s (include/stereo_hip.h,
INTEGRATION.md "sd_selfsup_loss"); it is held to the NumPy restatement tests/selfsup_ref.py. Kernels: csrc/selfsup.hip.
There is no CPU fallback.

``SelfSupLoss(..., ssim=0.85)`` mixes a structural term into the photometric error, e' = (1 - ssim) e + ssim s with s
the SSIM dissimilarity of the 3 x 3 window of counted pixels around each pixel: two sensors of a real rig never agree in
gain, exposure or white balance, which gives an absolute colour difference a floor that no disparity removes, whereas
SSIM compares local structure and is largely insensitive to gain and offset. The stage is then ``sd_selfsup_loss_ssim``
(csrc/selfsup_ssim.hip, INTEGRATION.md "sd_selfsup_loss_ssim", restated in tests/selfsup_ssim_ref.py). The default is 0:
the stage and every byte are then ``sd_selfsup_loss``'s. 0.85 is the literature's mix, not an optimum measured here.

``adapt_step(..., proxy=ProxyLoss(...))`` adds proxy supervision (proxy.py): the semi-global matcher labels the pixels
it is sure of, and their gradient is added onto this loss's maps; ``loss=None`` trains on the labels alone.

The frames are taken as rectified: a pixel (x, y) of the left frame is looked for at (x - d, y) of the right frame. The
defaults (``w_photo`` = 1, ``w_smooth`` = 0.1, ``eps`` = ``eps_s`` = 0.01, ``gamma`` = 10, ``occ_tol`` = 0.5 px) are
parameters and not measured optima: how much smoothness a scene bears, and how sharp an image edge must be before a
disparity edge is free, depend on the rig and the scene.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .check import StereoCheck, check_params

MAX_SAMPLES = 65535
STEP_PIXELS = 1024  # csrc/selfsup.hip SS_STEP: pixels per step of a block's walk over its rows, four per thread
ROW = 8             # doubles per sample: counted, sum l, sum e, sum smoothness terms, pairs, sum |gdisp|, 0, 0
                    # (with ssim > 0: [6] sum s)
SSIM_TILE_W, SSIM_TILE_H = 32, 16  # csrc/selfsup_ssim.hip SSIM_TW, SSIM_TH: the pixels a block of the tiled pass owns
ROW_SSIM = 6        # the column of ``rows`` that holds sum s
TOTAL_SSIM = 8      # sum s over every run rides behind ``totals`` in the same buffer
SUMMARY_KEYS = ("loss", "photo", "smooth", "visible_fraction", "grad_l1")
# totals: the columns of ``rows`` summed over every sample of every step, then [6] steps and [7] pixels
TOTAL_STEPS, TOTAL_PIXELS = 6, 7


def selfsup_params(w_photo=1.0, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10.0) -> tuple[float, ...]:
    """The five parameters as the float32 values the kernel computes with: w_photo, w_smooth, gamma finite and >= 0;
    eps, eps_s finite and > 0."""
    out = []
    for name, v, strict in (("w_photo", w_photo, False), ("w_smooth", w_smooth, False), ("eps", eps, True),
                            ("eps_s", eps_s, True), ("gamma", gamma, False)):
        f = float(np.float32(v))
        if not math.isfinite(f) or f < 0 or (strict and f == 0):
            raise ValueError(f"{name} must be finite and {'> 0' if strict else '>= 0'}, got {v}")
        out.append(f)
    return tuple(out)


def ssim_param(ssim=0.0) -> float:
    """The weight of the SSIM term as the float32 value the kernel computes with: in [0, 1]."""
    f = float(np.float32(ssim))
    if not 0.0 <= f <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"ssim must be in [0, 1], got {ssim}")
    return f


def summary_from_rows(rows, pixels: int, w_photo: float, w_smooth: float) -> dict:
    """The figures of rows [k][8] (one step's samples, or the totals of many steps) over ``pixels`` pixels, in fp64:
    ``photo`` the mean Charbonnier error e over the counted pixels, ``smooth`` the mean smoothness term per pixel,
    ``loss`` = w_photo * sum l / max(1, counted) + w_smooth * smooth (what ``gdisp`` is the gradient of),
    ``visible_fraction`` counted / pixels, ``grad_l1`` sum |gdisp|."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, ROW).sum(axis=0)
    counted, px = float(r[0]), max(float(pixels), 1.0)
    smooth = float(r[3]) / px
    return {"loss": w_photo * float(r[1]) / max(counted, 1.0) + w_smooth * smooth,
            "photo": float(r[2]) / counted if counted > 0 else None, "smooth": smooth,
            "visible_fraction": counted / px, "grad_l1": float(r[5])}


class SelfSupResult:
    """Device tensors of one ``SelfSupLoss.run`` (views of the loss object's buffers: its next run overwrites them).

    gdisp:   float32 [n, H, W], d loss / d disparity
    glogvar: float32 [n, H, W], d loss / d logvar; None without uncertainty
    rows:    float64 [n, 8]
    count:   int32 [1], the counted pixels of the batch (the AdamW gate reads it)
    cls:     uint8 [n, H, W], the geometry-only classes of ``check.CLASSES``"""

    __slots__ = ("gdisp", "glogvar", "rows", "count", "cls", "_pin", "_device", "_w", "_ssim")

    def __init__(self, gdisp, glogvar, rows, count, cls, pin, device, w, ssim=False):
        self.gdisp, self.glogvar, self.rows, self.count, self.cls = gdisp, glogvar, rows, count, cls
        self._pin, self._device, self._w, self._ssim = pin, device, w, ssim

    def summary(self) -> dict:
        """The dict of ``SUMMARY_KEYS`` over the batch (with ``ssim`` > 0 also ``"ssim"``, the mean s over the counted
        pixels, None when nothing counted). One copy of ``rows`` through a pinned buffer and the only host
        synchronisation."""
        n = self.rows.shape[0]
        self._pin[:n].copy_(self.rows, non_blocking=True)
        torch.cuda.current_stream(self._device).synchronize()
        rows = self._pin[:n].numpy().copy()
        out = summary_from_rows(rows, self.gdisp.numel(), *self._w)
        if self._ssim:
            counted = float(rows[:, 0].sum())
            out["ssim"] = float(rows[:, ROW_SSIM].sum()) / counted if counted > 0 else None
        return out


class SelfSupLoss:
    """``sd_stereo_check`` (geometry only) and ``sd_selfsup_loss`` with their buffers: up to ``streams`` (1..65535)
    samples of one size per call, five launches whatever their number. Buffers are made once per size and only grow;
    ``run`` issues launches only. ``totals`` accumulates the rows of every run on the device; ``means()`` reads them.
    ``ssim`` in [0, 1] is the weight of the SSIM term in the photometric error (0: none, and ``sd_selfsup_loss`` as it
    always was; above 0 the stage is ``sd_selfsup_loss_ssim``; 0.85 is the literature's mix, not a measured optimum)."""

    def __init__(self, streams: int = 1, w_photo=1.0, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10.0, occ_tol=0.5,
                 uncertainty: bool = True, device="cuda", ssim=0.0):
        n = int(streams)
        if not 1 <= n <= MAX_SAMPLES:
            raise ValueError(f"streams must be in [1, {MAX_SAMPLES}], got {streams}")
        self.streams = n
        self.w_photo, self.w_smooth, self.eps, self.eps_s, self.gamma = selfsup_params(w_photo, w_smooth, eps, eps_s,
                                                                                       gamma)
        self.occ_tol, _ = check_params(occ_tol, math.inf)
        self.ssim = ssim_param(ssim)
        self.uncertainty = bool(uncertainty)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SelfSupLoss runs only on a HIP device (no CPU path), got {device}")
        self.check = StereoCheck(n, self.device)
        self._disp = self._logvar = self._gdisp = self._glogvar = self._rows = self._work = None
        self._count = self._pin = self._totals = self._inc = self._tpin = None

    def describe(self) -> dict:
        out = {"w_photo": self.w_photo, "w_smooth": self.w_smooth, "eps": self.eps, "eps_s": self.eps_s,
               "gamma": self.gamma, "occ_tol": self.occ_tol, "uncertainty": self.uncertainty}
        if self.ssim != 0:
            out["ssim"] = self.ssim
        return out

    def _bind_device(self, t: torch.Tensor):
        if self.device.index is None:
            self.device = torch.device("cuda", t.device.index)
        if t.device != self.device:
            raise ValueError(f"the tensor is on {t.device}, the loss on {self.device}")

    def maps(self, n: int, H: int, W: int):
        """The loss object's own (disp, logvar) float32 [n, 1, H, W] for the heads to write into (logvar None without
        uncertainty)."""
        if not 1 <= n <= self.streams:
            raise ValueError(f"1..{self.streams} samples, got {n}")
        px = n * H * W
        with torch.cuda.device(self.device):
            disp = L.grow(self, "_disp", px, torch.float32)[:px].view(n, 1, H, W)
            logvar = L.grow(self, "_logvar", px, torch.float32)[:px].view(n, 1, H, W) if self.uncertainty else None
        return disp, logvar

    @property
    def totals(self) -> torch.Tensor:
        """float64 [8] on the device: the columns of ``rows`` summed over every sample of every ``run`` since
        ``reset()``, then the number of runs and of pixels. A view of a buffer of nine doubles: the ninth is the sum of
        s (``ssim`` > 0), so that ``means()`` stays one copy."""
        if self._totals is None:
            with torch.inference_mode(False):
                self._totals9 = torch.zeros(ROW + 1, dtype=torch.float64, device=self.device)
                self._totals = self._totals9[:ROW]
                self._inc = torch.zeros(ROW, dtype=torch.float64, device=self.device)
        return self._totals

    def reset(self):
        self.totals  # noqa: B018 (makes the buffer)
        self._totals9.zero_()

    def means(self, since=None) -> dict | None:
        """``summary_from_rows`` of the totals (minus ``since``, an earlier host copy of them), pixel-weighted over the
        runs, plus ``steps`` and, with ``ssim`` > 0, ``ssim``: the mean s over the counted pixels; None when nothing ran.
        One pinned copy, one synchronisation. ``last_totals`` is the host copy to hand back as ``since`` (with ``ssim``
        > 0 it carries the sum of s as a ninth value)."""
        if self._tpin is None:
            self._tpin = torch.zeros(ROW + 1, dtype=torch.float64).pin_memory()
        self.totals  # noqa: B018 (makes the buffer)
        self._tpin.copy_(self._totals9, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        t9 = self._tpin.numpy().copy()
        self.last_totals = (t9 if self.ssim != 0 else t9[:ROW]).copy()
        if since is not None:
            since = np.asarray(since, dtype=np.float64)
            t9[:len(since)] -= since
        t = t9[:ROW]
        if t[TOTAL_STEPS] <= 0:
            return None
        out = summary_from_rows(t, int(t[TOTAL_PIXELS]), self.w_photo, self.w_smooth)
        out["steps"] = int(t[TOTAL_STEPS])
        if self.ssim != 0:
            out["ssim"] = float(t9[TOTAL_SSIM]) / float(t[0]) if t[0] > 0 else None
        return out

    def run(self, disp: torch.Tensor, logvar: torch.Tensor | None, inputs: torch.Tensor,
            count: torch.Tensor | None = None) -> SelfSupResult:
        """disp: float32 [n, H, W] or [n, 1, H, W] on the device, the heads' disparity in pixels of the input frames.
        logvar: the same shape, or None (required with ``uncertainty``, ignored without). inputs: float32 [n, 6, H, W],
        the model's input batch. count: an int32 device tensor of one element to receive the counted pixels (the
        engine's count slot in ``adapt_step``); by default the loss object's own. Launches only."""
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
        if (not isinstance(inputs, torch.Tensor) or inputs.dtype != torch.float32
                or tuple(inputs.shape) != (n, 6, H, W) or inputs.device != self.device):
            raise ValueError(f"inputs must be a float32 tensor of {(n, 6, H, W)} on {self.device}")
        if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or count.device != self.device):
            raise ValueError("count must be an int32 device tensor of one element")
        disp, inputs = disp.contiguous(), inputs.contiguous()
        px = n * H * W
        chk = self.check.run(disp, occ_tol=self.occ_tol, want=("cls", "rows"))
        with torch.cuda.device(self.device):
            gdisp = L.grow(self, "_gdisp", px, torch.float32)[:px].view(n, H, W)
            glogvar = L.grow(self, "_glogvar", px, torch.float32)[:px].view(n, H, W) if logvar is not None else None
            rows = L.grow(self, "_rows", self.streams * ROW, torch.float64)[:n * ROW].view(n, ROW)
            ws = "sd_selfsup_ssim_ws_bytes" if self.ssim != 0 else "sd_selfsup_ws_bytes"
            work = L.grow(self, "_work", L.call(ws, n, H, W) // 8, torch.float64)
            if count is None:
                count = L.grow(self, "_count", 1, torch.int32)
            if self._pin is None:
                self._pin = torch.zeros(self.streams, ROW, dtype=torch.float64).pin_memory()
            head = (n, disp.data_ptr(), L.ptr(logvar), inputs.data_ptr(), chk.cls.data_ptr(), chk.rows.data_ptr(), H, W,
                    self.w_photo, self.w_smooth, self.eps, self.eps_s, self.gamma)
            tail = (gdisp.data_ptr(), L.ptr(glogvar), rows.data_ptr(), count.data_ptr(), work.data_ptr(),
                    L.stream_handle(self.device))
            totals = self.totals
            if self.ssim != 0:
                L.call("sd_selfsup_loss_ssim", *head, self.ssim, *tail)
                # rows[6] is the sum of s here: it goes behind the totals, whose [6] and [7] stay steps and pixels
                with torch.no_grad():
                    sums = rows.sum(dim=0)
                    self._totals9[:ROW_SSIM].add_(sums[:ROW_SSIM])
                    self._totals9[TOTAL_SSIM:].add_(sums[ROW_SSIM:ROW_SSIM + 1])
                    self._add_step(px)
            else:
                L.call("sd_selfsup_loss", *head, *tail)
                # the per-interval sums: rows[6..7] are 0, so the steps and pixels ride in those two slots
                with torch.no_grad():
                    totals.add_(rows.sum(dim=0))
                    self._add_step(px)
        return SelfSupResult(gdisp, glogvar, rows, count, chk.cls, self._pin, self.device,
                             (self.w_photo, self.w_smooth), self.ssim != 0)

    def _add_step(self, px: int):
        """totals[6] += 1, totals[7] += px, without a host-to-device copy per run: the increment vector is refilled only
        when the batch's pixel count changes."""
        if getattr(self, "_inc_px", None) != px:
            self._inc.zero_()
            self._inc[TOTAL_STEPS] = 1.0
            self._inc[TOTAL_PIXELS] = float(px)
            self._inc_px = px
        self._totals.add_(self._inc)


def adapt_step(model, optimizer, inputs: torch.Tensor, loss: SelfSupLoss | None, proxy=None):
    """The label-free sibling of ``train_step``: one training step of ``model`` on ``inputs`` (float32 [n, 6, H, W] on
    the device) against ``loss``, in train mode, fp32 or bf16. Weight packs, the training forward, the heads into the
    loss object's maps, the geometry-only check, ``sd_selfsup_loss`` (its count into the engine's current count slot),
    the heads' GRADS mode, the hand-scheduled backward and AdamW, gated on the device by that count: a batch without a
    counted pixel leaves the weights alone. No host synchronisation. The sums accumulate in ``loss.totals``.

    ``proxy``: a ``proxy.ProxyLoss`` whose matcher labels train the heads as well. After ``loss.run`` its gradient is
    added onto the loss's maps and its labelled pixels onto the count, so the gate opens when either stage found pixels;
    the result is the loss's (its maps then hold the sum), the proxy's own is ``proxy.last``. ``loss=None`` with a proxy
    is the labels-only step: the heads write into the proxy's maps, no check stage and no photometric stage run, and
    the ``ProxyResult`` is returned. ``loss`` and ``proxy`` must agree on ``uncertainty``."""
    if getattr(model, "precision", None) == "fp8":
        raise RuntimeError("adapt_step: precision='fp8' is the inference-only forward; adapt in fp32 or bf16")
    if proxy is None:
        if loss is None:
            raise ValueError("adapt_step needs a loss, a proxy or both")
    elif loss is not None and bool(loss.uncertainty) != bool(proxy.uncertainty):
        raise ValueError(f"loss (uncertainty={loss.uncertainty}) and proxy (uncertainty={proxy.uncertainty}) must agree "
                         "on uncertainty")
    eng = model.engine(inputs.device)
    n, _, H, W = (int(v) for v in inputs.shape)
    if proxy is not None:
        proxy._check_inputs(inputs)  # a frame no label fits into is refused before the forward
    with torch.cuda.device(eng.device):
        eng.pack_weights(train=True)
        eng.forward(inputs, train=True)
        disp, logvar = (loss if loss is not None else proxy).maps(n, H, W)
        eng.heads(L.SD_HEADS_INFER, disp=disp, logvar=logvar)
        if loss is not None:
            res = loss.run(disp, logvar, inputs, count=eng.count)
            if proxy is not None:
                proxy.last = proxy.run(disp, logvar, inputs, into=res, count=eng.count)
        else:
            res = proxy.last = proxy.run(disp, logvar, inputs, count=eng.count)
        eng.heads(L.SD_HEADS_GRADS, gdisp=res.gdisp, glogvar=res.glogvar)
        eng.backward()
        optimizer.fused_step(gather_grads=False, gate_on_count=True)
    return res


def adapt_epoch(model, loader, device, optimizer, loss: SelfSupLoss | None, log_every_batches: int | None = None,
                logger=None, proxy=None):
    """``adapt_step`` over the batches ``{"input": float32 [n, 6, H, W]}`` of ``loader`` (any other key is ignored: labels
    are not used). Returns the epoch's pixel-weighted means (``SelfSupLoss.means``: loss, photo, smooth,
    visible_fraction, grad_l1, steps; ssim when the loss has the term). The sums are read once per ``log_every_batches`` steps (``logger.log_metrics``,
    as ``run_epoch``) and once at the end. With ``proxy`` (a ``proxy.ProxyLoss``) the means also carry its ``proxy_*``
    keys (``ProxyLoss.means``); with ``loss=None`` they are the proxy's alone."""
    model.train(True)
    if loss is None and proxy is None:
        raise ValueError("adapt_epoch needs a loss, a proxy or both")
    stages = [s for s in (loss, proxy) if s is not None]
    for s in stages:
        s._bind_device(torch.empty(0, device=device))
        s.reset()

    def read(since):
        """The stages' means merged (the loss's keys, then the proxy's ``proxy_*``), and their host totals."""
        out, tot = None, []
        for s, prev in zip(stages, since):
            m = s.means(prev)
            tot.append(s.last_totals)
            if m is None:
                continue
            if s is proxy and loss is not None:
                m = {k: v for k, v in m.items() if k.startswith("proxy_")}
            out = m if out is None else {**out, **m}
        return out, tot

    since, step = [None] * len(stages), 0
    for batch in loader:
        step += 1
        adapt_step(model, optimizer, batch["input"].to(device, non_blocking=True), loss, proxy=proxy)
        if logger is not None and log_every_batches and step % log_every_batches == 0:
            m, since = read(since)
            if m is not None:
                logger.log_metrics({f"adapt_{k}_step": v for k, v in m.items() if v is not None}, step=step)
    means, _ = read([None] * len(stages))
    if means is None:
        raise RuntimeError("No batches in this epoch.")
    return means
