"""Uncertainty evaluation: does the log-variance head rank the errors, and does it have the right size?

``sd_uncert_eval`` (csrc/uncert.hip; include/stereo_hip.h and INTEGRATION.md "Uncertainty evaluation" state the
arithmetic) takes the two heads' maps at the model resolution and the native RGB24 ground truth and gives one float64
row per sample: the sparsification curve of the predicted uncertainty and the oracle's, their areas AUSE / AURG, the
coverage counts at 0.5, 1, 2 and 3 times the predicted Laplace scale, and the NLL sum in the training log's form. The
curves come from integer histograms, tied pixels sharing the cut: no sort, and no dependence on any order.

``UncertaintyEval`` owns the device buffers; ``summary_from_row`` and ``aggregate_rows`` turn rows into the figures
``predict --eval-uncertainty`` and ``adapt --eval-uncertainty`` record.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

HEAD = 16  # doubles of a row ahead of the two curves
MAX_STEPS = 256
COVERAGE_Z = (0.5, 1.0, 2.0, 3.0)
COVERAGE_NOMINAL = tuple(1.0 - math.exp(-z) for z in COVERAGE_Z)  # Laplace with b = exp(logvar)


def row_len(steps: int) -> int:
    return HEAD + 2 * int(steps)


def check_steps(steps) -> int:
    if int(steps) != steps or not 1 <= int(steps) <= MAX_STEPS:
        raise ValueError(f"sparsification steps must be an integer in [1, {MAX_STEPS}], got: {steps}")
    return int(steps)


class UncertaintyEval:
    """The device stage: ``run`` queues ``sd_uncert_eval`` on the current stream. The workspace and the rows buffer are
    kept per (n, Hs, Ws) and reused; the result is a view of the rows buffer, overwritten by the next ``run`` of that
    key."""

    def __init__(self, steps: int = 20, device=None):
        L.load()
        self.steps = check_steps(steps)
        self.device = torch.device(device) if device is not None else None
        self._buf: dict = {}

    def _buffers(self, n: int, Hs: int, Ws: int, device) -> tuple:
        key = (n, Hs, Ws, device)
        b = self._buf.get(key)
        if b is None:
            ws = L.call("sd_uncert_eval_ws_bytes", n, Hs, Ws, self.steps)
            if ws < 0:
                raise ValueError(f"UncertaintyEval: sizes out of range: n = {n}, {Hs} x {Ws}")
            with torch.inference_mode(False):
                b = (torch.empty(n, row_len(self.steps), device=device, dtype=torch.float64),
                     torch.empty(ws // 8, device=device, dtype=torch.float64))
            self._buf[key] = b
        return b

    def run(self, disp: torch.Tensor, logvar: torch.Tensor, gt_rgb: torch.Tensor, out_hw=None) -> torch.Tensor:
        """disp, logvar: contiguous float32 [n,H,W] or [n,1,H,W] on a HIP device; gt_rgb: contiguous uint8 [n,Hs,Ws,3],
        the RGB24 ground truth; out_hw = (Hs, Ws), by default gt_rgb's. Returns float64 [n, 16 + 2 steps] on the device
        without synchronising."""
        n, H, W = int(disp.shape[0]), int(disp.shape[-2]), int(disp.shape[-1])
        Hs, Ws = (int(v) for v in (out_hw if out_hw is not None else gt_rgb.shape[1:3]))
        dev = disp.device
        if dev.type != "cuda" or (self.device is not None and dev != self.device):
            raise RuntimeError(f"UncertaintyEval runs only on a HIP device (no CPU path); the maps are on {dev}")
        for name, t in (("disp", disp), ("logvar", logvar)):
            if t.dtype != torch.float32 or t.numel() != n * H * W or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"UncertaintyEval.run: {name} must be a contiguous float32 tensor of {(n, H, W)} on "
                                 f"{dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if (tuple(gt_rgb.shape) != (n, Hs, Ws, 3) or gt_rgb.dtype != torch.uint8 or not gt_rgb.is_contiguous()
                or gt_rgb.device != dev):
            raise ValueError(f"UncertaintyEval.run: gt_rgb must be a contiguous uint8 tensor of {(n, Hs, Ws, 3)} on "
                             f"{dev}, got {gt_rgb.dtype} {tuple(gt_rgb.shape)} on {gt_rgb.device}")
        rows, work = self._buffers(n, Hs, Ws, dev)
        with torch.cuda.device(dev):
            L.call("sd_uncert_eval", disp.data_ptr(), logvar.data_ptr(), n, H, W, gt_rgb.data_ptr(), Hs, Ws, self.steps,
                   rows.data_ptr(), work.data_ptr(), L.stream_handle(dev))
        return rows


def _split(row, steps: int):
    r = np.asarray(row, dtype=np.float64).reshape(-1)
    if r.size != row_len(steps):
        raise ValueError(f"a row of {steps} steps holds {row_len(steps)} doubles, got {r.size}")
    return r, r[HEAD:HEAD + steps], r[HEAD + steps:]


def _normalised(curve: np.ndarray, u0: float) -> list:
    return [float(v) / u0 if u0 > 0 else 0.0 for v in curve]


def summary_from_row(row, steps: int) -> dict:
    """The figures of one sample's row; None for each when no pixel counted. ``sparsification`` is unc / unc_0 and
    ``sparsification_oracle`` orc / unc_0 (zeros when unc_0 == 0: no error to remove)."""
    r, unc, orc = _split(row, steps)
    n = r[0]
    out = {"valid_pixels": int(n), "steps": int(steps), "coverage_nominal": {str(z): p for z, p in
                                                                              zip(COVERAGE_Z, COVERAGE_NOMINAL)}}
    if n <= 0:
        out.update(nll=None, coverage=None, ause=None, aurg=None, sparsification=None, sparsification_oracle=None,
                   saturated_pixels=None)
        return out
    u0 = float(unc[0])
    out.update(nll=float(r[2]) / n, coverage={str(z): float(r[3 + i]) / n for i, z in enumerate(COVERAGE_Z)},
               ause=float(r[7]), aurg=float(r[8]), sparsification=_normalised(unc, u0),
               sparsification_oracle=_normalised(orc, u0),
               saturated_pixels={"logvar": int(r[9]), "error": int(r[10])})
    return out


def aggregate_rows(rows, steps: int) -> dict:
    """Figures over samples, rows [N][16 + 2 steps]. The pixel-weighted ones (``nll``, ``coverage``, the saturation
    counts) come from the column sums in fp64, as ``predict.aggregate_rows`` forms its own. ``ause``, ``aurg`` and the
    two normalised curves are NOT pixel-weighted: a curve is a property of one sample's ranking, so they are the plain
    mean over the samples with n > 0, added in index order. None for each when no sample has a counted pixel."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, row_len(steps))
    tot = rows.sum(axis=0)
    n = tot[0]
    out = {"valid_pixels": int(n), "steps": int(steps), "samples": int((rows[:, 0] > 0).sum()),
           "coverage_nominal": {str(z): p for z, p in zip(COVERAGE_Z, COVERAGE_NOMINAL)}}
    if n <= 0:
        out.update(nll=None, coverage=None, ause=None, aurg=None, sparsification=None, sparsification_oracle=None,
                   saturated_pixels=None)
        return out
    ause = aurg = 0.0
    spars, oracle = [0.0] * steps, [0.0] * steps
    for row in rows:
        if row[0] <= 0:
            continue
        s = summary_from_row(row, steps)
        ause += s["ause"]
        aurg += s["aurg"]
        spars = [a + b for a, b in zip(spars, s["sparsification"])]
        oracle = [a + b for a, b in zip(oracle, s["sparsification_oracle"])]
    k = out["samples"]
    out.update(nll=float(tot[2]) / n, coverage={str(z): float(tot[3 + i]) / n for i, z in enumerate(COVERAGE_Z)},
               ause=ause / k, aurg=aurg / k, sparsification=[v / k for v in spars],
               sparsification_oracle=[v / k for v in oracle],
               saturated_pixels={"logvar": int(tot[9]), "error": int(tot[10])})
    return out
