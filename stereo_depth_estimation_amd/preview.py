"""Per-epoch preview montages — mirror of the reference's ``train.py:254-289`` (``log_epoch_previews``) and
``eval_utils.py:42-73`` (``_normalize_map``, ``save_preview_montage``).

For each preview sample one PNG of four panels, ``left | right | gray(target) | gray(pred)``; the two maps are
normalised to the 5th-95th percentile of their own finite values. The reference copies input, target and prediction
to the host and sorts them there with NumPy; here the percentiles are an exact radix select on the device
(``sd_quantile_select_n``) and the bytes are composed there (``sd_preview_compose_n``), so one uint8 montage batch per
loader batch crosses to the host, where it is written as PNG with the standard library alone.

Nothing here draws from a random generator or touches a BatchNorm buffer: a run with previews trains bit for bit as
a run without.
"""

from __future__ import annotations

import struct
import zlib
from pathlib import Path

import numpy as np
import torch

from . import _lib as L

Q_LO, Q_HI = 0.05, 0.95  # eval_utils.py:47-48
MAX_BATCH = 64  # samples per select / compose call (the entry points' limit)

_buffers: dict = {}  # (device, chunk size) -> (select workspace, sel of target, sel of pred)


def _select_buffers(device: torch.device, m: int):
    """The zeroed select workspace (every call leaves it zero) and the two ``sel`` row buffers, kept per device and
    chunk size."""
    key = (device.type, device.index, m)
    if key not in _buffers:
        words = L.call("sd_quantile_select_ws_bytes", m) // 4
        with torch.inference_mode(False):  # ordinary tensors: they outlive the inference-mode block of the first call
            _buffers[key] = (torch.zeros(words, dtype=torch.int32, device=device),
                             torch.zeros((m, 8), dtype=torch.float32, device=device),
                             torch.zeros((m, 8), dtype=torch.float32, device=device))
    return _buffers[key]


def _f32(t: torch.Tensor, shape) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.reshape(shape).contiguous()


def montages(inputs: torch.Tensor, targets: torch.Tensor, preds: torch.Tensor, out: torch.Tensor | None = None):
    """uint8 ``[B, H, 4W, 3]`` device tensor of the reference's montages (``save_preview_montage``) of a batch:
    ``inputs`` ``[B, 6, H, W]``, ``targets`` and ``preds`` ``[B, 1, H, W]`` (or ``[B, H, W]``). Two select calls and one
    compose call per chunk of up to 64 samples, on the current stream; no synchronisation."""
    if inputs.dim() != 4 or inputs.shape[1] != 6:
        raise ValueError(f"montages: inputs must be [B, 6, H, W], got {tuple(inputs.shape)}")
    B, _, H, W = inputs.shape
    device = inputs.device
    if device.type != "cuda":
        raise RuntimeError(f"montages composes on a HIP device; got {device}. There is no CPU fallback.")
    if targets.numel() != B * H * W or preds.numel() != B * H * W:
        raise ValueError(f"montages: targets / preds must hold B * H * W = {B * H * W} values, got "
                         f"{tuple(targets.shape)} / {tuple(preds.shape)}")
    if targets.device != device or preds.device != device:
        raise ValueError("montages: inputs, targets and preds must be on one device")
    inp, tgt, prd = _f32(inputs, (B, 6, H, W)), _f32(targets, (B, H, W)), _f32(preds, (B, H, W))
    if out is None:
        out = torch.empty((B, H, 4 * W, 3), dtype=torch.uint8, device=device)
    elif (tuple(out.shape) != (B, H, 4 * W, 3) or out.dtype != torch.uint8 or out.device != device
          or not out.is_contiguous()):
        raise ValueError(f"montages: out must be a contiguous uint8 tensor of {(B, H, 4 * W, 3)} on {device}")
    with torch.cuda.device(device):
        s = L.stream_handle(device)
        for b0 in range(0, B, MAX_BATCH):
            m = min(MAX_BATCH, B - b0)
            work, sel_t, sel_p = _select_buffers(device, m)
            t, p = tgt[b0:b0 + m], prd[b0:b0 + m]
            L.call("sd_quantile_select_n", m, t.data_ptr(), H * W, Q_LO, Q_HI, work.data_ptr(), sel_t.data_ptr(), s)
            L.call("sd_quantile_select_n", m, p.data_ptr(), H * W, Q_LO, Q_HI, work.data_ptr(), sel_p.data_ptr(), s)
            L.call("sd_preview_compose_n", m, inp[b0:b0 + m].data_ptr(), t.data_ptr(), p.data_ptr(), H, W,
                   sel_t.data_ptr(), sel_p.data_ptr(), out[b0:b0 + m].data_ptr(), s)
    return out


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, rgb_u8, level: int = 6) -> None:
    """An 8-bit RGB, non-interlaced PNG of a uint8 ``[H, W, 3]`` array: filter type 0 on every row, one zlib stream."""
    a = np.ascontiguousarray(rgb_u8.cpu().numpy() if isinstance(rgb_u8, torch.Tensor) else rgb_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected uint8 [H, W, 3], got {a.dtype} {a.shape}")
    h, w, _ = a.shape
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)  # byte 0 of a row: filter type 0 (None)
    rows[:, 1:] = a.reshape(h, 3 * w)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)  # 8 bits, colour type 2 (RGB), deflate, adaptive set, no interlace
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level))
           + _chunk(b"IEND", b""))
    Path(path).write_bytes(png)


def preview_path(preview_root, epoch: int, batch_index: int, inner_index: int) -> Path:
    """train.py:261,275-277."""
    return Path(preview_root) / f"epoch_{epoch:04d}" / f"sample_{batch_index:03d}_{inner_index:02d}.png"


def log_epoch_previews(model, loader, device, epoch: int, preview_root) -> int:
    """train.py:254-289: an eval forward of every loader batch under ``torch.inference_mode()`` and one montage PNG per
    sample in ``<preview_root>/epoch_XXXX/``. One montage batch and one device-to-host copy per loader batch.
    ``model.training`` is restored. Returns the number of files written."""
    previews_dir = preview_path(preview_root, epoch, 0, 0).parent
    previews_dir.mkdir(parents=True, exist_ok=True)
    was_training = model.training
    model.eval()
    written = 0
    try:
        with torch.inference_mode():
            for batch_index, batch in enumerate(loader):
                inputs = batch["input"].to(device, non_blocking=True)
                targets = batch["target"].to(device, non_blocking=True)
                preds = model(inputs)
                host = montages(inputs, targets, preds).cpu().numpy()
                for inner_index in range(host.shape[0]):
                    write_png(preview_path(preview_root, epoch, batch_index, inner_index), host[inner_index])
                    written += 1
    finally:
        if was_training:
            model.train()
    return written
