"""Cache builder of the HIP path: mirror of reference ``cache.py`` (``foundation-stereo-cache``).

    python -m stereo_depth_estimation_amd.cache --dataset-root DIR --cache-root DIR [reference flags]

Pre-resizes FoundationStereo into the reference's cache (one ``.npz`` per sample: uint8 RGB, float16 disparity;
``cache_meta.json`` beside them), the input of ``--cache-root ... --require-cache`` training. Same flags, defaults,
skip / overwrite rule, metadata keys and closing lines as ``cache.py:18-112``; the entries hold what the training path
computes for a sample (``sd_stereo_to_cache`` shares its per-pixel code with ``sd_stereo_preprocess``), so a cache
built here and one left by a first epoch through ``DeviceLoader`` are interchangeable. What differs:

* samples are handled a batch at a time: PNG frames are decoded by the threaded native reader into pinned memory
  (JPEG and other frames by PIL), resized and packed to the cache's bytes on the device, and written by the native
  writer, with the decode of batch i+1, the device work of batch i and the writing of batch i-1 overlapping;
* an entry is written under a temporary name and renamed, so an interrupted build leaves no truncated entry for the
  next run to skip (the reference writes in place);
* ``--batch-size``, ``--read-threads`` and ``--device`` are new; ``--device cpu`` is rejected (no CPU path).
"""

from __future__ import annotations

import argparse
import json
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from .dataset import (discover_samples, png_size, read_png_batch, read_rgb_uint8, sample_cache_relpath,
                      write_cache_batch)

_FRAMES = ("left_rgb_path", "right_rgb_path", "disparity_path")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Build a resized FoundationStereo cache for faster training I/O.")
    p.add_argument("--dataset-root", type=str, default="/home/geoffrey/Reference/OffTopic/Datasets/FoundationStereo",
                   help="Path to raw FoundationStereo dataset root.")
    p.add_argument("--cache-root", type=str, required=True, help="Path to write cache files (prefer SSD).")
    p.add_argument("--height", type=int, default=240, help="Cached image height.")
    p.add_argument("--width", type=int, default=320, help="Cached image width.")
    p.add_argument("--max-samples", type=int, default=0, help="Optional cap on number of samples.")
    p.add_argument("--overwrite", action="store_true", help="Overwrite existing cache entries.")
    p.add_argument("--compress", action="store_true", help="Deflate the entries (smaller files, slower build/read).")
    p.add_argument("--batch-size", type=int, default=64, help="Samples per device batch.")
    p.add_argument("--read-threads", type=int, default=16, help="Host threads of the PNG reader and of the writer.")
    p.add_argument("--device", type=str, default="cuda")
    return p


def _resolve_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"--device {device}: the cache builder runs only on a HIP device (no CPU path).")
    return dev


def plan_batches(samples, batch_size: int) -> list[tuple[tuple[int, int] | None, list]]:
    """(source size, samples) batches: samples grouped by the size in their left frame's PNG header (None: not a PNG
    the native reader takes; those go through PIL), groups in order of first occurrence, cut into batch_size pieces."""
    by_size: dict = {}
    for s in samples:
        by_size.setdefault(png_size(s.left_rgb_path), []).append(s)
    return [(hw, group[i:i + batch_size]) for hw, group in by_size.items() for i in range(0, len(group), batch_size)]


class CachePipeline:
    """The three stages of a build over two sets of buffers (slots). ``decode`` fills a slot's pinned source frames,
    ``resize`` queues H2D copies, ``sd_stereo_to_cache`` and the D2H copies of the cache's 8 bytes per pixel on a side
    stream and returns their event, ``write`` waits for that event and writes the files. A slot's source frames may be
    refilled once its event has completed, its outputs once its write has returned; :func:`build_cache` keeps to that."""

    def __init__(self, image_size: tuple[int, int], batch_size: int, device: torch.device, compress: bool = False,
                 read_threads: int = 16):
        L.load()
        self.H, self.W = image_size
        self.bmax, self.device, self.compress, self.threads = batch_size, device, compress, read_threads
        self.stream = torch.cuda.Stream(device)
        self._src = [None, None]  # per slot: (source size, three pinned uint8 [bmax,Hs,Ws,3])
        H, W = image_size
        self._out = [(torch.empty(batch_size, H, W, 3, dtype=torch.uint8).pin_memory(),
                      torch.empty(batch_size, H, W, 3, dtype=torch.uint8).pin_memory(),
                      torch.empty(batch_size, H, W, dtype=torch.int16).pin_memory()) for _ in range(2)]

    def _pinned_src(self, slot: int, hw: tuple[int, int]):
        if self._src[slot] is None or self._src[slot][0] != hw:
            self._src[slot] = (hw, tuple(torch.empty(self.bmax, *hw, 3, dtype=torch.uint8).pin_memory()
                                         for _ in range(3)))
        return self._src[slot][1]

    def decode(self, slot: int, hw, samples) -> list[tuple]:
        """Source frames of one batch as parts (left, right, disparity RGB24), each uint8 [n,Hs,Ws,3] pinned and of one
        source size, in the batch's order."""
        n = len(samples)
        if hw is not None:
            views = tuple(t[:n] for t in self._pinned_src(slot, hw))
            if all(read_png_batch([getattr(s, a) for s in samples], hw, v, self.threads) for a, v in zip(_FRAMES, views)):
                return [views]
        # PIL for these frames (JPEG, other PNG kinds, or sizes that differ from the left frame's)
        parts, run, run_shape = [], [], None
        for s in samples:
            f = [read_rgb_uint8(getattr(s, a)) for a in _FRAMES]
            if not (f[0].shape == f[1].shape == f[2].shape):
                raise ValueError(f"left/right/disparity sizes differ for sample {s.disparity_path}")
            if run and f[0].shape != run_shape:
                parts.append(run)
                run = []
            run_shape = f[0].shape
            run.append(f)
        parts.append(run)
        return [tuple(torch.from_numpy(np.stack([f[a] for f in run])).pin_memory() for a in range(3)) for run in parts]

    def resize(self, slot: int, parts) -> torch.cuda.Event:
        H, W, dev = self.H, self.W, self.device
        out = self._out[slot]
        with torch.cuda.stream(self.stream):
            off = 0
            for left, right, disp in parts:
                n, Hs, Ws = left.shape[:3]
                ld, rd, dd = (t.to(dev, non_blocking=True) for t in (left, right, disp))
                ol = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
                orr = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
                od = torch.empty(n, H, W, dtype=torch.int16, device=dev)
                L.call("sd_stereo_to_cache", ld.data_ptr(), rd.data_ptr(), dd.data_ptr(), n, Hs, Ws, H, W,
                       ol.data_ptr(), orr.data_ptr(), od.data_ptr(), L.stream_handle(dev))
                for host, t in zip(out, (ol, orr, od)):
                    host[off:off + n].copy_(t, non_blocking=True)
                off += n
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return ev

    def write(self, slot: int, paths, ev: torch.cuda.Event) -> None:
        ev.synchronize()
        n = len(paths)
        left, right, disp = (t[:n] for t in self._out[slot])
        write_cache_batch(paths, (self.H, self.W), left, right, disp, self.compress, self.threads)


def build_cache(dataset_root, cache_root, height: int = 240, width: int = 320, max_samples: int = 0,
                overwrite: bool = False, compress: bool = False, batch_size: int = 64, read_threads: int = 16,
                device="cuda") -> dict:
    """Reference ``cache.py:50-112``: writes the missing (or, with overwrite, all) cache entries of the samples under
    dataset_root and ``cache_meta.json``; returns the metadata dict."""
    dev = _resolve_device(device)
    if batch_size < 1:
        raise ValueError(f"--batch-size must be >= 1, got: {batch_size}")
    dataset_root = Path(dataset_root).expanduser().resolve()
    cache_root = Path(cache_root).expanduser().resolve()
    cache_root.mkdir(parents=True, exist_ok=True)

    samples = discover_samples(dataset_root)
    if max_samples > 0:
        samples = samples[:max_samples]
    if not samples:
        raise ValueError(f"No samples discovered under: {dataset_root}")

    started_at = time.time()
    todo = []
    for s in samples:
        cache_file = cache_root / sample_cache_relpath(s)
        if cache_file.exists() and not overwrite:  # not validated, as in the reference
            continue
        cache_file.parent.mkdir(parents=True, exist_ok=True)
        todo.append(s)
    skipped = len(samples) - len(todo)

    if todo:
        batches = plan_batches(todo, batch_size)
        pipe = CachePipeline((height, width), batch_size, dev, compress, read_threads)
        events, writes, held = [None, None], [None, None], [None, None]
        try:
            with ThreadPoolExecutor(1) as reader, ThreadPoolExecutor(1) as writer:
                fut = reader.submit(pipe.decode, 0, *batches[0])
                for i, (_, sm) in enumerate(batches):
                    k = i & 1
                    parts = fut.result()
                    if i + 1 < len(batches):
                        if events[k ^ 1] is not None:
                            events[k ^ 1].synchronize()  # the other slot's source frames are on the device
                        fut = reader.submit(pipe.decode, k ^ 1, *batches[i + 1])
                    if writes[k] is not None:
                        writes[k].result()  # this slot's outputs are on disk
                    events[k] = pipe.resize(k, parts)
                    held[k] = parts  # pinned frames stay alive until their copies are done (the slot's next turn)
                    paths = [cache_root / sample_cache_relpath(s) for s in sm]
                    writes[k] = writer.submit(pipe.write, k, paths, events[k])
                for w in writes:
                    if w is not None:
                        w.result()
        finally:
            pipe.stream.synchronize()

    elapsed_sec = time.time() - started_at
    metadata = {
        "format_version": 1,
        "dataset_root": str(dataset_root),
        "cache_root": str(cache_root),
        "height": height,
        "width": width,
        "num_samples_total": len(samples),
        "num_written": len(todo),
        "num_skipped": skipped,
        "compressed": bool(compress),
        "elapsed_seconds": elapsed_sec,
        "created_at_unix": time.time(),
    }
    (cache_root / "cache_meta.json").write_text(json.dumps(metadata, indent=2), encoding="utf-8")
    print(f"Cache build complete: total={len(samples)} written={len(todo)} skipped={skipped} elapsed={elapsed_sec:.1f}s")
    print(f"Metadata: {cache_root / 'cache_meta.json'}")
    return metadata


def main(argv=None) -> dict:
    a = build_parser().parse_args(argv)
    return build_cache(a.dataset_root, a.cache_root, height=a.height, width=a.width, max_samples=a.max_samples,
                       overwrite=a.overwrite, compress=a.compress, batch_size=a.batch_size,
                       read_threads=a.read_threads, device=a.device)


if __name__ == "__main__":
    main()
