#!/usr/bin/env python3
"""Time the point-cloud stage on the GPU (sd_cloud_build_n through cloud.PointCloudBuilder) against the same work
written in torch on the device: fp64 reprojection of every pixel, the keep predicate, then ``xyz[keep]`` and
``color[keep]`` per stream (boolean-mask indexing: a host synchronisation and an allocation per stream).

Cases: 640x480 with n = 1 and n = 8, 1920x1080 with n = 1; stride 1, z_range (0.3, 10) m, coloured points, disparities
from StereoSGM on a synthetic shifted-texture pair (each stream its own pair). Per case: ms per call by HIP events over
back-to-back calls (the torch form by wall clock too, since it synchronises), the kept points, and the bytes the stage
must move: per pixel 4 (disp) read by the count pass, 4 again by the scatter pass, and per kept point 3 colour bytes
read and 16 bytes written, over the time: the achieved GB/s. The same calls captured into a HIP graph and replayed give
the device's time without the host's enqueue between launches. Whether a case is launch-bound or bandwidth-bound is
judged by those figures against the HBM rate; every call re-reads the same buffers, which fit the 256 MB Infinity Cache.

    python tools/cloud_bench.py --json profiles/cloud_bench.json
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stereo_depth_estimation_amd import _lib as L  # noqa: E402
from stereo_depth_estimation_amd import cloud, sgm  # noqa: E402

CASES = ((480, 640, 1), (480, 640, 8), (1080, 1920, 1))
Z_RANGE = (0.3, 10.0)


def _events(fn, iters: int, warmup: int) -> tuple[float, float]:
    """(ms per call by HIP events, ms per call by wall clock) of fn(), whose work ends on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters


def _graph_ms(fn, iters: int, per_graph: int = 20) -> float:
    """ms per call with per_graph calls captured into one HIP graph and replayed: the device's own time for the
    launches of a call, without the host's enqueue between them."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    replays = max(iters // per_graph, 5)
    ms, _ = _events(g.replay, replays, 3)
    return ms / per_graph


def scene(H: int, W: int, n: int, dev):
    """n synthetic pairs: a random texture, the right frame shifted by 24 + 4 i px with noise; BGR left frames and the
    matcher's disparities (float32, NaN where it found none)."""
    rng = np.random.default_rng(0)
    lefts, gl, gr = [], [], []
    for i in range(n):
        left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        right = np.roll(left, -(24 + 4 * i), axis=1)
        right = np.clip(right.astype(np.int16) + rng.integers(-6, 7, right.shape), 0, 255).astype(np.uint8)
        lefts.append(left)
        for frame, out in ((left, gl), (right, gr)):
            c = frame.astype(np.int32)
            out.append(((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8))
    q = sgm.StereoSGM(num_disparities=128, block_size=7).compute_batch(torch.as_tensor(np.stack(gl)).to(dev),
                                                                      torch.as_tensor(np.stack(gr)).to(dev))
    disp = torch.where(q > 0, q.float() / 16.0, torch.full((), float("nan"), device=dev))
    return disp.contiguous(), torch.as_tensor(np.stack(lefts)).to(dev)


def torch_cloud(disp, color, Qd, z_range):
    """The baseline: the stage's arithmetic in torch ops (fp64, one op per rounding), then boolean-mask indexing."""
    n, H, W = disp.shape
    y, x = torch.meshgrid(torch.arange(H, device=disp.device, dtype=torch.float64),
                          torch.arange(W, device=disp.device, dtype=torch.float64), indexing="ij")
    out = []
    for i in range(n):
        Q = Qd[i]
        has = torch.isfinite(disp[i]) & (disp[i] > 0)
        d = torch.where(has, disp[i], torch.ones((), device=disp.device)).double()
        R = [((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] for r in range(4)]
        xyz = torch.stack([(R[k] / R[3]).float() for k in range(3)], dim=-1)
        keep = has & torch.isfinite(xyz).all(dim=-1) & (xyz[..., 2] >= z_range[0]) & (xyz[..., 2] <= z_range[1])
        out.append((xyz[keep], color[i][keep].flip(-1)))  # the sync and the allocations
    return out


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--json", type=str, default=None, help="Write the results here.")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("cloud_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    L.load()
    f, B = 520.0, 0.12
    rows = []
    for H, W, n in CASES:
        disp, color = scene(H, W, n, dev)
        Q = cloud.pinhole_Q(f * W / 640.0, B, (W - 1) / 2, (H - 1) / 2)
        builder = cloud.PointCloudBuilder(n, dev)
        res = builder.build(disp, Q, color=color, z_range=Z_RANGE)
        counts = res.counts()
        Qd = torch.as_tensor(np.stack([Q] * n)).to(dev)
        base = torch_cloud(disp, color, Qd, Z_RANGE)
        # the two forms are timed as the same work only if they keep the same points: recorded, not assumed
        same_counts = [int(c) for c in counts] == [int(p.shape[0]) for p, _ in base]
        r0 = res.numpy(0)
        same_xyz = same_counts and np.array_equal(np.stack([r0["x"], r0["y"], r0["z"]], axis=-1), base[0][0].cpu().numpy())
        ms, wall = _events(lambda: builder.build(disp, Q, color=color, z_range=Z_RANGE), a.iters, a.warmup)
        ms_graph = _graph_ms(lambda: builder.build(disp, Q, color=color, z_range=Z_RANGE), a.iters)
        ms_xyz, _ = _events(lambda: builder.build(disp, Q, color=color, z_range=Z_RANGE, organized=True), a.iters,
                            a.warmup)
        t_ms, t_wall = _events(lambda: torch_cloud(disp, color, Qd, Z_RANGE), max(a.iters // 10, 5), 3)
        kept = int(counts.sum())
        moved = n * H * W * 8 + kept * 19
        rows.append({"H": H, "W": W, "streams": n, "stride": 1, "z_range": list(Z_RANGE), "pixels": n * H * W,
                     "points": kept, "ms_per_call": ms, "ms_per_call_wall": wall, "ms_per_call_with_xyz": ms_xyz,
                     "ms_per_call_graph_replay": ms_graph, "bytes_moved": moved,
                     "achieved_GBps": moved / (ms * 1e-3) / 1e9, "achieved_GBps_graph_replay": moved / (ms_graph * 1e-3) / 1e9,
                     "torch_ms_per_call": t_ms, "torch_ms_per_call_wall": t_wall, "speedup_vs_torch": t_wall / ms,
                     "torch_keeps_the_same_points": same_counts, "torch_gives_the_same_xyz": bool(same_xyz)})
        print(json.dumps(rows[-1]))
    out = {"tool": "tools/cloud_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "warmup": a.warmup, "cases": rows}
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
