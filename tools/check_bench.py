#!/usr/bin/env python3
"""Time the label-free check on the GPU (sd_stereo_check through check.StereoCheck, all five outputs) against the same
work written in torch on the device: ``flip`` / ``cummin`` / ``flip`` for the suffix minimum, ``gather`` for the warp,
``where`` chains for the classes and masked sums for the rows; one op per rounding, no host synchronisation.

Cases: 640x480 with n = 1 and n = 8, 960x540 with n = 32; occ_tol 0.5, photo_thr 250. Disparities are piecewise constant
per row (runs of 8 pixels, 1..64 px) with 5 % NaN, frames are random: every class occurs, and the time of neither form
depends on the values. Both forms are timed in the same process in alternating rounds (HIP events over back-to-back
calls, after a warm-up at the shape); the figures are the median round and the spread over the rounds. The stage is
also captured into a HIP graph and replayed: the device's time without the host's enqueue. The bytes the stage must move
are 4 (disp) + 3 (left) + 3 (right, gathered) read and 1 + 4 + 4 + 3 written per pixel, over the time: the achieved
GB/s; every call re-reads the same buffers, which fit the 256 MB Infinity Cache up to n = 8. Whether the two forms
compute the same classes and residuals is recorded, not assumed.

    python tools/check_bench.py --json profiles/check_bench.json
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stereo_depth_estimation_amd import _lib as L  # noqa: E402
from stereo_depth_estimation_amd import check  # noqa: E402

CASES = ((480, 640, 1), (480, 640, 8), (540, 960, 32))
OCC_TOL, PHOTO_THR = 0.5, 250.0
BYTES_PER_PIXEL = 4 + 3 + 3 + 1 + 4 + 4 + 3


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
    """ms per call with per_graph calls captured into one HIP graph and replayed."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    ms, _ = _events(g.replay, max(iters // per_graph, 5), 3)
    return ms / per_graph


def scene(H: int, W: int, n: int, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    runs = torch.rand(n, H, (W + 7) // 8, device=dev, generator=gen) * 63 + 1
    disp = runs.repeat_interleave(8, dim=2)[:, :, :W].contiguous()
    disp = disp + (torch.rand(n, H, W, device=dev, generator=gen) - 0.5) * 0.4
    disp[torch.rand(n, H, W, device=dev, generator=gen) < 0.05] = float("nan")
    left = torch.randint(0, 256, (n, H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    right = torch.randint(0, 256, (n, H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    return disp, left, right


def torch_check(disp, left, right, tol: float, thr: float):
    """The baseline: the stage's arithmetic in torch ops (float32, one op per rounding). Returns cls, resid, disp_vis,
    vis_rgb, rows as the stage defines them."""
    n, H, W = disp.shape
    dev = disp.device
    inf = torch.full((), float("inf"), device=dev)
    nan = torch.full((), float("nan"), device=dev)
    has = torch.isfinite(disp) & (disp > 0)
    xr = torch.arange(W, device=dev, dtype=torch.float32) - torch.where(has, disp, torch.zeros((), device=dev))
    oov = has & (xr < 0)
    incl = torch.where(has, xr, inf).flip(-1).cummin(-1).values.flip(-1)
    m = torch.cat([incl[..., 1:], inf.expand(n, H, 1)], dim=-1)
    occ = has & ~oov & ((m + tol) <= xr)
    vis = has & ~oov & ~occ
    xs = torch.where(vis, xr, torch.zeros((), device=dev))
    x0 = xs.floor().long().clamp(max=W - 1)
    f = xs - x0.float()
    x1 = (x0 + 1).clamp(max=W - 1)
    rf = right.float()
    a = torch.gather(rf, 2, x0[..., None].expand(-1, -1, -1, 3))
    b = torch.gather(rf, 2, x1[..., None].expand(-1, -1, -1, 3))
    r = a + f[..., None] * (b - a)
    ad = (left.float() - r).abs()
    e = (ad[..., 0] + ad[..., 1]) + ad[..., 2]
    mis = vis & (e > thr)
    u8 = lambda v: torch.full((), v, device=dev, dtype=torch.uint8)  # noqa: E731
    cls = torch.where(mis, u8(4), torch.where(vis, u8(0), torch.where(occ, u8(3), torch.where(oov, u8(2), u8(1)))))
    resid = torch.where(vis, e, nan)
    disp_vis = torch.where(vis & ~mis, disp, nan)
    # a device tensor as the divisor: by a Python scalar torch multiplies by the reciprocal, which rounds otherwise
    three = torch.full((), 3.0, device=dev)
    g = (torch.where(vis, e, torch.zeros((), device=dev)) / three).to(torch.int32).clamp(max=255).to(torch.uint8)
    colour = lambda c: torch.tensor(c, device=dev, dtype=torch.uint8)  # noqa: E731
    vis_rgb = g[..., None].expand(-1, -1, -1, 3)
    for mask, c in ((~has, (0, 0, 0)), (oov, (0, 0, 255)), (occ, (255, 0, 0)), (mis, (255, 255, 0))):
        vis_rgb = torch.where(mask[..., None], colour(c), vis_rgb)
    e64 = torch.where(vis, e, torch.zeros((), device=dev)).double()
    cnt = lambda t: t.sum(dim=(1, 2)).double()  # noqa: E731
    rows = torch.stack([cnt(has), cnt(oov), cnt(occ), cnt(vis), e64.sum(dim=(1, 2)), (e64 * e64).sum(dim=(1, 2)),
                        cnt(mis), torch.zeros(n, device=dev, dtype=torch.float64)], dim=1)
    return cls, resid, disp_vis, vis_rgb.contiguous(), rows


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=2000, help="Calls of the stage per round.")
    ap.add_argument("--torch-iters", type=int, default=100, help="Calls of the torch form per round.")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--json", type=str, default=None, help="Write the results here.")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("check_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    L.load()
    out_rows = []
    for H, W, n in CASES:
        disp, left, right = scene(H, W, n, dev)
        chk = check.StereoCheck(n, dev)
        stage = lambda: chk.run(disp, left, right, occ_tol=OCC_TOL, photo_thr=PHOTO_THR)  # noqa: E731
        base = lambda: torch_check(disp, left, right, OCC_TOL, PHOTO_THR)  # noqa: E731
        res, ref = stage(), base()
        torch.cuda.synchronize()
        same_cls = bool(torch.equal(res.cls, ref[0]))
        same_resid = bool(torch.equal(torch.nan_to_num(res.resid, nan=-1.0), torch.nan_to_num(ref[1], nan=-1.0)))
        same_rgb = bool(torch.equal(res.vis_rgb, ref[3]))
        same_counts = bool(torch.equal(res.rows[:, [0, 1, 2, 3, 6]], ref[4][:, [0, 1, 2, 3, 6]]))
        shares = (torch.bincount(res.cls.reshape(-1).long(), minlength=5).double() / res.cls.numel()).tolist()
        _events(stage, a.warmup, a.warmup)
        _events(base, 5, 5)
        ms_s, ms_t, wall_s = [], [], []
        for _ in range(a.rounds):  # alternating, in one process
            ms, wall = _events(stage, a.iters, 0)
            ms_s.append(ms)
            wall_s.append(wall)
            ms_t.append(_events(base, a.torch_iters, 0)[0])
        ms_graph = _graph_ms(stage, a.iters)
        ms_rows_only, _ = _events(lambda: chk.run(disp, left, right, occ_tol=OCC_TOL, photo_thr=PHOTO_THR,
                                                  want=("rows",)), a.iters, a.warmup)
        ms, t_ms = statistics.median(ms_s), statistics.median(ms_t)
        moved = n * H * W * BYTES_PER_PIXEL
        out_rows.append({"H": H, "W": W, "samples": n, "pixels": n * H * W, "occ_tol": OCC_TOL, "photo_thr": PHOTO_THR,
                         "class_shares": shares, "ms_per_call": ms, "ms_per_call_rounds": ms_s,
                         "ms_per_call_wall": statistics.median(wall_s), "ms_per_call_graph_replay": ms_graph,
                         "ms_per_call_rows_only": ms_rows_only, "bytes_moved": moved,
                         "achieved_GBps": moved / (ms * 1e-3) / 1e9,
                         "achieved_GBps_graph_replay": moved / (ms_graph * 1e-3) / 1e9,
                         "torch_ms_per_call": t_ms, "torch_ms_per_call_rounds": ms_t, "speedup_vs_torch": t_ms / ms,
                         "torch_gives_the_same_cls": same_cls, "torch_gives_the_same_resid": same_resid,
                         "torch_gives_the_same_vis_rgb": same_rgb, "torch_gives_the_same_counts": same_counts})
        print(json.dumps(out_rows[-1]))
    out = {"tool": "tools/check_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "torch_iters": a.torch_iters, "rounds": a.rounds, "warmup": a.warmup, "cases": out_rows}
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
