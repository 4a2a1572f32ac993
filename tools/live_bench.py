#!/usr/bin/env python3
"""Time the live loop's frame path on the GPU: ms per frame, by HIP events and by wall clock, after warm-up.

  (i)  device : LiveDepth.step + readout (uint8 frames in, uint8 images and three scalars out)
  (ii) host   : the same frame served as before the device path existed: the numpy front end of the test oracle
                (tests/live_ref.py: remap, resize, /255), the fp32 upload from pageable memory,
                model(x, return_uncertainty=True), two .cpu() copies, the numpy post stage of the oracle.
                Its stages are also timed one by one (wall clock). The oracle's numpy is float64 and not tuned; an
                application with cv2 spends less in the two numpy stages, so read them as an upper bound and the
                upload / forward / read-back lines as they are.
  stages      : each new C-ABI stage alone, GPU time per call by HIP events over back-to-back launches, next to the
                forward it wraps (model(x) on a device tensor, events).

    python tools/live_bench.py --frames 640x480 --models 320x240,960x720 --precisions fp8,bf16 --json out.json

With --streams 1,2,4,8 it times several camera pairs per step instead (see bench_streams): LiveDepthBatch against N
LiveDepth objects stepped in turn, and the batched stages, with the shader clock probed before and after each row.
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
sys.path.insert(0, str(ROOT / "tests"))

import live_ref as R  # noqa: E402
from stereo_depth_estimation_amd import _lib as L  # noqa: E402
from stereo_depth_estimation_amd import live  # noqa: E402
from stereo_depth_estimation_amd.model import StereoUNet  # noqa: E402


def _size(s: str) -> tuple[int, int]:
    w, h = s.lower().split("x")
    return int(w), int(h)


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


def _wall(fn, iters: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _scene(rng, wc: int, hc: int):
    """A smooth synthetic stereo pair (uint8 BGR) and mildly distorted rectification maps."""
    y, x = np.mgrid[0:hc, 0:wc]
    base = 127 + 80 * np.sin(x / 23.0) * np.cos(y / 17.0)
    frames = []
    for shift in (0, 9):
        img = np.stack([np.roll(base, shift + 3 * c, axis=1) for c in range(3)], axis=-1)
        frames.append(np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8))
    K = np.array([[0.8 * wc, 0, wc / 2.0], [0, 0.8 * wc, hc / 2.0], [0, 0, 1]])
    P1 = np.hstack([K, np.zeros((3, 1))])
    P2 = P1.copy()
    P2[0, 3] = -0.8 * wc * 0.12
    dist = np.array([-0.12, 0.03, 0.001, -0.001, 0.0])
    ml = live.rectify_maps(K, dist, np.eye(3), P1, (wc, hc))
    mr = live.rectify_maps(K, -dist, np.eye(3), P2, (wc, hc))
    rect = live.Rectification(ml[0], ml[1], mr[0], mr[1], (wc, hc), float(P1[0, 0]), live.estimate_baseline_m(P1, P2))
    return frames, rect


def bench_one(precision: str, wm: int, hm: int, wc: int, hc: int, iters: int, warmup: int, host_iters: int) -> dict:
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    (fl, fr), rect = _scene(rng, wc, hc)
    torch.manual_seed(0)
    model = StereoUNet(base_channels=32, precision=precision).to(dev).eval()
    ld = live.LiveDepth(model, (wm, hm), rectification=rect)
    out = {"precision": precision, "model": f"{wm}x{hm}", "frames": f"{wc}x{hc}"}
    with torch.inference_mode():
        # ---- (i) the device path
        def device_frame():
            ld.step(fl, fr).readout()

        ev, wall = _events(device_frame, iters, warmup)
        out["device_ms_events"], out["device_ms_wall"] = ev, wall

        # ---- the forward alone, and each new stage alone (GPU time, events)
        x = torch.rand(1, 6, hm, wm, device=dev)
        out["forward_ms_events"] = _events(lambda: model(x, return_uncertainty=True), iters, warmup)[0]
        b, s = ld._batch._buf, L.stream_handle(dev)  # [1] of every buffer: stream 0's slice starts at the base pointer
        eng = model.engine()
        fld, frd = b["frames"][0], b["frames"][1]
        maps = [b[k].data_ptr() for k in ("m1l", "m2l", "m1r", "m2r")]
        xin = eng.ws.t["xin"].data_ptr()
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        fb = f32(ld.focal_length_px_model * ld.baseline_m)
        stages = {
            "frontend": lambda: L.call("sd_live_frontend", eng.sd_dtype, fld.data_ptr(), frd.data_ptr(), hc, wc, *maps,
                                       hm, wm, xin, None, None, 0, -1, s),
            "rectify_view": lambda: L.call("sd_live_rectify", fld.data_ptr(), hc, wc, maps[0], maps[1],
                                           b["view"].data_ptr(), s),
            "post": lambda: L.call("sd_live_post", b["disp"].data_ptr(), b["logvar"].data_ptr(), hm, wm,
                                   b["state"].data_ptr(), 1, 0.0, 1.0, 1, fb, b["depth"].data_ptr(),
                                   b["conf"].data_ptr(), b["dcode"].data_ptr(), 0.0, 10.0, b["ccode"].data_ptr(), 0.0,
                                   5.0, s),
            "contours": lambda: L.call("sd_live_contours", b["depth"].data_ptr(), hm, wm, 0.0, 10.0, 0.5,
                                       b["edge"].data_ptr(), s),
            "select_auto_range": lambda: L.call("sd_live_select", b["state"].data_ptr(), hm, wm,
                                                b["sel_ws"].data_ptr(), b["sel"].data_ptr(), b["ccode"].data_ptr(), s),
            "center": lambda: L.call("sd_live_center", b["state"].data_ptr(), b["depth"].data_ptr(),
                                     b["conf"].data_ptr(), hm, wm, ld.center_window, b["center"].data_ptr(), s),
            "compose": lambda: L.call("sd_live_compose", b["dcode"].data_ptr(), b["lut_a"].data_ptr(),
                                      b["depth_vis"].data_ptr(), b["ccode"].data_ptr(), b["lut_b"].data_ptr(),
                                      b["conf_vis"].data_ptr(), b["edge"].data_ptr(), b["view"].data_ptr(),
                                      b["left_view"].data_ptr(), hm, wm, hc, wc, s),
        }
        out["stage_us"] = {k: 1e3 * _events(fn, 4 * iters, warmup)[0] for k, fn in stages.items()}
        used = ("frontend", "rectify_view", "post", "contours", "center", "compose")  # the depth-enabled frame
        out["stages_ms_sum"] = sum(out["stage_us"][k] for k in used) / 1e3

        # ---- (ii) the host path, whole and stage by stage
        lut_a, lut_b = live.colormap_lut("turbo"), live.colormap_lut("viridis")
        maps_l, maps_r = (rect.map_l_1, rect.map_l_2), (rect.map_r_1, rect.map_r_2)
        focal, base = float(ld.focal_length_px_model), float(ld.baseline_m)
        keep = {}

        def h_front():
            keep["x"] = torch.from_numpy(R.front_end(fl, fr, maps_l, maps_r, hm, wm).astype(np.float32)).unsqueeze(0)
            keep["view"] = R.view_u8(fl, *maps_l)

        def h_upload():
            keep["xd"] = keep["x"].to(dev)

        def h_forward():
            keep["d"], keep["lv"] = model(keep["xd"], return_uncertainty=True)

        def h_readback():
            keep["dn"] = keep["d"][0, 0].cpu().numpy().astype(np.float32)
            keep["ln"] = keep["lv"][0, 0].cpu().numpy().astype(np.float32)

        def h_post():
            R.host_post(keep["dn"], keep["ln"], keep["view"], lut_a, lut_b, focal, base)

        def host_frame():
            for f in (h_front, h_upload, h_forward, h_readback, h_post):
                f()

        out["host_ms_wall"] = _wall(host_frame, host_iters, 2)
        out["host_stage_ms_wall"] = {f.__name__[2:]: _wall(f, host_iters, 1)
                                     for f in (h_front, h_upload, h_forward, h_readback, h_post)}
    return out


def clock_probe(dev, iters: int = 20000) -> float:
    """Median effective shader clock in MHz under sd_clock_probe's MFMA load (as bench.py reports it)."""
    n = 256
    out = torch.zeros(4 * n, dtype=torch.int64, device=dev)
    sink = torch.zeros(256, dtype=torch.float32, device=dev)
    L.call("sd_clock_probe", n, iters, out.data_ptr(), sink.data_ptr(), L.stream_handle(dev))
    torch.cuda.synchronize(dev)
    o = out.view(n, 4).cpu().double()
    mhz = ((o[:, 1] - o[:, 0]) / (o[:, 3] - o[:, 2]) * 100.0).sort().values
    return round(float(mhz[n // 2]), 1)


def bench_streams(precision: str, wm: int, hm: int, wc: int, hc: int, iters: int, warmup: int, n: int) -> dict:
    """n camera pairs per step, on one model:
      (a) batch : LiveDepthBatch.step + readout (one front end, one batch-n forward, one display stage, one read-out)
      (b) loop  : n LiveDepth objects sharing the model, each stepped and read out in turn (n batch-1 forwards, n display
                  stages, n syncing read-outs): what a host with n rigs could do before the batch existed
      (c) stages: GPU time of the batched stages around the forward for n streams, each alone by events over
                  back-to-back launches, and their sum for the depth-enabled frame
    (a) and (b) are timed twice each, alternating, with the shader clock probed before and after."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    (fl, fr), rect = _scene(rng, wc, hc)
    fls = np.stack([np.roll(fl, 5 * i, axis=1) for i in range(n)])  # every rig sees its own frames
    frs = np.stack([np.roll(fr, 5 * i, axis=1) for i in range(n)])
    torch.manual_seed(0)
    model = StereoUNet(base_channels=32, precision=precision).to(dev).eval()
    out = {"precision": precision, "model": f"{wm}x{hm}", "frames": f"{wc}x{hc}", "streams": n,
           "clock_mhz_before": clock_probe(dev)}
    with torch.inference_mode():
        ldb = live.LiveDepthBatch(model, n, (wm, hm), rectification=rect)
        lds = [live.LiveDepth(model, (wm, hm), rectification=rect) for _ in range(n)]

        def batch_step():
            ldb.step(fls, frs).readout()

        def loop_step():
            for i, ld in enumerate(lds):
                ld.step(fls[i], frs[i]).readout()

        runs = {"batch": [], "loop": []}
        for _ in range(2):  # alternating: the engine's workspace and graph follow the batch size, so each run warms up
            for name, fn in (("batch", batch_step), ("loop", loop_step)):
                runs[name].append(_events(fn, iters, warmup))
        for name in runs:
            ev, wall = min(runs[name])
            out[f"{name}_ms_events"], out[f"{name}_ms_wall"] = ev, wall
            out[f"{name}_ms_events_runs"] = [r[0] for r in runs[name]]
            out[f"{name}_frames_per_s"] = n / (wall * 1e-3)
        batch_step()  # the engine's workspace is the batch's again
        x = torch.rand(n, 6, hm, wm, device=dev)
        out["forward_ms_events"] = _events(lambda: model(x, return_uncertainty=True), iters, warmup)[0]
        batch_step()
        b, s, eng = ldb._buf, L.stream_handle(dev), model.engine()
        fld, frd = b["frames"][0], b["frames"][1]
        maps = [b[k].data_ptr() for k in ("m1l", "m2l", "m1r", "m2r")]
        xin = eng.ws.t["xin"].data_ptr()
        p = {k: v.data_ptr() for k, v in b.items() if isinstance(v, torch.Tensor)}
        stages = {
            "frontend": lambda: L.call("sd_live_frontend_n", n, eng.sd_dtype, fld.data_ptr(), frd.data_ptr(), hc, wc, *maps,
                                       0, hm, wm, xin, None, None, 0, -1, s),
            "rectify_view": lambda: L.call("sd_live_rectify_n", n, fld.data_ptr(), hc, wc, maps[0], maps[1], 0, p["view"],
                                           s),
            "post": lambda: L.call("sd_live_post_n", n, p["disp"], p["logvar"], hm, wm, p["state"], (1 << n) - 1, 0, 0.0,
                                   1.0, 1, p["fb"], p["depth"], p["conf"], p["dcode"], 0.0, 10.0, p["ccode"], 0.0, 5.0, s),
            "contours": lambda: L.call("sd_live_contours_n", n, p["depth"], hm, wm, 0.0, 10.0, 0.5, p["edge"], 0, s),
            "select_auto_range": lambda: L.call("sd_live_select_n", n, p["state"], hm, wm, p["sel_ws"], p["sel"],
                                                p["ccode"], 0, s),
            "center": lambda: L.call("sd_live_center_n", n, p["state"], p["depth"], p["conf"], hm, wm,
                                     ldb.center_window, p["center"], 0, s),
            "compose": lambda: L.call("sd_live_compose_n", n, p["dcode"], p["lut_a"], p["depth_vis"], p["ccode"],
                                      p["lut_b"], p["conf_vis"], p["edge"], p["view"], p["left_view"], hm, wm, hc, wc, 0, s),
        }
        out["stage_us"] = {k: 1e3 * _events(fn, 4 * iters, warmup)[0] for k, fn in stages.items()}
        used = ("frontend", "rectify_view", "post", "contours", "center", "compose")  # the depth-enabled frame
        out["stages_ms_sum"] = sum(out["stage_us"][k] for k in used) / 1e3
    out["clock_mhz_after"] = clock_probe(dev)
    return out


def main_streams(args, wc: int, hc: int) -> None:
    rows = []
    for precision in args.precisions.split(","):
        for m in args.models.split(","):
            wm, hm = _size(m)
            for n in (int(v) for v in args.streams.split(",")):
                row = bench_streams(precision, wm, hm, wc, hc, args.iters, args.warmup, n)
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("\n| precision | model | N | batch ms/step (events / wall) | batch frames/s | N x LiveDepth ms/step (events / "
          "wall) | loop frames/s | batch-N forward ms | batched stages ms | clock MHz |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['precision']} | {r['model']} | {r['streams']} | {r['batch_ms_events']:.3f} / {r['batch_ms_wall']:.3f} | "
              f"{r['batch_frames_per_s']:.0f} | {r['loop_ms_events']:.3f} / {r['loop_ms_wall']:.3f} | "
              f"{r['loop_frames_per_s']:.0f} | {r['forward_ms_events']:.3f} | {r['stages_ms_sum']:.3f} | "
              f"{r['clock_mhz_before']:.0f} / {r['clock_mhz_after']:.0f} |")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(rows, indent=1))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="640x480")
    ap.add_argument("--models", default="320x240,960x720")
    ap.add_argument("--precisions", default="fp8,bf16")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--json", type=Path, default=None)
    ap.add_argument("--streams", default=None, metavar="N,N,...",
                    help="e.g. 1,2,4,8: time LiveDepthBatch with N camera pairs per step against N LiveDepth objects "
                         "stepped in turn, and the batched stages (instead of the single-stream report)")
    args = ap.parse_args()
    if args.streams and not all(1 <= int(v) <= live.MAX_STREAMS for v in args.streams.split(",")):
        raise SystemExit(f"--streams: counts in 1..{live.MAX_STREAMS}")
    if not torch.cuda.is_available():
        raise SystemExit("live_bench needs a HIP device: there is no CPU fallback and no CPU timing")
    wc, hc = _size(args.frames)
    if args.streams:
        return main_streams(args, wc, hc)
    rows = []
    for precision in args.precisions.split(","):
        for m in args.models.split(","):
            wm, hm = _size(m)
            row = bench_one(precision, wm, hm, wc, hc, args.iters, args.warmup, args.host_iters)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n| precision | model | device path ms (events / wall) | forward ms | new stages ms | host path ms (wall) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['precision']} | {r['model']} | {r['device_ms_events']:.3f} / {r['device_ms_wall']:.3f} | "
              f"{r['forward_ms_events']:.3f} | {r['stages_ms_sum']:.3f} | {r['host_ms_wall']:.1f} |")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
