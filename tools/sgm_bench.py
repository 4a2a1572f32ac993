#!/usr/bin/env python3
"""Time the classical live loop's frame path on the GPU (ClassicDepth: rectify, gray, the semi-global matcher,
reprojection, centre distance, colour image): ms per frame by HIP events and by wall clock, after warm-up, and each
C-ABI stage alone, GPU time per call by HIP events over back-to-back launches (as tools/live_bench.py does).

The matcher's reference points are arithmetic, not measurements: the two uint16 volumes C and S are each
2 * H * W * D bytes. The three recurrences move seven of them (top-down reads C, writes S; left-right reads C and S,
writes S; right-left reads C and S), and each is one sequential chain of H or W - maxD steps per scan line; the cost
stage writes its row sums into S as scratch, reads them about twice and writes C. The table prints the volume bytes
over each stage's time next to the chain's time per step. --mode hh4 / sgbm / hh runs the frame with that mode's
further paths (each one launch that reads C and S and writes S: three volumes, H steps per chain) and times each of
them alone, with top -> down as an adding pass of the same kernel beside them.

--streams N times, in one session and at the same frame, parameters and protocol, ClassicDepthBatch(N) (N rigs through
one launch per stage) against N ClassicDepth objects (each a batch of one) stepped in turn, and the batch's entry
points alone (the matcher as one stage: its kernels have no batched entry points of their own; a kernel trace of this
tool splits it).

    python tools/sgm_bench.py --frames 640x480 --num-disparities 128 --block-size 7 --mode hh --json out.json
    python tools/sgm_bench.py --streams 8 --mode 3way
    python tools/sgm_bench.py --cost census --census-window 7x9

--cost census runs the frame with the census / Hamming pixel cost (StereoSGM(cost="census")): the stage table then
holds the two descriptor launches ("census (x2)") and the census cost stage in place of the two prefilter launches and
the Birchfield-Tomasi cost stage they replace.
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
from stereo_depth_estimation_amd import live, sgm  # noqa: E402


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


def _scene(rng, wc: int, hc: int):
    """A textured synthetic stereo pair (uint8 BGR) with a disparity ramp, mildly distorted rectification maps and Q."""
    base = rng.integers(0, 256, (hc, wc + 128, 3)).astype(np.float64)
    for _ in range(2):  # a little smoothing: texture with structure at the block size
        base = (base + np.roll(base, 1, axis=1) + np.roll(base, 1, axis=0)) / 3.0
    base = (base - base.min()) / (base.max() - base.min()) * 255.0
    left = base[:, 64:64 + wc]
    right = np.empty_like(left)
    for y in range(hc):  # right[x] = left[x + d], d from 8 at the top to 48 at the bottom
        d = 8 + (40 * y) // hc
        right[y] = base[y, 64 + d:64 + d + wc]
    frames = [np.clip(f + rng.normal(0, 3, f.shape), 0, 255).astype(np.uint8) for f in (left, right)]
    K = np.array([[0.8 * wc, 0, wc / 2.0], [0, 0.8 * wc, hc / 2.0], [0, 0, 1]])
    P1 = np.hstack([K, np.zeros((3, 1))])
    P2 = P1.copy()
    P2[0, 3] = -0.8 * wc * 0.12
    dist = np.array([-0.05, 0.01, 0.0005, -0.0005, 0.0])
    ml = live.rectify_maps(K, dist, np.eye(3), P1, (wc, hc))
    mr = live.rectify_maps(K, -dist, np.eye(3), P2, (wc, hc))
    rect = live.Rectification(ml[0], ml[1], mr[0], mr[1], (wc, hc), float(P1[0, 0]), 0.12)
    Q = np.array([[1, 0, 0, -wc / 2.0], [0, 1, 0, -hc / 2.0], [0, 0, 0, 0.8 * wc], [0, 0, 1 / 0.12, 0]])
    return frames, rect, Q


# the vertical-family paths a mode adds to the three of "3way", in the order sd_sgm_compute_mode launches them
EXTRA_PATHS = {"3way": (), "hh4": ((-1, 0),), "sgbm": ((1, 1), (1, -1)),
               "hh": ((1, 1), (1, -1), (-1, 0), (-1, 1), (-1, -1))}


def _cost_kw(cost: str, window) -> dict:
    """StereoSGM's two keywords; a window with cost "bt" is passed on, so that the constructor refuses it."""
    return {"cost": cost, **({} if window is None else {"census_window": window})}


def bench(wc: int, hc: int, D: int, bs: int, iters: int, warmup: int, mode: str = "3way", cost: str = "bt",
          window=None) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    (fl, fr), rect, Q = _scene(np.random.default_rng(0), wc, hc)
    cd = sgm.ClassicDepth(rectification=rect, Q=Q, num_disparities=D, block_size=bs, mode=mode, device=dev,
                          **_cost_kw(cost, window))
    out = {"frames": f"{wc}x{hc}", "num_disparities": D, "block_size": bs, "mode": mode, "cost": cost,
           "census_window": None if cost == "bt" else "%dx%d" % cd.matcher.census_window, "iters": iters,
           "warmup": warmup, "clock_mhz_before": clock_probe(dev)}

    def frame():
        cd.step(fl, fr).readout()

    out["frame_ms_events"], out["frame_ms_wall"] = _events(frame, iters, warmup)
    res = cd.step(fl, fr)
    torch.cuda.synchronize()
    q = res.disparity_q4
    out["valid_fraction"] = float((q[:, D:] != cd.matcher.invalid_value).float().mean())

    # each stage alone, back-to-back launches on the frame's own buffers ([1] of every buffer: stream 0's slice starts
    # at the base pointer), through the single-stream entry points
    b, m, s = cd._batch._buf, cd.matcher, L.stream_handle(dev)
    H, W, P = hc, wc, hc * wc
    vol = (2 * P * D + 255) // 256 * 256
    ws = m.workspace(dev, H, W)
    C, S = ws.data_ptr(), ws.data_ptr() + vol
    pl = ws.data_ptr() + 2 * vol
    pr = pl + (P + 255) // 256 * 256
    sw = pr + (P + 255) // 256 * 256
    dl = ws.data_ptr() + L.call("sd_sgm_ws_bytes", H, W, D)  # census: the descriptor planes follow the BT layout
    dr = dl + (8 * P + 255) // 256 * 256
    fld, frd = b["frames"][0][0], b["frames"][0][1]
    gl, gr = b["gray"][0], b["gray"][1]
    q_tmp = torch.empty_like(q)
    Q = np.ascontiguousarray(cd.Q)
    agg = (C, H, W, m.min_disparity, D, m.P1, m.P2)
    if cost == "census":
        wh, ww = m.census_window
        cost_stages = {
            "census (x2)": lambda: [L.call("sd_sgm_census_n", 1, g.data_ptr(), H, W, wh, ww, d, s)
                                    for g, d in ((gl, dl), (gr, dr))],
            "census cost": lambda: L.call("sd_sgm_cost_census", dl, dr, H, W, m.min_disparity, D, bs, m.nbits, C, S, s),
        }
    else:
        cost_stages = {
            "prefilter (x2)": lambda: [L.call("sd_sgm_prefilter", g.data_ptr(), H, W, m.pre_filter_cap, p, s)
                                       for g, p in ((gl, pl), (gr, pr))],
            "cost": lambda: L.call("sd_sgm_cost", gl.data_ptr(), gr.data_ptr(), pl, pr, H, W, m.min_disparity, D, bs, C, S,
                                   s),
        }
    stages = {
        "rectify (x2)": lambda: [L.call("sd_live_rectify", f.data_ptr(), H, W, b[f"m1{k}"].data_ptr(),
                                        b[f"m2{k}"].data_ptr(), b["rect"][i].data_ptr(), s)
                                 for i, (f, k) in enumerate(((fld, "l"), (frd, "r")))],
        "gray (x2)": lambda: [L.call("sd_sgm_gray", b["rect"][i].data_ptr(), H, W, b["gray"][i].data_ptr(), s)
                              for i in range(2)],
        **cost_stages,
        "aggregate top-down": lambda: L.call("sd_sgm_aggregate", *agg, 0, S, s),
        "aggregate right-left + winner": lambda: L.call("sd_sgm_winner", C, S, H, W, m.min_disparity, D, m.P1, m.P2,
                                                        m.uniqueness_ratio, m.disp12_max_diff, None, None,
                                                        q_tmp.data_ptr(), s),
        "aggregate left-right": lambda: L.call("sd_sgm_aggregate", *agg, 1, S, s),
        **{f"aggregate ({dy:+d}, {dx:+d}) adding": (lambda dy=dy, dx=dx: L.call("sd_sgm_aggregate_dir", *agg, dy, dx, 1, S, s))
           for dy, dx in (((1, 0),) + EXTRA_PATHS[mode] if mode != "3way" else ())},
        "speckle": lambda: (q_tmp.copy_(q), L.call("sd_sgm_speckle", q_tmp.data_ptr(), H, W, m.invalid_value,
                                                   m.speckle_window_size, m.speckle_range, sw, s)),
        "post": lambda: L.call("sd_sgm_post", q.data_ptr(), H, W, Q.ctypes.data, b["disp"].data_ptr(),
                               b["z"].data_ptr(), b["code"].data_ptr(), b["minmax"].data_ptr(), s),
        "center": lambda: L.call("sd_sgm_center", b["z"].data_ptr(), H, W, cd.center_window, b["center"].data_ptr(), s),
        "compose": lambda: L.call("sd_live_compose", b["code"].data_ptr(), b["lut"].data_ptr(), b["vis"].data_ptr(),
                                  None, None, None, None, None, None, H, W, H, W, s),
    }
    # the left-right pass and a mode's further paths add into S on every launch, so they are timed after the winner
    # kernel (which reads S)
    out["stage_us"] = {k: 1e3 * _events(fn, iters, warmup)[0] for k, fn in stages.items()}
    out["stages_ms_sum"] = sum(out["stage_us"].values()) / 1e3
    volume_bytes = 2 * P * D
    out["cost_stages_us"] = sum(out["stage_us"][k] for k in cost_stages)  # what the choice of pixel cost decides
    passes = {"census cost" if cost == "census" else "cost": 1, "aggregate top-down": 2, "aggregate left-right": 3, "aggregate right-left + winner": 2}
    extra = [k for k in stages if k.endswith("adding")]
    passes.update({k: 3 for k in extra})
    out["volume_bytes"] = volume_bytes
    out["volume_GBps"] = {k: n * volume_bytes / (out["stage_us"][k] * 1e-6) / 1e9 for k, n in passes.items()}
    maxD = m.min_disparity + D
    steps = {"aggregate top-down": H, "aggregate left-right": W - maxD, "aggregate right-left + winner": W - maxD}
    out["chain_ns_per_step"] = {k: out["stage_us"][k] * 1e3 / n for k, n in steps.items()}
    out["chain_ns_per_step"].update({k: out["stage_us"][k] * 1e3 / H for k in extra})
    # the frame's own aggregation: the three passes and the mode's further paths (not the adding top-down pass,
    # which is there for comparison only)
    own = list(steps) + [k for k in extra if not k.startswith("aggregate (+1, +0)")]
    agg_us = sum(out["stage_us"][k] for k in own)
    out["aggregate_ms"] = agg_us / 1e3
    out["aggregate_volume_GBps"] = sum(passes[k] for k in own) * volume_bytes / (agg_us * 1e-6) / 1e9
    out["clock_mhz_after"] = clock_probe(dev)
    return out


def bench_streams(wc: int, hc: int, D: int, bs: int, iters: int, warmup: int, mode: str, n: int,
                  batch_only: bool = False, cost: str = "bt", window=None) -> dict:
    """ClassicDepthBatch(n) against n ClassicDepth objects in turn: every stream has frames of its own, the maps and Q
    are shared. A frame of the batch is step + readout (one sync); the n single objects are timed both with a readout
    after every step (n syncs, what n independent loops do) and with all steps issued before the n readouts.
    batch_only leaves the single objects out, so that a kernel trace of the run holds the batch's launches alone."""
    dev = torch.device("cuda", torch.cuda.current_device())
    scenes = [_scene(np.random.default_rng(i), wc, hc) for i in range(n)]
    fl = np.stack([sc[0][0] for sc in scenes])
    fr = np.stack([sc[0][1] for sc in scenes])
    rect, Q = scenes[0][1], scenes[0][2]
    kw = dict(rectification=rect, Q=Q, num_disparities=D, block_size=bs, mode=mode, device=dev, **_cost_kw(cost, window))
    out = {"frames": f"{wc}x{hc}", "num_disparities": D, "block_size": bs, "mode": mode, "cost": cost,
           "census_window": None, "iters": iters, "warmup": warmup, "streams": n,
           "workspace_bytes": L.call("sd_sgm_ws_bytes_cost_n", n, hc, wc, D, sgm.COSTS[cost]),
           "clock_mhz_before": clock_probe(dev)}
    batch = sgm.ClassicDepthBatch(n, **kw)
    singles = [] if batch_only else [sgm.ClassicDepth(**kw) for _ in range(n)]

    def frame_batch():
        batch.step(fl, fr).readout()

    def frame_turn():
        for i, cd in enumerate(singles):
            cd.step(fl[i], fr[i]).readout()

    def frame_turn_late():
        res = [cd.step(fl[i], fr[i]) for i, cd in enumerate(singles)]
        for r in res:
            r.readout()

    paths = (("batch", frame_batch), ("in_turn", frame_turn), ("in_turn_late_readout", frame_turn_late))
    for key, fn in paths[:1] if batch_only else paths:
        ev, wall = _events(fn, iters, warmup)
        out[key] = {"step_ms_events": ev, "step_ms_wall": wall, "frames_per_s": n / (wall * 1e-3)}
    if not batch_only:
        out["speedup_wall"] = out["in_turn"]["step_ms_wall"] / out["batch"]["step_ms_wall"]
    res = batch.step(fl, fr)
    torch.cuda.synchronize()
    q = res.disparity_q4
    m = batch.matcher
    out["census_window"] = None if m.census_window is None else "%dx%d" % m.census_window
    out["valid_fraction"] = float((q[:, :, D:] != m.invalid_value).float().mean())
    if not batch_only:
        one = singles[0].step(fl[0], fr[0])
        torch.cuda.synchronize()
        out["stream0_equals_single"] = bool(torch.equal(q[0], one.disparity_q4))

    # the batch's entry points alone, back-to-back launches on the step's own buffers
    b, s = batch._buf, L.stream_handle(dev)
    H, W = hc, wc
    ws = m.workspace(dev, H, W, n)
    frames = b["frames"][0]
    q_tmp = torch.empty_like(q)
    sw = torch.empty(n * L.call("sd_sgm_speckle_ws_bytes", H, W), dtype=torch.uint8, device=dev)
    stages = {
        "rectify (x2)": lambda: [L.call("sd_live_rectify_n", n, frames[i].data_ptr(), H, W, b[f"m1{k}"].data_ptr(),
                                        b[f"m2{k}"].data_ptr(), 0, b["rect"][i].data_ptr(), s)
                                 for i, k in enumerate("lr")],
        "gray (x2)": lambda: [L.call("sd_sgm_gray", b["rect"][i].data_ptr(), n * H, W, b["gray"][i].data_ptr(), s)
                              for i in range(2)],
        "matcher": lambda: L.call("sd_sgm_compute_cost_n", n, b["gray"][0].data_ptr(), b["gray"][1].data_ptr(), H, W,
                                  *m.params(), m.mode_id, m.cost_id, *(m.census_window or (0, 0)), ws.data_ptr(),
                                  q_tmp.data_ptr(), s),
        "speckle alone": lambda: (q_tmp.copy_(q), L.call("sd_sgm_speckle_n", n, q_tmp.data_ptr(), H, W, m.invalid_value,
                                                         m.speckle_window_size, m.speckle_range, sw.data_ptr(), s)),
        "post": lambda: L.call("sd_sgm_post_n", n, q.data_ptr(), H, W, b["Q"].data_ptr(), b["disp"].data_ptr(),
                               b["z"].data_ptr(), b["code"].data_ptr(), b["minmax"].data_ptr(), s),
        "center": lambda: L.call("sd_sgm_center_n", n, b["z"].data_ptr(), H, W, batch.center_window,
                                 b["center"].data_ptr(), s),
        "compose": lambda: L.call("sd_live_compose_n", n, b["code"].data_ptr(), b["lut"].data_ptr(), b["vis"].data_ptr(),
                                  None, None, None, None, None, None, H, W, H, W, 0, s),
    }
    out["stage_us"] = {k: 1e3 * _events(fn, iters, warmup)[0] for k, fn in stages.items()}
    out["clock_mhz_after"] = clock_probe(dev)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="640x480")
    ap.add_argument("--num-disparities", type=int, default=128)
    ap.add_argument("--block-size", type=int, default=7)
    ap.add_argument("--mode", choices=sorted(sgm.MODES), default="3way")
    ap.add_argument("--cost", choices=sorted(sgm.COSTS), default="bt", help="pixel cost of the matcher")
    ap.add_argument("--census-window", default=None, help="HxW, rows x columns (default 7x9; with --cost census)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--streams", type=int, default=0,
                    help="N > 0: ClassicDepthBatch(N) against N ClassicDepth objects in turn")
    ap.add_argument("--batch-only", action="store_true", help="with --streams: leave the N single objects out")
    ap.add_argument("--json", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgm_bench needs a HIP device: there is no CPU fallback and no CPU timing")
    w, h = (int(v) for v in args.frames.lower().split("x"))
    if args.streams:
        r = bench_streams(w, h, args.num_disparities, args.block_size, args.iters, args.warmup, args.mode, args.streams,
                          args.batch_only, args.cost, args.census_window)
        print(json.dumps(r), flush=True)
        print(f"\n{r['streams']} streams of {r['frames']}, D = {r['num_disparities']}, bs = {r['block_size']}, mode "
              f"{r['mode']}, cost {r['cost']}{'' if r['census_window'] is None else ' ' + r['census_window']}; workspace {r['workspace_bytes'] / 1e6:.0f} MB; clock {r['clock_mhz_before']} / "
              f"{r['clock_mhz_after']} MHz; valid {r['valid_fraction']:.2f}; stream 0 equals the single-stream step: "
              f"{r.get('stream0_equals_single', 'not compared')}")
        print("\n| path | ms per step (events) | ms per step (wall) | frames/s |\n|---|---|---|---|")
        for key in (k for k in ("batch", "in_turn", "in_turn_late_readout") if k in r):
            v = r[key]
            print(f"| {key} | {v['step_ms_events']:.3f} | {v['step_ms_wall']:.3f} | {v['frames_per_s']:.0f} |")
        print("\n| stage of the batch | us |\n|---|---|")
        for k, us in r["stage_us"].items():
            print(f"| {k} | {us:.1f} |")
        if args.json:
            args.json.parent.mkdir(parents=True, exist_ok=True)
            args.json.write_text(json.dumps(r, indent=1))
        return
    r = bench(w, h, args.num_disparities, args.block_size, args.iters, args.warmup, args.mode, args.cost,
              args.census_window)
    print(json.dumps(r), flush=True)
    print(f"\nframe {r['frames']}, D = {r['num_disparities']}, bs = {r['block_size']}, mode {r['mode']}, cost "
          f"{r['cost']}{'' if r['census_window'] is None else ' ' + r['census_window']}: {r['frame_ms_events']:.3f} ms (events) / {r['frame_ms_wall']:.3f} ms (wall) per step + readout; "
          f"clock {r['clock_mhz_before']} / {r['clock_mhz_after']} MHz; valid {r['valid_fraction']:.2f}")
    print("\n| stage | us | volume GB/s | ns per chain step |\n|---|---|---|---|")
    for k, us in r["stage_us"].items():
        gb = r["volume_GBps"].get(k)
        ns = r["chain_ns_per_step"].get(k)
        print(f"| {k} | {us:.1f} | {'' if gb is None else f'{gb:.0f}'} | {'' if ns is None else f'{ns:.0f}'} |")
    print(f"| sum | {1e3 * r['stages_ms_sum']:.1f} | | |")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(r, indent=1))


if __name__ == "__main__":
    main()
