#!/usr/bin/env python3
"""Time proxy-label adaptation on the GPU: its three stages, the loss stage against torch ops, and the training step.

First figures, at 64 x 240x320: ms per call of ``sd_proxy_gray``, of the matcher (``StereoSGM.compute_batch``, D = 64,
block 5, 3-way) and of ``sd_proxy_loss`` (four launches; accumulate mode onto existing maps, and overwrite mode), each
on its own, by HIP events over back-to-back calls after a warm-up at the shape; the loss stage also captured into a HIP
graph and replayed (the device's time without the host's enqueue). The bytes the loss stage must move per pixel are
4 (disp) + 2 (label) read by the count, 4 + 4 (logvar) + 2 read and 4 + 4 read and written by the pass in accumulate
mode: 32 (26 in the pass), over the time: the achieved GB/s (every call re-reads the same buffers, which fit the
Infinity Cache).

Second: the loss stage against the same masked NLL and its gradient written in torch ops (float32) with autograd on
the same tensors, both in the same process in alternating rounds; how far the two forms' gradients are apart is
recorded, not assumed.

Third: ms per ``adapt_step`` with ``proxy=`` (photometric + proxy), labels only, and without a proxy (the parent's
code path) of the full-width model at 64 x 240x320 in bf16, in alternating rounds.

    python tools/proxy_bench.py --json profiles/proxy_bench.json

``--census-window HxW`` adds, in the same alternating rounds, the matcher and the two proxy steps with the census /
Hamming pixel cost of that window (``ProxyLoss(cost="census")``): ``matcher_census``, ``adapt_step_proxy_census`` and
``adapt_step_proxy_only_census``, and their ratios to the Birchfield-Tomasi figures.

    python tools/proxy_bench.py --census-window 7x9 --json profiles/proxy_census_bench.json
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from selfsup_bench import _events, _graph_ms  # noqa: E402

from stereo_depth_estimation_amd import _lib as L  # noqa: E402
from stereo_depth_estimation_amd import proxy, selfsup  # noqa: E402

B, H, W = 64, 240, 320
COUNT_BYTES, PASS_BYTES = 4 + 2, 4 + 4 + 2 + 2 * (4 + 4)
MATCHER = dict(num_disparities=64, block_size=5, mode="3way")


def scene(dev):
    """A stereo batch with a known smooth disparity (4..40 px): the right view is low-pass noise, the left view the right
    one warped. Returns inputs float32 [B, 6, H, W] in [0, 1], a disparity prediction near the truth and a logvar map."""
    gen = torch.Generator(device=dev).manual_seed(0)
    right = torch.rand(B, 3, H // 2, (W + 64) // 2, device=dev, generator=gen)
    right = torch.nn.functional.interpolate(right, size=(H, W + 64), mode="bilinear")
    coarse = torch.rand(B, 1, H // 32 + 2, W // 32 + 2, device=dev, generator=gen)
    d = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear")[:, 0] * 36 + 4
    xr = torch.arange(W, device=dev, dtype=torch.float32) - d + 48  # the right view's columns start 48 into the noise
    x0 = xr.floor().long().clamp(0, W + 62)
    f = (xr - x0.float())[:, None]
    idx = x0[:, None].expand(-1, 3, -1, -1)
    left = torch.gather(right, 3, idx) * (1 - f) + torch.gather(right, 3, idx + 1) * f
    x = torch.cat([left, right[..., 48:48 + W]], dim=1).contiguous()
    disp = (d + torch.randn(B, H, W, device=dev, generator=gen)).contiguous()
    logvar = torch.rand(B, H, W, device=dev, generator=gen) * 4 - 3
    return x, disp, logvar


def torch_loss(disp, logvar, q4, w: float):
    """The baseline: the masked NLL of the labelled pixels in torch ops (float32), autograd for the two gradients."""
    d = disp.clone().requires_grad_(True)
    lv = logvar.clone().requires_grad_(True)
    target = q4.float() / 16
    valid = (q4 > 0) & torch.isfinite(d)
    err = (torch.where(valid, d, torch.zeros_like(d)) - target).abs()
    ell = err * torch.exp(-lv) + lv
    loss = w * torch.where(valid, ell, torch.zeros_like(ell)).sum() / valid.sum().clamp(min=1)
    loss.backward()
    return d.grad, lv.grad, loss.detach()


def rounds_of(fns: dict, iters: dict, rounds: int) -> dict:
    """Median ms per call and the rounds of every function, timed in alternating rounds in this process."""
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(_events(fn, iters[k], 0)[0])
    return {k: {"ms_per_call": statistics.median(v), "rounds": v} for k, v in ms.items()}


def bench_stages(a, dev) -> dict:
    x, disp, logvar = scene(dev)
    px = proxy.ProxyLoss(B, device=dev, **MATCHER)
    pc = proxy.ProxyLoss(B, device=dev, cost="census", census_window=a.census_window, **MATCHER) if a.census_window else None
    q4 = px.labels(x).clone()
    stream = lambda: L.stream_handle(dev)  # noqa: E731 (the current stream: a graph capture has its own)
    n = B * H * W
    gray = torch.empty(2, B, H, W, dtype=torch.uint8, device=dev)
    gd, gl = torch.zeros(B, H, W, device=dev), torch.zeros(B, H, W, device=dev)
    rows = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(L.call("sd_proxy_ws_bytes", B, H, W) // 8, dtype=torch.float64, device=dev)
    q_out = torch.empty_like(q4)

    def loss_call(acc):
        return lambda: L.call("sd_proxy_loss", B, disp.data_ptr(), logvar.data_ptr(), q4.data_ptr(), H, W, 1.0, acc,
                              gd.data_ptr(), gl.data_ptr(), rows.data_ptr(), count.data_ptr(), work.data_ptr(), stream())

    fns = {"gray": lambda: L.call("sd_proxy_gray", B, x.data_ptr(), H, W, gray[0].data_ptr(), gray[1].data_ptr(),
                                  stream()),
           "matcher": lambda: px.matcher.compute_batch(gray[0], gray[1], out=q_out),
           **({"matcher_census": lambda: pc.matcher.compute_batch(gray[0], gray[1], out=q_out)} if pc else {}),
           "loss_accumulate": loss_call(1), "loss_overwrite": loss_call(0),
           "torch_loss": lambda: torch_loss(disp, logvar, q4, 1.0)}
    iters = {"gray": a.iters, "matcher": a.matcher_iters, "matcher_census": a.matcher_iters, "loss_accumulate": a.iters,
             "loss_overwrite": a.iters, "torch_loss": a.torch_iters}
    # the two forms' numbers on the same tensors
    fns["loss_overwrite"]()
    ref = torch_loss(disp, logvar, q4, 1.0)
    summary = px.run(disp, logvar, x).summary()
    diffs = {"gdisp_max_diff_vs_torch_rel": float((gd - ref[0]).abs().max() / ref[0].abs().max()),
             "glogvar_max_diff_vs_torch_rel": float((gl - ref[1]).abs().max() / ref[1].abs().max()),
             "torch_loss_value": float(ref[2]), **summary}
    for k, fn in fns.items():
        _events(fn, 3 if k in ("matcher", "matcher_census", "torch_loss") else a.warmup, 3)
    out = rounds_of(fns, iters, a.rounds)
    for k in ("loss_accumulate", "loss_overwrite"):
        out[k]["ms_per_call_graph_replay"] = _graph_ms(fns[k], a.iters)
    acc = out["loss_accumulate"]
    acc["bytes_moved"] = n * (COUNT_BYTES + PASS_BYTES)
    acc["achieved_GBps"] = acc["bytes_moved"] / (acc["ms_per_call"] * 1e-3) / 1e9
    acc["achieved_GBps_graph_replay"] = acc["bytes_moved"] / (acc["ms_per_call_graph_replay"] * 1e-3) / 1e9
    out["loss_speedup_vs_torch"] = out["torch_loss"]["ms_per_call"] / out["loss_overwrite"]["ms_per_call"]
    out.update(batch=B, H=H, W=W, pixels=n, matcher_params=MATCHER, **diffs)
    if pc:
        out["census_window"] = "%dx%d" % pc.matcher.census_window
        out["matcher_census_over_matcher"] = out["matcher_census"]["ms_per_call"] / out["matcher"]["ms_per_call"]
        out["census_labels"] = pc.run(disp, logvar, x).summary()
    print(json.dumps(out))
    return out


def bench_step(a, dev) -> dict:
    """adapt_step with a proxy, labels only and without a proxy: full-width model, bf16, alternating rounds."""
    from stereo_depth_estimation_amd.model import StereoUNet
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x, _, _ = scene(dev)
    torch.manual_seed(0)
    m = StereoUNet(base_channels=32, precision="bf16").to(dev).train()
    opt = FusedAdamW(m.parameters(), lr=1e-6, weight_decay=0.0)
    loss = selfsup.SelfSupLoss(B, device=dev)
    px = proxy.ProxyLoss(B, device=dev, **MATCHER)
    fns = {"adapt_step": lambda: selfsup.adapt_step(m, opt, x, loss),
           "adapt_step_proxy": lambda: selfsup.adapt_step(m, opt, x, loss, proxy=px),
           "adapt_step_proxy_only": lambda: selfsup.adapt_step(m, opt, x, None, proxy=px)}
    if a.census_window:
        pc = proxy.ProxyLoss(B, device=dev, cost="census", census_window=a.census_window, **MATCHER)
        fns["adapt_step_proxy_census"] = lambda: selfsup.adapt_step(m, opt, x, loss, proxy=pc)
        fns["adapt_step_proxy_only_census"] = lambda: selfsup.adapt_step(m, opt, x, None, proxy=pc)
    for fn in fns.values():
        _events(fn, a.step_warmup, a.step_warmup)
    out = rounds_of(fns, {k: a.step_iters for k in fns}, a.rounds)
    base = out["adapt_step"]["ms_per_call"]
    out.update(batch=B, H=H, W=W, precision="bf16", base_channels=32,
               proxy_minus_adapt_ms=out["adapt_step_proxy"]["ms_per_call"] - base,
               proxy_over_adapt=out["adapt_step_proxy"]["ms_per_call"] / base,
               proxy_only_over_adapt=out["adapt_step_proxy_only"]["ms_per_call"] / base,
               means=loss.means(), proxy_means=px.means())
    if a.census_window:
        out.update(census_window="%dx%d" % pc.matcher.census_window,
                   proxy_census_over_proxy=out["adapt_step_proxy_census"]["ms_per_call"]
                   / out["adapt_step_proxy"]["ms_per_call"],
                   proxy_only_census_over_proxy_only=out["adapt_step_proxy_only_census"]["ms_per_call"]
                   / out["adapt_step_proxy_only"]["ms_per_call"], proxy_census_means=pc.means())
    print(json.dumps(out))
    return out


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=300, help="Calls of a stage per round.")
    ap.add_argument("--matcher-iters", type=int, default=10, help="Calls of the matcher per round.")
    ap.add_argument("--torch-iters", type=int, default=20, help="Calls of the torch form per round.")
    ap.add_argument("--step-iters", type=int, default=15, help="Training steps of each kind per round.")
    ap.add_argument("--step-warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--census-window", type=str, default=None,
                    help="HxW: also time the matcher and the proxy steps with the census cost of this window.")
    ap.add_argument("--json", type=str, default=None, help="Write the results here.")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("proxy_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    L.load()
    out = {"tool": "tools/proxy_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "matcher_iters": a.matcher_iters, "torch_iters": a.torch_iters, "step_iters": a.step_iters, "rounds": a.rounds,
           "warmup": a.warmup, "stages": bench_stages(a, dev)}
    torch.cuda.empty_cache()
    out["step"] = bench_step(a, dev)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
