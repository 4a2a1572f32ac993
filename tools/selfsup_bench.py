#!/usr/bin/env python3
"""Time the label-free adaptation loss on the GPU and the training step built on it.

First figure: ms per call of the loss stage (the geometry-only ``sd_stereo_check`` plus ``sd_selfsup_loss``, through
``selfsup.SelfSupLoss.run``: five launches and the two tiny adds of the running totals) at 64 x 240x320 and at
1 x 720x960, against the same loss written in torch ops on the device in float32 and differentiated by autograd: the
suffix minimum by ``flip`` / ``cummin`` / ``flip``, the warp by ``gather`` (whose backward is a scatter-add), masked sums,
``backward()`` for the two gradient maps. Both forms are timed in the same process in alternating rounds (HIP events over
back-to-back calls, after a warm-up at the shape); the figures are the median round and the rounds themselves. The stage
is also captured into a HIP graph and replayed: the device's time without the host's enqueue. The bytes the stage must
move per pixel are 4 (disp) read and 1 (cls) written by the check, 4 (disp) + 4 (logvar) + 24 (input) + 1 (cls) read and
4 + 4 written by the loss: 46, over the time: the achieved GB/s (every call re-reads the same buffers; 64 x 240x320 is
226 MB of them and fits the Infinity Cache). How far the two forms' gradients are apart is recorded, not assumed.

Second figure: ms per ``adapt_step`` against ms per ``train_step`` of the full-width model at 64 x 240x320 in bf16, in the
same process in alternating rounds; ``train_step`` is the parent's, so their difference is what the label-free objective
costs over the supervised one.

With ``--ssim A`` (say 0.85, the literature's mix) the same figures are also taken for the loss with the SSIM term
(``SelfSupLoss(ssim=A)``, ``sd_selfsup_loss_ssim``): the stage beside the plain one and beside the same loss in torch ops
(window moments by ``avg_pool2d``-style shifted sums of the masked planes) with autograd, and ``adapt_step`` with the
term beside ``adapt_step`` without it, all in the same alternating rounds.

    python tools/selfsup_bench.py --json profiles/selfsup_bench.json
    python tools/selfsup_bench.py --ssim 0.85 --json profiles/selfsup_ssim_bench.json
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
from stereo_depth_estimation_amd import selfsup  # noqa: E402

CASES = ((240, 320, 64), (720, 960, 1))
BYTES_PER_PIXEL = 4 + 4 + 4 + 24 + 1 + 1 + 4 + 4
PARAMS = dict(w_photo=1.0, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10.0)


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
    """A smooth disparity (2..40 px) with 2 % NaN, a log-variance map and frames of low-pass noise in [0, 1]."""
    gen = torch.Generator(device=dev).manual_seed(0)
    coarse = torch.rand(n, 1, H // 16 + 2, W // 16 + 2, device=dev, generator=gen)
    disp = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear")[:, 0] * 38 + 2
    disp = disp.contiguous()
    disp[torch.rand(n, H, W, device=dev, generator=gen) < 0.02] = float("nan")
    logvar = torch.rand(n, H, W, device=dev, generator=gen) * 9 - 6
    x = torch.rand(n, 6, H // 2, W // 2, device=dev, generator=gen)
    x = torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear").contiguous()
    return disp, logvar, x


def _box(v, m, H, W):
    """The sum of the masked plane over the 3 x 3 window around every pixel."""
    q = torch.nn.functional.pad(v * m, (1, 1, 1, 1))
    return sum(q[..., i:i + H, j:j + W] for i in range(3) for j in range(3))


def torch_ssim(left, r, vis):
    """s per pixel in torch ops: the SSIM dissimilarity over the window's counted pixels."""
    H, W = left.shape[-2:]
    m = vis[:, None].float()
    k = _box(torch.ones_like(m), m, H, W).clamp(min=1)
    muL, mur = _box(left, m, H, W) / k, _box(r, m, H, W) / k
    sL = _box(left * left, m, H, W) / k - muL * muL
    sr = _box(r * r, m, H, W) / k - mur * mur
    sLr = _box(left * r, m, H, W) / k - muL * mur
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    S = ((2 * muL * mur + c1) * (2 * sLr + c2)) / ((muL * muL + mur * mur + c1) * (sL + sr + c2))
    return (1 - S).sum(dim=1) / 6


def torch_loss(disp, logvar, x, occ_tol: float, p: dict, ssim: float = 0.0):
    """The baseline: the geometry-only classes and the loss in torch ops (float32), autograd for the gradients. Returns
    (gdisp, glogvar, loss, counted)."""
    n, H, W = disp.shape
    dev = disp.device
    zero, inf = torch.zeros((), device=dev), torch.full((), float("inf"), device=dev)
    with torch.no_grad():
        has = torch.isfinite(disp) & (disp > 0)
        xr = torch.arange(W, device=dev, dtype=torch.float32) - torch.where(has, disp, zero)
        oov = has & (xr < 0)
        incl = torch.where(has, xr, inf).flip(-1).cummin(-1).values.flip(-1)
        m = torch.cat([incl[..., 1:], inf.expand(n, H, 1)], dim=-1)
        vis = has & ~oov & ~((m + occ_tol) <= xr)
        N = vis.sum().clamp(min=1).float()
        finite = torch.isfinite(disp)
    d = torch.where(finite, disp, zero).requires_grad_(True)
    lv = logvar.clone().requires_grad_(True)
    xs = torch.arange(W, device=dev, dtype=torch.float32) - torch.where(vis, d, zero)
    x0 = xs.detach().floor().long().clamp(0, W - 1)
    x1 = (x0 + 1).clamp(max=W - 1)
    f = xs - x0.float()
    left, right = x[:, :3], x[:, 3:]
    a = torch.gather(right, 3, x0[:, None].expand(-1, 3, -1, -1))
    b = torch.gather(right, 3, x1[:, None].expand(-1, 3, -1, -1))
    r = a + f[:, None] * (b - a)
    t = left - r
    e = torch.sqrt(t * t + p["eps"] ** 2).sum(dim=1) / 3
    if ssim > 0:
        e = (1 - ssim) * e + ssim * torch_ssim(left, r, vis)
    ell = e * torch.exp(-lv) + lv
    photo = torch.where(vis, ell, zero).sum() / N
    smooth = zero
    for ax in (2, 1):
        k = d.shape[ax] - 1
        ok = finite.narrow(ax, 0, k) & finite.narrow(ax, 1, k)
        g = (left.narrow(ax + 1, 1, k) - left.narrow(ax + 1, 0, k)).abs().sum(dim=1) / 3
        tx = d.narrow(ax, 1, k) - d.narrow(ax, 0, k)
        smooth = smooth + torch.where(ok, torch.exp(-p["gamma"] * g) * torch.sqrt(tx * tx + p["eps_s"] ** 2), zero).sum()
    loss = p["w_photo"] * photo + p["w_smooth"] * smooth / (n * H * W)
    loss.backward()
    return torch.where(finite, d.grad, zero), lv.grad, loss.detach(), vis.sum()


def bench_stage(a, dev) -> list:
    out = []
    for H, W, n in CASES:
        disp, logvar, x = scene(H, W, n, dev)
        loss = selfsup.SelfSupLoss(n, device=dev, **PARAMS)
        stage = lambda: loss.run(disp, logvar, x)  # noqa: E731
        base = lambda: torch_loss(disp, logvar, x, 0.5, PARAMS)  # noqa: E731
        res, ref = stage(), base()
        s = res.summary()
        scale = float(ref[0].abs().max())
        gd_diff = float((res.gdisp - ref[0]).abs().max()) / scale
        gl_diff = float((res.glogvar - ref[1]).abs().max()) / float(ref[1].abs().max())
        _events(stage, a.warmup, a.warmup)
        _events(base, 3, 3)
        ms_s, ms_t, wall_s = [], [], []
        for _ in range(a.rounds):  # alternating, in one process
            ms, wall = _events(stage, a.iters, 0)
            ms_s.append(ms)
            wall_s.append(wall)
            ms_t.append(_events(base, a.torch_iters, 0)[0])
        ms_graph = _graph_ms(stage, a.iters)
        ms, t_ms = statistics.median(ms_s), statistics.median(ms_t)
        moved = n * H * W * BYTES_PER_PIXEL
        extra = {}
        if a.ssim > 0:
            # the same rounds for the loss with the SSIM term, beside the plain stage's of this process
            loss_s = selfsup.SelfSupLoss(n, device=dev, ssim=a.ssim, **PARAMS)
            stage_s = lambda: loss_s.run(disp, logvar, x)  # noqa: E731
            base_s = lambda: torch_loss(disp, logvar, x, 0.5, PARAMS, a.ssim)  # noqa: E731
            res_s, ref_s = stage_s(), base_s()
            sum_s = res_s.summary()
            gd_s = float((res_s.gdisp - ref_s[0]).abs().max()) / float(ref_s[0].abs().max())
            _events(stage_s, a.warmup, a.warmup)
            _events(base_s, 3, 3)
            r_s, r_p, r_t = [], [], []
            for _ in range(a.rounds):
                r_s.append(_events(stage_s, a.iters, 0)[0])
                r_p.append(_events(stage, a.iters, 0)[0])
                r_t.append(_events(base_s, a.torch_iters, 0)[0])
            m_s, m_p, m_t = statistics.median(r_s), statistics.median(r_p), statistics.median(r_t)
            extra = {"ssim": a.ssim, "ssim_mean_s": sum_s["ssim"], "ssim_loss": sum_s["loss"],
                     "ssim_torch_loss": float(ref_s[2]), "ssim_ms_per_call": m_s, "ssim_ms_per_call_rounds": r_s,
                     "plain_ms_per_call_same_rounds": m_p, "ssim_over_plain": m_s / m_p,
                     "ssim_ms_per_call_graph_replay": _graph_ms(stage_s, a.iters),
                     "ssim_torch_ms_per_call": m_t, "ssim_torch_ms_per_call_rounds": r_t,
                     "ssim_speedup_vs_torch": m_t / m_s, "ssim_gdisp_max_diff_vs_torch_rel": gd_s}
            del loss_s, res_s, ref_s
        out.append({"H": H, "W": W, "samples": n, "pixels": n * H * W, **PARAMS, "occ_tol": 0.5, **extra,
                    "visible_fraction": s["visible_fraction"], "loss": s["loss"], "torch_loss": float(ref[2]),
                    "counted": int(res.count.item()), "torch_counted": int(ref[3]),
                    "ms_per_call": ms, "ms_per_call_rounds": ms_s, "ms_per_call_wall": statistics.median(wall_s),
                    "ms_per_call_graph_replay": ms_graph, "bytes_moved": moved,
                    "achieved_GBps": moved / (ms * 1e-3) / 1e9,
                    "achieved_GBps_graph_replay": moved / (ms_graph * 1e-3) / 1e9,
                    "torch_ms_per_call": t_ms, "torch_ms_per_call_rounds": ms_t, "speedup_vs_torch": t_ms / ms,
                    "gdisp_max_diff_vs_torch_rel": gd_diff, "glogvar_max_diff_vs_torch_rel": gl_diff})
        print(json.dumps(out[-1]))
        del loss, disp, logvar, x, res, ref
        torch.cuda.empty_cache()
    return out


def bench_step(a, dev) -> dict:
    """adapt_step against train_step, full-width model, 64 x 240x320, bf16, alternating rounds in one process."""
    from stereo_depth_estimation_amd.data import synthetic_batch
    from stereo_depth_estimation_amd.model import StereoUNet
    from stereo_depth_estimation_amd.optim import FusedAdamW
    from stereo_depth_estimation_amd.train import train_step

    B, H, W = 64, 240, 320
    torch.manual_seed(0)
    b = {k: v.to(dev) for k, v in synthetic_batch(B, H, W, seed=0).items()}
    m = StereoUNet(base_channels=32, precision="bf16").to(dev).train()
    opt = FusedAdamW(m.parameters(), lr=1e-6, weight_decay=0.0)
    loss = selfsup.SelfSupLoss(B, device=dev, **PARAMS)
    sup = lambda: train_step(m, opt, b["input"], b["target"], b["valid_mask"])  # noqa: E731
    ada = lambda: selfsup.adapt_step(m, opt, b["input"], loss)  # noqa: E731
    loss_s = selfsup.SelfSupLoss(B, device=dev, ssim=a.ssim, **PARAMS) if a.ssim > 0 else None
    ada_s = lambda: selfsup.adapt_step(m, opt, b["input"], loss_s)  # noqa: E731
    _events(sup, a.step_warmup, a.step_warmup)
    _events(ada, a.step_warmup, a.step_warmup)
    if loss_s is not None:
        _events(ada_s, a.step_warmup, a.step_warmup)
    ms_sup, ms_ada, ms_ada_s = [], [], []
    for _ in range(a.rounds):
        ms_sup.append(_events(sup, a.step_iters, 0)[0])
        ms_ada.append(_events(ada, a.step_iters, 0)[0])
        if loss_s is not None:
            ms_ada_s.append(_events(ada_s, a.step_iters, 0)[0])
    s, d = statistics.median(ms_sup), statistics.median(ms_ada)
    out = {"batch": B, "H": H, "W": W, "precision": "bf16", "base_channels": 32, "train_step_ms": s,
           "train_step_ms_rounds": ms_sup, "adapt_step_ms": d, "adapt_step_ms_rounds": ms_ada,
           "adapt_minus_train_ms": d - s, "adapt_over_train": d / s, "means": loss.means()}
    if loss_s is not None:
        ds = statistics.median(ms_ada_s)
        out.update({"ssim": a.ssim, "adapt_step_ssim_ms": ds, "adapt_step_ssim_ms_rounds": ms_ada_s,
                    "adapt_ssim_minus_adapt_ms": ds - d, "adapt_ssim_over_adapt": ds / d, "ssim_means": loss_s.means()})
    print(json.dumps(out))
    return out


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=500, help="Calls of the stage per round.")
    ap.add_argument("--torch-iters", type=int, default=20, help="Calls of the torch form per round.")
    ap.add_argument("--step-iters", type=int, default=30, help="Training steps of each kind per round.")
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--ssim", type=float, default=0.0,
                    help="Also measure the loss with this SSIM weight (0.85 is the literature's mix, not an optimum).")
    ap.add_argument("--json", type=str, default=None, help="Write the results here.")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("selfsup_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    L.load()
    out = {"tool": "tools/selfsup_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "torch_iters": a.torch_iters, "step_iters": a.step_iters, "rounds": a.rounds, "warmup": a.warmup,
           "bytes_per_pixel": BYTES_PER_PIXEL, "stage": bench_stage(a, dev), "step": bench_step(a, dev)}
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
