"""Cost of the uncertainty evaluation: sd_uncert_eval (csrc/uncert.hip) alone, against the same figures as torch ops and
against sd_disp_export's metric pass, and what ``predict --eval-uncertainty`` costs the tool.

    python tools/uncert_bench.py [--pairs 512] [--rounds 3] [--precision bf16] [--parent-root DIR]
                                 [--out profiles/uncert_bench.json]

The parent process never touches the GPU: every arm runs as a child process under its own time limit, and after a child
that fails or overruns nothing more is started (tools/predict_bench.py's scheme; its synthetic tree, frame size 960x540
unless a dataset is found, model 240x320, batch 32, at most 16 host threads). Arms alternate over the rounds:
  kernel   by device events at B = 32, 240x320 -> 540x960, 20 cuts, 10 warm-up launches then 5 repeats of 50 launches,
           on two kinds of input: "smooth" maps (low-frequency, as a trained model's: the lanes of a wave fall into the
           same few bins, the worst case for the LDS atomics) and "random" ones (every lane its own bin):
             a  sd_uncert_eval (memset node + histogram pass + scan pass)                      -> us
             b  the same figures as torch ops on the device: F.interpolate of both maps, the decode, two stable
                torch.sort per image, gather + cumsum, the cuts, NLL and coverage               -> us
             c  sd_disp_export with the metric rows alone: one pass over the same pixels       -> us
  c_off    predict_dataset evaluating only, without the flag                                   -> pairs/s
  c_on     the same with eval_uncertainty=True                                                 -> pairs/s
  c_parent c_off run from --parent-root, a built checkout of the parent commit (skipped without it) -> pairs/s
  device   the pipeline's device stage alone (H2D + preprocess + forward + export [+ sd_uncert_eval] + D2H, synchronised
           per batch), without and with the flag                                               -> ms per batch of 32
Prints one JSON line with the per-round figures, medians and ranges; --out also writes it to a file."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG_ROOT = Path(os.environ.get("UNCERT_BENCH_PKG_ROOT") or ROOT)  # c_parent: the package of another checkout
sys.path.insert(0, str(ROOT / "tools"))

from cache_bench import ASSUMED_SIZE, DEFAULT_ROOTS, real_frame_size, write_tree  # noqa: E402

sys.path.insert(0, str(PKG_ROOT))  # after cache_bench, which puts its own checkout first

H, W, BATCH, THREADS, WARM, STEPS = 240, 320, 32, 16, 64, 20
LIMITS = {"kernel": 240, "c_off": 300, "c_on": 300, "c_parent": 300, "device": 300}  # seconds per child


def make_model(precision: str):
    import torch

    from stereo_depth_estimation_amd.model import StereoUNet

    torch.manual_seed(0)
    return StereoUNet(base_channels=32, precision=precision).to("cuda").eval()


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


# ------------------------------------------------------------------------------------------- children (GPU)
def arm_kernel(root: Path, precision: str) -> dict:
    import torch
    import torch.nn.functional as F

    from stereo_depth_estimation_amd import _lib as L

    L.load()
    dev = torch.device("cuda")
    Hs, Ws = ASSUMED_SIZE
    mul = Ws / float(W)
    g = torch.Generator().manual_seed(0)

    def inputs(kind):
        if kind == "random":
            disp = torch.rand(BATCH, H, W, generator=g) * 60
            logvar = torch.rand(BATCH, H, W, generator=g) * 5 - 4
        else:
            yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
            ph = torch.rand(BATCH, 1, 1, generator=g) * 6.28
            disp = 30 + 25 * torch.sin(3 * xx[None] + 2 * yy[None] + ph)
            logvar = -1.5 + 1.5 * torch.cos(2 * xx[None] - 3 * yy[None] + ph)
        disp, logvar = disp.to(dev).contiguous(), logvar.to(dev).contiguous()
        d_up = F.interpolate(disp[:, None], size=(Hs, Ws), mode="bilinear", align_corners=False)[:, 0] * mul
        lv_up = F.interpolate(logvar[:, None], size=(Hs, Ws), mode="bilinear", align_corners=False)[:, 0]
        noise = torch.distributions.Laplace(0.0, 1.0).sample(d_up.shape).to(dev) * torch.exp(lv_up) * mul
        c = torch.round(torch.clamp((d_up + noise).double() * 1000, 0, 16646655)).long()
        c[torch.rand(c.shape, device=dev) < 0.1] = 0
        gt = torch.stack([c // 65025, (c % 65025) // 255, (c % 65025) % 255], -1).to(torch.uint8).contiguous()
        return disp, logvar, gt

    def timed(fn, launches=50, repeats=5):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / launches * 1e3)
        return spread(out)

    s = L.stream_handle(dev)
    rows = torch.zeros(BATCH, 16 + 2 * STEPS, dtype=torch.float64, device=dev)
    work = torch.empty(L.call("sd_uncert_eval_ws_bytes", BATCH, Hs, Ws, STEPS) // 8, dtype=torch.float64, device=dev)
    mrows = torch.zeros(BATCH, 8, dtype=torch.float64, device=dev)
    mwork = torch.zeros(L.call("sd_disp_export_ws_bytes", BATCH, Hs, Ws) // 8, dtype=torch.float64, device=dev)
    cuts = torch.arange(STEPS, device=dev)
    out = {"source_hw": [Hs, Ws], "steps": STEPS}
    for kind in ("smooth", "random"):
        disp, logvar, gt = inputs(kind)

        def uncert():
            L.call("sd_uncert_eval", disp.data_ptr(), logvar.data_ptr(), BATCH, H, W, gt.data_ptr(), Hs, Ws, STEPS,
                   rows.data_ptr(), work.data_ptr(), s)

        def export_rows():
            L.call("sd_disp_export", disp.data_ptr(), None, BATCH, H, W, gt.data_ptr(), Hs, Ws, None, None, None,
                   mrows.data_ptr(), mwork.data_ptr(), s)

        def torch_route():
            d = F.interpolate(disp[:, None], size=(Hs, Ws), mode="bilinear", align_corners=False)[:, 0] * mul
            lv = F.interpolate(logvar[:, None], size=(Hs, Ws), mode="bilinear", align_corners=False)[:, 0]
            t = gt.to(torch.float32)
            t = (t[..., 0] * 65025 + t[..., 1] * 255 + t[..., 2]) / 1000
            m = (t > 0) & torch.isfinite(d) & torch.isfinite(lv)
            e = (d - t).abs()
            n = m.flatten(1).sum(1)
            keep = n[:, None] - (n[:, None] * cuts[None]) // STEPS
            ef = torch.where(m, e, 0.0).flatten(1)
            curves = []
            for key in (lv, e):
                order = torch.sort(torch.where(m, key, float("inf")).flatten(1), dim=1, stable=True).indices
                cs = torch.cumsum(ef.gather(1, order).double(), 1)
                curves.append(cs.gather(1, (keep - 1).clamp(min=0)) / keep.clamp(min=1))
            e_m = e / mul
            nll = torch.where(m, e_m * torch.exp(-lv) + lv, 0.0).double().flatten(1).sum(1)
            b = torch.exp(lv)
            cov = [(m & (e_m <= z * b)).flatten(1).sum(1) for z in (0.5, 1.0, 2.0, 3.0)]
            return curves, nll, cov, n

        res = {"a_uncert_eval_us": timed(uncert), "c_disp_export_rows_us": timed(export_rows),
               "b_torch_ops_us": timed(torch_route, launches=5, repeats=5)}
        res["a_over_c"] = res["a_uncert_eval_us"]["median"] / res["c_disp_export_rows_us"]["median"]
        res["b_over_a"] = res["b_torch_ops_us"]["median"] / res["a_uncert_eval_us"]["median"]
        # the two routes agree on what they measure (the binned curve against the sorted one, sample 0)
        uncert()
        curves, nll, cov, n = torch_route()
        torch.cuda.synchronize()
        r0 = rows[0].cpu().numpy()
        res["check_n"] = [float(r0[0]), float(n[0])]
        res["check_unc_last_binned_vs_sorted"] = [float(r0[16 + STEPS - 1]), float(curves[0][0, -1])]
        res["check_ause"] = float(r0[7])
        out[kind] = res
    return out


def _predict(model, root: Path, max_samples: int = 0, **kw) -> dict:
    from stereo_depth_estimation_amd.predict import predict_dataset

    return predict_dataset(None, root, None, model=model, height=H, width=W, batch_size=BATCH,
                           max_samples=max_samples, read_threads=THREADS, **kw)


def arm_c(root: Path, precision: str, **kw) -> dict:
    model = make_model(precision)
    _predict(model, root, max_samples=WARM, **kw)
    t0 = time.perf_counter()
    meta = _predict(model, root, **kw)
    dt = time.perf_counter() - t0
    out = {"pairs": meta["num_samples"], "seconds": dt, "pairs_s": meta["num_samples"] / dt, "epe": meta["epe"]}
    if kw:
        out["ause"] = meta["uncertainty"]["ause"]
    return out


def arm_c_on(root: Path, precision: str) -> dict:
    return arm_c(root, precision, eval_uncertainty=True, sparsification_steps=STEPS)


def arm_device(root: Path, precision: str) -> dict:
    import torch

    from stereo_depth_estimation_amd import predict as P
    from stereo_depth_estimation_amd.uncert import UncertaintyEval

    items = P.dataset_items(root)[:4 * BATCH]
    batches = P.plan_batches(items, BATCH)
    predictor = P.Predictor(make_model(precision), (W, H))
    out = {}
    for name, unc in (("off", None), ("on", UncertaintyEval(STEPS, predictor.device))):
        pipe = P.PredictPipeline(predictor, BATCH, True, False, False, 1, THREADS, None, None, unc)
        parts = pipe.decode(0, *batches[0])
        for _ in range(3):
            ev, _ = pipe.device_work(0, parts)
            ev.synchronize()
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(8):
                ev, _ = pipe.device_work(0, parts)
                ev.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / 8)
        out[f"{name}_ms_per_batch"] = statistics.median(ms)
        out[f"{name}_ms_per_batch_range"] = [min(ms), max(ms)]
    return out


ARMS = {"kernel": arm_kernel, "c_off": arm_c, "c_on": arm_c_on, "c_parent": arm_c, "device": arm_device}


# ------------------------------------------------------------------------------------------------- parent
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", type=str, default="bf16", choices=("fp32", "bf16", "fp8"))
    ap.add_argument("--arms", type=str, default="kernel,c_off,c_on,c_parent,device")
    ap.add_argument("--parent-root", type=str, default=None, help="A built checkout of the parent commit (c_parent).")
    ap.add_argument("--dataset-root", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", nargs=2, metavar=("ARM", "ROOT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        arm, root = a.child
        print("RESULT " + json.dumps(ARMS[arm](Path(root), a.precision)), flush=True)
        return

    arms = [x for x in a.arms.split(",") if x != "c_parent" or a.parent_root]
    size, found = real_frame_size((a.dataset_root,) + DEFAULT_ROOTS)
    out = {"pairs": a.pairs, "model_hw": [H, W], "batch": BATCH, "host_threads": THREADS, "precision": a.precision,
           "steps": STEPS, "source_hw": list(size or ASSUMED_SIZE),
           "source_hw_from": found or "ASSUMED (no dataset on this machine)", "parent_measured": bool(a.parent_root),
           "rounds": {}}
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        root = Path(tmp) / "data"
        write_tree(root, a.pairs, *out["source_hw"])
        ok = True
        for rnd in range(a.rounds):
            for arm in arms:
                if arm == "kernel" and rnd:
                    continue  # its repeats are inside the child
                env = dict(os.environ)
                if arm == "c_parent":
                    env["UNCERT_BENCH_PKG_ROOT"] = str(Path(a.parent_root).resolve())
                cmd = ["timeout", "-k", "10", str(LIMITS[arm]), sys.executable, str(Path(__file__).resolve()),
                       "--precision", a.precision, "--child", arm, str(root)]
                p = subprocess.run(cmd, capture_output=True, text=True, env=env)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    out["failed"] = {"arm": arm, "round": rnd, "returncode": p.returncode, "stderr": p.stderr[-2000:]}
                    ok = False
                    break
                out["rounds"].setdefault(arm, []).append(json.loads(lines[-1][7:]))
                print(f"round {rnd} {arm}: {out['rounds'][arm][-1]}", file=sys.stderr, flush=True)
            if not ok:
                break  # nothing more is started on the GPU after a child that failed or overran
    summary = {}
    for arm, runs in out["rounds"].items():
        for k in runs[0]:
            if k.endswith(("pairs_s", "ms_per_batch")):
                summary[f"{arm}_{k}"] = {n: round(v, 3) for n, v in spread([r[k] for r in runs]).items()}
    if "kernel" in out["rounds"]:
        summary["kernel"] = out["rounds"]["kernel"][0]
    out["summary"] = summary
    print(json.dumps(out), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
