"""Predict-and-evaluate throughput: stereo_depth_estimation_amd/predict.py against the route a user had before it, a
Python loop per batch (PIL decode, model(x), F.interpolate on the device, .cpu(), NumPy encoding of the RGB24 codes,
preview.write_png at zlib level 6, NumPy metrics).

    python tools/predict_bench.py [--pairs 512] [--rounds 3] [--precision bf16] [--dataset-root DIR]
                                  [--out profiles/predict_bench.json]

Synthesises `--pairs` PNG triplets (smooth images plus noise, as tools/cache_bench.py; freshly written, so every arm
reads them from the page cache) at the real dataset's frame size when a FoundationStereo tree is found under
--dataset-root or the CLI defaults, else at 960x540, which is then an ASSUMPTION about the dataset and is reported as
such. The model is the full-width StereoUNet (base 32, seeded random weights: the arithmetic does not depend on the
weights) at 240x320, batch 32, at most 16 host threads.

The parent process never touches the GPU: every arm runs as a child process under its own time limit, and after a
child that fails or overruns nothing more is started. Arms alternate over the rounds (a b c stages write kernel, a b
...); a child warms its route up on the first 64 samples, then times one pass over all of them:
  a       the Python loop described above (decode by a 16-thread PIL pool, which is generous to it)  -> pairs/s
  b       predict_dataset with an output root (disparity files written)                             -> pairs/s
  c       predict_dataset evaluating only                                                           -> pairs/s
  stages  the pipeline's three stages each alone over the same batches -> ms per batch of 32: decode (PNG files ->
          pinned frames), device (H2D + sd_stereo_preprocess + forward + sd_disp_export + D2H, synchronised per
          batch), write (pinned bytes -> PNG files at level 1)
  write   the write stage at --png-level 1 and 6 -> ms and bytes per file
  kernel  sd_disp_export alone by device events at B = 32, 240x320 -> 540x960, all outputs, its four-pixel and its
          per-pixel store path (disp_rgb one byte off alignment) -> us, the bytes moved computed from the shapes, and
          their share of the 8.0 TB/s HBM peak (MI355X_MICROARCH.md; 6.29 TB/s measured for a float4 copy)
Prints one JSON line with the per-round figures, medians and ranges; --out also writes it to a file."""

import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from cache_bench import ASSUMED_SIZE, DEFAULT_ROOTS, real_frame_size, write_tree  # noqa: E402

H, W, BATCH, THREADS, WARM = 240, 320, 32, 16, 64
HBM_PEAK = 8.0e12
LIMITS = {"a": 900, "b": 300, "c": 300, "stages": 300, "write": 300, "kernel": 120}  # seconds per child


def make_model(precision: str):
    import torch

    from stereo_depth_estimation_amd.model import StereoUNet

    torch.manual_seed(0)
    return StereoUNet(base_channels=32, precision=precision).to("cuda").eval()


# ------------------------------------------------------------------------------------------- children (GPU)
def arm_a(root: Path, scratch: Path, precision: str) -> dict:
    """The route without predict.py. The preprocessing is sd_stereo_preprocess (DeviceLoader's kernel, which a user
    has today); everything after the forward is host Python per image."""
    import torch
    import torch.nn.functional as F

    from stereo_depth_estimation_amd import _lib as L
    from stereo_depth_estimation_amd import dataset as D
    from stereo_depth_estimation_amd.preview import write_png

    L.load()
    dev = torch.device("cuda")
    model = make_model(precision)
    samples = D.discover_samples(root)
    pool = ThreadPoolExecutor(THREADS)

    def one_pass(sm, out_root):
        rows = np.zeros(7)
        for i in range(0, len(sm), BATCH):
            part = sm[i:i + BATCH]
            paths = [p for s in part for p in (s.left_rgb_path, s.right_rgb_path, s.disparity_path)]
            frames = list(pool.map(D.read_rgb_uint8, paths))
            left, right, gt = (np.stack(frames[k::3]) for k in range(3))
            n, Hs, Ws = left.shape[:3]
            ld, rd, gd = (torch.from_numpy(a).to(dev) for a in (left, right, gt))
            inp = torch.empty(n, 6, H, W, device=dev)
            tgt = torch.empty(n, 1, H, W, device=dev)
            val = torch.empty(n, 1, H, W, device=dev, dtype=torch.bool)
            L.call("sd_stereo_preprocess", ld.data_ptr(), rd.data_ptr(), gd.data_ptr(), n, Hs, Ws, H, W, inp.data_ptr(),
                   tgt.data_ptr(), val.data_ptr(), L.stream_handle(dev))
            with torch.inference_mode():
                d = model(inp)
                up = F.interpolate(d, size=(Hs, Ws), mode="bilinear", align_corners=False) * (Ws / float(W))
            up = up[:, 0].cpu().numpy()
            for k, s in enumerate(part):
                c = np.round(np.clip(np.nan_to_num(up[k]) * 1000.0, 0, 16646655)).astype(np.int64)
                r = c // 65025
                rem = c - r * 65025
                g = rem // 255
                rgb = np.stack([r, g, rem - g * 255], axis=-1).astype(np.uint8)
                dst = out_root / D.sample_cache_relpath(s).with_suffix(".png")
                dst.parent.mkdir(parents=True, exist_ok=True)
                write_png(dst, rgb)
                t = gt[k].astype(np.float32)
                t = (t[..., 0] * 65025 + t[..., 1] * 255 + t[..., 2]) / np.float32(1000)
                m = t > 0
                e = np.abs(up[k][m] - t[m]).astype(np.float64)
                rows += [m.sum(), e.sum(), (e * e).sum(), (e > 1).sum(), (e > 2).sum(), (e > 3).sum(),
                         ((e > 3) & (e > 0.05 * t[m])).sum()]
        return rows

    one_pass(samples[:WARM], scratch / "warm")
    t0 = time.perf_counter()
    rows = one_pass(samples, scratch / "out")
    dt = time.perf_counter() - t0
    return {"pairs": len(samples), "seconds": dt, "pairs_s": len(samples) / dt, "epe": rows[1] / max(rows[0], 1)}


def _predict(model, root: Path, out_root, max_samples: int = 0) -> dict:
    from stereo_depth_estimation_amd.predict import predict_dataset

    return predict_dataset(None, root, out_root, model=model, height=H, width=W, batch_size=BATCH,
                           max_samples=max_samples, read_threads=THREADS)


def arm_b(root: Path, scratch: Path, precision: str, write: bool = True) -> dict:
    model = make_model(precision)
    _predict(model, root, scratch / "warm" if write else None, max_samples=WARM)
    t0 = time.perf_counter()
    meta = _predict(model, root, scratch / "out" if write else None)
    dt = time.perf_counter() - t0
    return {"pairs": meta["num_samples"], "seconds": dt, "pairs_s": meta["num_samples"] / dt, "epe": meta["epe"]}


def arm_c(root: Path, scratch: Path, precision: str) -> dict:
    return arm_b(root, scratch, precision, write=False)


def _pipeline(root: Path, precision: str):
    from stereo_depth_estimation_amd import predict as P

    items = P.dataset_items(root)
    batches = P.plan_batches(items, BATCH)
    pipe = P.PredictPipeline(P.Predictor(make_model(precision), (W, H)), BATCH, True, True, False, 1, THREADS)
    return items, batches, pipe


def arm_stages(root: Path, scratch: Path, precision: str) -> dict:
    import torch

    items, batches, pipe = _pipeline(root, precision)
    out = {"batches": len(batches), "pairs": len(items)}
    (scratch / "warm").mkdir(parents=True)
    (scratch / "out").mkdir(parents=True)
    n = len(batches[0][1])
    for _ in range(3):  # warm-up: buffers pinned, the eval graph captured, first files written
        parts = pipe.decode(0, *batches[0])
        ev, outs = pipe.device_work(0, parts)
        pipe.write([scratch / "warm" / f"{i}.png" for i in range(n)], None, ev, outs)
    t0 = time.perf_counter()
    for hw, its in batches:
        parts = pipe.decode(0, hw, its)
    out["decode_ms_per_batch"] = 1e3 * (time.perf_counter() - t0) / len(batches)
    n = len(batches[-1][1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in batches:  # the last decoded batch again: the same bytes moved and computed per batch
        ev, outs = pipe.device_work(0, parts)
        ev.synchronize()
    out["device_ms_per_batch"] = 1e3 * (time.perf_counter() - t0) / len(batches)
    t0 = time.perf_counter()
    for b in range(len(batches)):
        pipe.write([scratch / "out" / f"{b}_{i}.png" for i in range(n)], None, ev, outs)
    out["write_ms_per_batch"] = 1e3 * (time.perf_counter() - t0) / len(batches)
    return out


def arm_write(root: Path, scratch: Path, precision: str) -> dict:
    """One batch of real predictions (smooth maps, as a trained model's are not guaranteed to be: the random model's
    output is what is at hand) written 8 times at each level."""
    from stereo_depth_estimation_amd.dataset import write_png_batch

    items, batches, pipe = _pipeline(root, precision)
    ev, outs = pipe.device_work(0, pipe.decode(0, *batches[0]))
    ev.synchronize()
    n, hw, h_disp, _, _ = outs[0]
    out = {"files_per_batch": n}
    for level in (1, 6):
        d = scratch / f"level{level}"
        d.mkdir(parents=True)
        write_png_batch([d / f"w_{i}.png" for i in range(n)], hw, h_disp, level, THREADS)  # warm
        t0 = time.perf_counter()
        for r in range(8):
            write_png_batch([d / f"{r}_{i}.png" for i in range(n)], hw, h_disp, level, THREADS)
        dt = time.perf_counter() - t0
        out[f"level{level}_ms_per_batch"] = 1e3 * dt / 8
        out[f"level{level}_ms_per_file"] = 1e3 * dt / (8 * n)
        out[f"level{level}_bytes_per_file"] = sum((d / f"0_{i}.png").stat().st_size for i in range(n)) / n
    return out


def arm_kernel(root: Path, scratch: Path, precision: str) -> dict:
    import torch

    from stereo_depth_estimation_amd import _lib as L

    L.load()
    dev = torch.device("cuda")
    Hs, Ws = ASSUMED_SIZE
    g = torch.Generator().manual_seed(0)
    disp = (torch.rand(BATCH, H, W, generator=g) * 60).to(dev)
    logvar = (torch.rand(BATCH, H, W, generator=g) * 5 - 4).to(dev)
    gt = torch.randint(0, 255, (BATCH, Hs, Ws, 3), dtype=torch.uint8, generator=g)
    gt[..., 0] = 0
    gt = gt.to(dev)
    px = BATCH * Hs * Ws
    rgb = torch.zeros(px * 3 + 16, dtype=torch.uint8, device=dev)
    sig = torch.zeros(px * 3 + 16, dtype=torch.uint8, device=dev)
    up = torch.zeros(px + 16, device=dev)
    rows = torch.zeros(BATCH, 8, dtype=torch.float64, device=dev)
    work = torch.zeros(L.call("sd_disp_export_ws_bytes", BATCH, Hs, Ws) // 8, dtype=torch.float64, device=dev)
    s = L.stream_handle(dev)

    def export(off, full=True):
        L.call("sd_disp_export", disp.data_ptr(), logvar.data_ptr() if full else None, BATCH, H, W, gt.data_ptr(), Hs, Ws,
               rgb.data_ptr() + off, sig.data_ptr() if full else None, up.data_ptr() if full else None, rows.data_ptr(),
               work.data_ptr(), s)

    def timed(fn, launches=100):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches * 1e3

    src = 2 * BATCH * H * W * 4
    full_bytes = src + px * 3 + px * (3 + 3 + 4)  # maps and ground truth read; two images and disp_up written
    tool_bytes = src // 2 + px * 3 + px * 3  # what the tool asks for without sigma: disp, gt -> disp_rgb, rows
    out = {"source_hw": [Hs, Ws], "bytes_all_outputs": full_bytes, "bytes_tool": tool_bytes}
    for name, fn, nbytes in (("four_pixel_us", lambda: export(0), full_bytes), ("per_pixel_us", lambda: export(1), full_bytes),
                             ("tool_four_pixel_us", lambda: export(0, False), tool_bytes)):
        us = timed(fn)
        out[name] = us
        out[name.replace("_us", "_hbm_share")] = nbytes / (us * 1e-6) / HBM_PEAK
    export(0)
    four, rows4 = rgb[:px * 3].clone(), rows.clone()
    export(1)
    torch.cuda.synchronize()
    out["paths_equal"] = bool(torch.equal(four, rgb[1:px * 3 + 1]) and torch.equal(rows4, rows))
    return out


ARMS = {"a": arm_a, "b": arm_b, "c": arm_c, "stages": arm_stages, "write": arm_write, "kernel": arm_kernel}


# ------------------------------------------------------------------------------------------------- parent
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", type=str, default="bf16", choices=("fp32", "bf16", "fp8"))
    ap.add_argument("--arms", type=str, default="a,b,c,stages,write,kernel")
    ap.add_argument("--dataset-root", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", nargs=3, metavar=("ARM", "ROOT", "SCRATCH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        arm, root, scratch = a.child
        res = ARMS[arm](Path(root), Path(scratch), a.precision)
        print("RESULT " + json.dumps(res), flush=True)
        return

    size, found = real_frame_size((a.dataset_root,) + DEFAULT_ROOTS)
    out = {"pairs": a.pairs, "model_hw": [H, W], "batch": BATCH, "host_threads": THREADS, "precision": a.precision,
           "source_hw": list(size or ASSUMED_SIZE),
           "source_hw_from": found or "ASSUMED (no dataset on this machine)", "rounds": {}}
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        root = Path(tmp) / "data"
        t0 = time.perf_counter()
        write_tree(root, a.pairs, *out["source_hw"])
        out["tree_write_s"] = round(time.perf_counter() - t0, 1)
        print(f"tree: {out}", file=sys.stderr, flush=True)
        ok = True
        for rnd in range(a.rounds):
            for arm in a.arms.split(","):
                scratch = Path(tmp) / f"{arm}_{rnd}"
                cmd = ["timeout", "-k", "10", str(LIMITS[arm]), sys.executable, str(Path(__file__).resolve()),
                       "--precision", a.precision, "--child", arm, str(root), str(scratch)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    out["failed"] = {"arm": arm, "round": rnd, "returncode": p.returncode, "stderr": p.stderr[-2000:]}
                    ok = False
                    break
                out["rounds"].setdefault(arm, []).append(json.loads(lines[-1][7:]))
                print(f"round {rnd} {arm}: {out['rounds'][arm][-1]}", file=sys.stderr, flush=True)
                subprocess.run(["rm", "-rf", str(scratch)])
            if not ok:
                break  # nothing more is started on the GPU after a child that failed or overran
    summary = {}
    for arm, runs in out["rounds"].items():
        for k in runs[0]:
            if k.endswith(("pairs_s", "ms_per_batch", "ms_per_file", "bytes_per_file", "_us", "_hbm_share")):
                v = [r[k] for r in runs]
                summary[f"{arm}_{k}"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                         "max": round(max(v), 4)}
    out["summary"] = summary
    print(json.dumps(out), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
