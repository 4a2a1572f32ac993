"""Cache-build throughput: the device cache builder (stereo_depth_estimation_amd/cache.py) against the route that
existed before it, one first epoch of `DeviceLoader` over a `cache_root` dataset without `require_cache`
(16 DataLoader workers decode with PIL, the main thread writes every miss with np.savez).

    python tools/cache_bench.py [--pairs 512] [--rounds 3] [--dataset-root DIR] [--out profiles/cache_bench.json]

Synthesises `--pairs` PNG triplets (smooth images plus noise, as tools/loader_bench.py; freshly written, so they are
read from the page cache by every arm) at the real dataset's frame size when a FoundationStereo tree is found under
--dataset-root or the CLI defaults, else at 960x540, which is then an ASSUMPTION about the dataset and is reported as
such. Caches are built at 240x320 with batch 64 and at most 16 host threads / workers.

The parent process never touches the GPU: every arm runs as a child process under its own time limit, and after a
child that fails or overruns nothing more is started. Arms alternate over the rounds (a b stages kernel, a b ...); a
child warms its route up on the first 64 samples, then times one pass over all of them into a fresh cache root:
  a       read-through DeviceLoader pass, num_workers 16                -> pairs/s
  b       build_cache                                                   -> pairs/s
  stages  build_cache's three stages each alone over the same batches   -> ms per batch of 64 and pairs/s:
          decode (PNG files -> pinned frames), device (H2D + sd_stereo_to_cache + D2H, synchronised per batch),
          write (pinned cache bytes -> files)
  kernel  sd_stereo_to_cache alone, device events: its four-pixel and per-pixel forms, sd_stereo_preprocess -> us
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
from PIL import Image

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

H, W, BATCH, THREADS = 240, 320, 64, 16
ASSUMED_SIZE = (540, 960)
DEFAULT_ROOTS = ("/mnt/bulk2/NVidia Foundation Stereo", "/home/geoffrey/Reference/OffTopic/Datasets/FoundationStereo")
LIMITS = {"a": 600, "b": 300, "stages": 300, "kernel": 120}  # seconds per child


def real_frame_size(roots):
    from stereo_depth_estimation_amd.dataset import discover_samples, read_rgb_uint8

    for r in roots:
        if r and Path(r).is_dir():
            samples = discover_samples(r)
            if samples:
                return tuple(read_rgb_uint8(samples[0].left_rgb_path).shape[:2]), str(r)
    return None, None


def write_sample(args):
    root, i, Hs, Ws, per_scene = args
    rng = np.random.default_rng(i)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    data = root / f"scene{i // per_scene:03d}" / "dataset" / "data"
    ph = rng.uniform(0, 6.28, 3)
    base = (127 + 100 * np.sin(xx[..., None] / 17.0 + yy[..., None] / 23.0 + ph)).astype(np.int16)
    left = np.clip(base + rng.integers(-20, 20, (Hs, Ws, 3)), 0, 255).astype(np.uint8)
    right = np.roll(left, -8, axis=1)
    drgb = np.stack([np.zeros((Hs, Ws)), (xx % 256), (yy % 256)], -1).astype(np.uint8)  # any RGB24 code decodes
    stem = f"{i % per_scene:06d}"
    Image.fromarray(left).save(data / "left/rgb" / f"{stem}.png")
    Image.fromarray(right).save(data / "right/rgb" / f"{stem}.png")
    Image.fromarray(drgb).save(data / "left/disparity" / f"{stem}.png")


def write_tree(root: Path, pairs: int, Hs: int, Ws: int, per_scene: int = 64):
    for s in range((pairs + per_scene - 1) // per_scene):
        for d in ("left/rgb", "right/rgb", "left/disparity"):
            (root / f"scene{s:03d}" / "dataset" / "data" / d).mkdir(parents=True, exist_ok=True)
    with ThreadPoolExecutor(THREADS) as ex:  # PIL's encoder releases the GIL
        list(ex.map(write_sample, [(root, i, Hs, Ws, per_scene) for i in range(pairs)]))


# ------------------------------------------------------------------------------------------- children (GPU)
def arm_a(root: Path, scratch: Path) -> dict:
    import torch

    from stereo_depth_estimation_amd import dataset as D

    samples = D.discover_samples(root)

    def one_pass(sm, cache):
        ds = D.FoundationStereoDataset(sm, image_size=(H, W), cache_root=cache)
        for _ in D.DeviceLoader(ds, BATCH, num_workers=THREADS, device="cuda"):
            pass
        torch.cuda.synchronize()

    one_pass(samples[:BATCH], scratch / "warm")
    t0 = time.perf_counter()
    one_pass(samples, scratch / "cache")
    dt = time.perf_counter() - t0
    return {"pairs": len(samples), "seconds": dt, "pairs_s": len(samples) / dt}


def arm_b(root: Path, scratch: Path) -> dict:
    from stereo_depth_estimation_amd.cache import build_cache

    build_cache(root, scratch / "warm", H, W, max_samples=BATCH, batch_size=BATCH, read_threads=THREADS)
    t0 = time.perf_counter()
    meta = build_cache(root, scratch / "cache", H, W, batch_size=BATCH, read_threads=THREADS)
    dt = time.perf_counter() - t0
    return {"pairs": meta["num_written"], "seconds": dt, "pairs_s": meta["num_written"] / dt}


def arm_stages(root: Path, scratch: Path) -> dict:
    import torch

    from stereo_depth_estimation_amd import cache as C
    from stereo_depth_estimation_amd import dataset as D

    samples = D.discover_samples(root)
    batches = C.plan_batches(samples, BATCH)
    pipe = C.CachePipeline((H, W), BATCH, torch.device("cuda"), False, THREADS)
    out = {"batches": len(batches), "pairs": len(samples)}

    def rate(name, seconds):
        out[f"{name}_ms_per_batch"] = 1e3 * seconds / len(batches)
        out[f"{name}_pairs_s"] = len(samples) / seconds

    parts = pipe.decode(0, *batches[0])  # warm-up: buffers pinned, code object loaded, first files written
    (scratch / "warm").mkdir(parents=True)
    pipe.write(0, [scratch / "warm" / f"{i}.npz" for i in range(len(batches[0][1]))], pipe.resize(0, parts))
    t0 = time.perf_counter()
    for hw, sm in batches:
        parts = pipe.decode(0, hw, sm)
    rate("decode", time.perf_counter() - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for hw, sm in batches:  # the last decoded batch again: the same bytes moved and computed per batch
        pipe.resize(0, parts).synchronize()
    rate("device", time.perf_counter() - t0)
    ev = pipe.resize(0, parts)
    (scratch / "cache").mkdir(parents=True)
    n = len(batches[-1][1])
    t0 = time.perf_counter()
    for b in range(len(batches)):
        pipe.write(0, [scratch / "cache" / f"{b}_{i}.npz" for i in range(n)], ev)
    dt = time.perf_counter() - t0
    out["write_ms_per_batch"] = 1e3 * dt / len(batches)
    out["write_pairs_s"] = n * len(batches) / dt
    return out


def arm_kernel(root: Path, scratch: Path) -> dict:
    """sd_stereo_to_cache alone on device-resident random frames, device events over 200 launches: its four-pixel form,
    its per-pixel form (out_left one byte off alignment) and sd_stereo_preprocess for scale; at the tree's source size
    (untagged keys) and at three smaller sources."""
    import torch

    from stereo_depth_estimation_amd import _lib as L
    from stereo_depth_estimation_amd import dataset as D

    L.load()
    tree_hw = tuple(D.read_rgb_uint8(D.discover_samples(root)[0].left_rgb_path).shape[:2])
    out = {}
    for tag, hw in (("", tree_hw), ("src480x640_", (480, 640)), ("src240x320_", (240, 320)), ("src120x160_", (120, 160))):
        for k, v in _kernel_times(torch, L, *hw).items():
            out[tag + k] = v
    out["source_hw"] = list(tree_hw)
    return out


def _kernel_times(torch, L, Hs: int, Ws: int) -> dict:
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    src = [torch.randint(0, 256, (BATCH, Hs, Ws, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(3)]
    n = BATCH * H * W
    ol, orr = (torch.zeros(n * 3 + 16, dtype=torch.uint8, device=dev) for _ in range(2))
    od = torch.zeros(n + 16, dtype=torch.int16, device=dev)
    inp, tgt = torch.empty(BATCH, 6, H, W, device=dev), torch.empty(BATCH, 1, H, W, device=dev)
    val = torch.empty(BATCH, 1, H, W, device=dev, dtype=torch.bool)
    s = L.stream_handle(dev)
    ptrs = [t.data_ptr() for t in src]

    def to_cache(off):
        L.call("sd_stereo_to_cache", *ptrs, BATCH, Hs, Ws, H, W, ol.data_ptr() + off, orr.data_ptr(), od.data_ptr(), s)

    def preprocess():
        L.call("sd_stereo_preprocess", *ptrs, BATCH, Hs, Ws, H, W, inp.data_ptr(), tgt.data_ptr(), val.data_ptr(), s)

    def timed(fn, launches=200):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches * 1e3

    out = {"bytes_source": 3 * BATCH * Hs * Ws * 3, "bytes_written": n * 8}
    for name, fn in (("four_pixel_us", lambda: to_cache(0)), ("per_pixel_us", lambda: to_cache(1)),
                     ("preprocess_us", preprocess)):
        out[name] = timed(fn)
    to_cache(0)
    four = ol[:n * 3].clone()
    to_cache(1)
    torch.cuda.synchronize()
    out["forms_equal"] = bool(torch.equal(four, ol[1:n * 3 + 1]))
    return out


# ------------------------------------------------------------------------------------------------- parent
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dataset-root", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", nargs=3, metavar=("ARM", "ROOT", "SCRATCH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        arm, root, scratch = a.child
        res = {"a": arm_a, "b": arm_b, "stages": arm_stages, "kernel": arm_kernel}[arm](Path(root), Path(scratch))
        print("RESULT " + json.dumps(res), flush=True)
        return

    size, found = real_frame_size((a.dataset_root,) + DEFAULT_ROOTS)
    out = {"pairs": a.pairs, "cache_hw": [H, W], "batch": BATCH, "host_threads": THREADS,
           "source_hw": list(size or ASSUMED_SIZE),
           "source_hw_from": found or "ASSUMED (no dataset on this machine)", "rounds": {}}
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        root = Path(tmp) / "data"
        t0 = time.perf_counter()
        write_tree(root, a.pairs, *out["source_hw"])
        out["tree_write_s"] = round(time.perf_counter() - t0, 1)
        out["tree_bytes"] = sum(p.stat().st_size for p in root.rglob("*.png"))
        print(f"tree: {out}", file=sys.stderr, flush=True)
        ok = True
        for rnd in range(a.rounds):
            for arm in ("a", "b", "stages", "kernel"):
                scratch = Path(tmp) / f"{arm}_{rnd}"
                cmd = ["timeout", "-k", "10", str(LIMITS[arm]), sys.executable, str(Path(__file__).resolve()), "--child",
                       arm, str(root), str(scratch)]
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
            if k.endswith(("pairs_s", "ms_per_batch", "_us")):
                v = [r[k] for r in runs]
                summary[f"{arm}_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                                         "max": round(max(v), 2)}
    out["summary"] = summary
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
