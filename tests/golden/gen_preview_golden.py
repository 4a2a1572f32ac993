#!/usr/bin/env python3
"""Generate tests/golden/preview.npz: inputs and montages of the reference's own save_preview_montage
(foundation_stereo_depth/eval_utils.py:55-73), for tests/test_preview_cpu.py and tests/test_gpu_preview.py.

Usage (CPU only, from the repository root):  python tests/golden/gen_preview_golden.py <reference>/src

The reference package is imported from the given path (as gen_golden.py imports it); its function writes each montage as
a PNG, which is read back with PIL. Only data (inputs and recorded results) is written.

Samples: 24x40 x 3, 5x7 x 1, 33x50 x 1. Inputs in [0, 1] with a few values at -0.1 and 1.2, exact k / 255 grid points
and their lower float32 neighbours (truncation cases: the neighbour's product with 255 lands below k); targets with a
block of zeros; predictions with negative values; one map with NaN / +-inf holes and one constant map.

Every stored sample satisfies: the NumPy restatement of the normative text (tests/preview_ref.py) reproduces the
reference's montage byte for byte. np.percentile interpolates in float32 and the statement in fp64, so a sample on
which the two disagree in a code is replaced by the next draw (the draw counter below); none was at the time of writing.
"""

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch
from PIL import Image

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO / "tests"))
sys.dont_write_bytecode = True
OUT = REPO / "tests" / "golden" / "preview.npz"

import preview_ref  # noqa: E402


def _inputs(rng, h, w):
    # multiples of 2^-12 (the file compresses; x * 255 is still inexact in float32), half of them replaced below
    x = (rng.integers(0, 4097, (6, h, w)).astype(np.float32) / np.float32(4096.0))
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, max(8, flat.size // 2), replace=False)
    grid = idx[: idx.size - 6]
    flat[grid] = (rng.integers(0, 256, grid.size).astype(np.float32) / np.float32(255.0))  # exact k / 255
    # float32(k / 255) * 255 is exactly k for every k; the float32 just below it gives a product below k, code k - 1
    below = grid[::3]
    flat[below] = np.nextafter(flat[below], np.float32(-1.0))
    flat[idx[-6:-3]] = np.float32(-0.1)
    flat[idx[-3:]] = np.float32(1.2)
    return x


def _sample(rng, h, w, kind):
    inp = _inputs(rng, h, w)
    tgt = (rng.integers(32, 5760, (h, w)).astype(np.float32) / np.float32(64.0))  # 0.5 .. 90 in steps of 1/64
    tgt[: max(1, h // 3), : max(1, w // 2)] = 0.0  # invalid pixels of a target are zeros
    pred = rng.normal(20.0, 25.0, (h, w)).astype(np.float32)  # softplus output never is, but the rule takes negatives
    if kind == "holes":
        flat = pred.reshape(-1)
        idx = rng.choice(flat.size, flat.size // 10, replace=False)
        flat[idx] = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)[rng.integers(0, 4, idx.size)]
    elif kind == "constant":
        pred[:] = np.float32(3.5)
    return inp, tgt, pred


def _reference_montage(ref_eval, tmp, inp, tgt, pred):
    path = Path(tmp) / "m.png"
    with np.errstate(all="ignore"):
        ref_eval.save_preview_montage(path, torch.from_numpy(inp), torch.from_numpy(tgt[None]), torch.from_numpy(pred[None]))
    return np.asarray(Image.open(path).convert("RGB"))


def main() -> None:
    sys.path.insert(0, sys.argv[1])
    from foundation_stereo_depth import eval_utils as ref_eval

    plan = [("a", 24, 40, "plain"), ("b", 24, 40, "holes"), ("c", 24, 40, "constant"), ("d", 5, 7, "plain"),
            ("e", 33, 50, "plain")]
    out, names = {}, []
    draws = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, h, w, kind in plan:
            for attempt in range(16):
                rng = np.random.default_rng([2026, draws])
                draws += 1
                inp, tgt, pred = _sample(rng, h, w, kind)
                ref = _reference_montage(ref_eval, tmp, inp, tgt, pred)
                if np.array_equal(preview_ref.montage(inp, tgt, pred), ref):
                    break
                print(f"sample {name}: restatement differs from the reference in a code, redrawn")
            else:
                raise SystemExit(f"sample {name}: no draw on which the restatement reproduces the reference")
            assert ref.shape == (h, 4 * w, 3) and ref.dtype == np.uint8
            out[f"{name}/input"], out[f"{name}/target"], out[f"{name}/pred"], out[f"{name}/montage"] = inp, tgt, pred, ref
            names.append(name)
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes", len(names), "samples", draws, "draws")


if __name__ == "__main__":
    main()
