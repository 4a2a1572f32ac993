"""The native PNG writer, no GPU: csrc/cache_io.cpp sd_write_png_batch and dataset.write_png_batch.

* files of four sizes at zlib levels 0, 1, 6 and 9 are read back to the written bytes by PIL, by sd_read_png_batch and
  sized by sd_png_size; the file is an 8-bit RGB, non-interlaced PNG with filter type 0 on every row, one IDAT chunk
  and correct CRCs;
* a failing path is reported by index + 1 and by name, leaves no temporary file, and the other files are written; a
  target that exists is replaced whole;
* cache_io.cpp alone, built with AddressSanitizer and UBSan into a stand-alone program
  (tests/png_write_check_main.cpp), repeats the round trip and the failure cases in a child process.
"""

from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import dataset as D

REPO = Path(__file__).resolve().parents[1]


def _images(n, H, W, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    img[0, 0, 0] = (0, 0, 0)
    img[-1, -1, -1] = (255, 255, 255)
    if n > 1:  # a smooth image, the kind a disparity file is: high bytes constant, low bytes running
        c = np.arange(H * W, dtype=np.int64).reshape(H, W) * 37
        img[1] = np.stack([c // 65025 % 256, c // 255 % 255, c % 255], axis=-1).astype(np.uint8)
    return img


def _raw_write(paths, H, W, img, level=1, threads=4):
    arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(str(p)) for p in paths])
    err = ctypes.create_string_buffer(1024)
    rc = L.load().sd_write_png_batch(ctypes.cast(arr, ctypes.c_void_p), len(paths), H, W, img.ctypes.data, level,
                                     threads, err, len(err))
    return rc, err.value.decode()


def _all_files(root: Path):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


def _chunks(data: bytes):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert int.from_bytes(data[pos + 8 + n:pos + 12 + n], "big") == zlib.crc32(kind + body), kind
        out.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    return out


@pytest.mark.parametrize("hw", [(1, 1), (17, 23), (45, 61), (64, 256)])
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_round_trip(tmp_path, hw, level):
    H, W = hw
    n = 3
    img = _images(n, H, W, seed=H * 10 + level)
    paths = [tmp_path / f"{i:03d}.png" for i in range(n)]
    D.write_png_batch(paths, (H, W), torch.from_numpy(img), level, threads=4)
    assert _all_files(tmp_path) == [p.name for p in paths]  # the files and nothing else (no temporary left)
    for i, p in enumerate(paths):
        with Image.open(p) as im:
            assert im.mode == "RGB" and im.size == (W, H)
            assert np.array_equal(np.array(im), img[i])
        assert D.png_size(p) == (H, W)
        chunks = _chunks(p.read_bytes())
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert chunks[0][1] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
        raw = zlib.decompress(chunks[1][1])  # one complete zlib stream
        assert len(raw) == H * (1 + 3 * W)
        rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + 3 * W)
        assert (rows[:, 0] == 0).all()  # filter type 0 on every row
        assert np.array_equal(rows[:, 1:].reshape(H, W, 3), img[i])
    back = torch.full((n, H, W, 3), 0xEE, dtype=torch.uint8)
    assert D.read_png_batch(paths, (H, W), back, threads=3)
    assert np.array_equal(back.numpy(), img)


def test_higher_levels_do_not_grow_a_smooth_image(tmp_path):
    H, W = 64, 256
    img = _images(2, H, W, seed=1)[1:]
    sizes = {}
    for level in (0, 1, 6):
        D.write_png_batch([tmp_path / f"l{level}.png"], (H, W), torch.from_numpy(img), level)
        sizes[level] = (tmp_path / f"l{level}.png").stat().st_size
    assert sizes[0] > H * W * 3 and sizes[1] < sizes[0] and sizes[6] <= sizes[1]


def test_failure_reports_first_bad_path_and_leaves_no_debris(tmp_path):
    H, W = 7, 5
    img = _images(4, H, W, seed=9)
    good = tmp_path / "good"
    good.mkdir()
    paths = [good / "0.png", good / "1.png", tmp_path / "missing" / "2.png", good / "3.png"]  # 2: no such directory
    rc, err = _raw_write(paths, H, W, img)
    assert rc == 3
    assert str(paths[2]) in err
    assert _all_files(tmp_path) == ["good/0.png", "good/1.png", "good/3.png"]  # the others written, no temporary
    for i in (0, 1, 3):
        assert np.array_equal(D.read_rgb_uint8(paths[i]), img[i])
    with pytest.raises(OSError, match="missing"):
        D.write_png_batch(paths, (H, W), torch.from_numpy(img))
    # a target whose temporary name would be too long for the file system keeps its earlier bytes
    old = good / ("x" * 246 + ".png")
    old.write_bytes(b"an earlier file")
    rc, err = _raw_write([good / "0.png", old, good / "3.png"], H, W, img, level=6)
    assert rc == 2 and old.name in err
    assert old.read_bytes() == b"an earlier file"
    assert _all_files(tmp_path) == sorted(["good/0.png", "good/1.png", "good/3.png", f"good/{old.name}"])
    # several failures: the lowest index is the one reported
    rc, err = _raw_write([tmp_path / "missing" / "a.png", good / "0.png", tmp_path / "missing" / "b.png"], H, W, img)
    assert rc == 1 and "a.png" in err
    # a target that exists is replaced whole
    (good / "0.png").write_bytes(b"x" * 100_000)
    D.write_png_batch([good / "0.png"], (H, W), torch.from_numpy(img[3:]))
    assert np.array_equal(D.read_rgb_uint8(good / "0.png"), img[3])
    assert (good / "0.png").stat().st_size < 1000
    # bad arguments
    lib = L.load()
    assert lib.sd_write_png_batch(None, 1, H, W, img.ctypes.data, 1, 1, None, 0) == -1
    for level in (-1, 10):
        rc, err = _raw_write([good / "never.png"], H, W, img, level=level)
        assert rc == -1 and "bad args" in err
    assert not (good / "never.png").exists()
    with pytest.raises(ValueError, match="contiguous CPU uint8"):
        D.write_png_batch([good / "never.png"], (H, W), torch.from_numpy(img))  # four images, one path
    with pytest.raises(ValueError, match="level"):
        D.write_png_batch([good / "never.png"], (H, W), torch.from_numpy(img[:1]), level=12)


def test_writer_under_address_and_ub_sanitizers(tmp_path):
    """cache_io.cpp and a main of its own, compiled with the system C++ compiler and -fsanitize=address,undefined into
    one program, run as a child process: round trips through sd_read_png_batch and sd_png_size at every level, and the
    failure cases. A host build run on its own; nothing is loaded into this process."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    prog = tmp_path / "png_write_check"
    # the sanitizer runtimes linked into the program itself: it then runs the same wherever it is started
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if is_clang else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt, "-pthread",
           f"-I{REPO / 'include'}", str(REPO / "stereo_depth_estimation_amd" / "csrc" / "cache_io.cpp"),
           str(REPO / "tests" / "png_write_check_main.cpp"), "-lz", "-o", str(prog)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    work = tmp_path / "work"
    work.mkdir()
    run = subprocess.run([str(prog), str(work)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "png_write_check: ok" in run.stdout
