"""The cache builder's host side, no GPU: the native writer (csrc/cache_io.cpp sd_write_cache_batch) and the CLI of
stereo_depth_estimation_amd/cache.py.

* files written stored and deflated are read back bit-equal by np.load, _load_cached_uint8 and sd_read_cache_batch,
  and pass zipfile's CRC check;
* a failing path is reported by index + 1 and by name, leaves no temporary file and no damage to an earlier file;
* cache_io.cpp alone, built with AddressSanitizer and UBSan into a stand-alone program (tests/cache_io_check_main.cpp),
  repeats the round trip and the failure cases in a child process;
* the parser's reference flags and defaults (reference cache.py:18-47), --device cpu, an empty dataset root.
"""

from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
import zipfile
from pathlib import Path

import numpy as np
import pytest
import torch

from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import cache as C
from stereo_depth_estimation_amd import dataset as D

REPO = Path(__file__).resolve().parents[1]

# float16 bit patterns a disparity can take: +-0, the smallest and largest subnormals, the smallest normal, 1.0,
# 2048 (the last power of two with integer spacing 1), values above it, the largest finite value, +inf
SPECIAL_F16 = np.array([0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x6800, 0x6801, 0x7000, 0x7BFF, 0x7C00],
                       dtype=np.uint16)


def _batch(n, H, W, seed):
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    bits = rng.uniform(0, 300, (n, H, W)).astype(np.float16).view(np.uint16)
    flat = bits.reshape(-1)
    flat[rng.choice(flat.size, SPECIAL_F16.size, replace=False)] = SPECIAL_F16
    assert np.isin(SPECIAL_F16, bits).all() and (bits.view(np.float16) > 2048).any()
    return left, right, bits


def _write(paths, H, W, left, right, bits, compress, threads=4):
    D.write_cache_batch(paths, (H, W), torch.from_numpy(left), torch.from_numpy(right),
                        torch.from_numpy(bits.view(np.int16)), compress, threads)


def _raw_write(paths, H, W, left, right, bits, compress=0, threads=4):
    arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(str(p)) for p in paths])
    err = ctypes.create_string_buffer(1024)
    rc = L.load().sd_write_cache_batch(ctypes.cast(arr, ctypes.c_void_p), len(paths), H, W, left.ctypes.data,
                                       right.ctypes.data, bits.ctypes.data, compress, threads, err, len(err))
    return rc, err.value.decode()


def _all_files(root: Path):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


@pytest.mark.parametrize("hw", [(24, 32), (7, 5)])
@pytest.mark.parametrize("compress", [False, True])
def test_writer_round_trip(tmp_path, hw, compress):
    H, W = hw
    n = 5
    left, right, bits = _batch(n, H, W, seed=H + int(compress))
    paths = [tmp_path / f"{i:06d}.npz" for i in range(n)]
    _write(paths, H, W, left, right, bits, compress)
    assert _all_files(tmp_path) == [p.name for p in paths]  # the files and nothing else (no temporary left)
    for i, p in enumerate(paths):
        with np.load(p) as z:
            assert sorted(z.files) == ["disparity", "left", "right"]
            got = z["left"], z["right"], z["disparity"]
        assert [a.dtype for a in got] == [np.uint8, np.uint8, np.float16]
        assert [a.shape for a in got] == [(H, W, 3), (H, W, 3), (H, W)]
        assert np.array_equal(got[0], left[i]) and np.array_equal(got[1], right[i])
        assert np.array_equal(got[2].view(np.uint16), bits[i])
        loaded = D._load_cached_uint8(p, (H, W))
        assert loaded is not None
        assert np.array_equal(loaded[0], left[i]) and np.array_equal(loaded[1], right[i])
        assert loaded[2].dtype == np.float16 and np.array_equal(loaded[2].view(np.uint16), bits[i])
        with zipfile.ZipFile(p) as zf:
            assert zf.testzip() is None
            assert zf.namelist() == ["left.npy", "right.npy", "disparity.npy"]
            want = zipfile.ZIP_DEFLATED if compress else zipfile.ZIP_STORED
            assert all(info.compress_type == want for info in zf.infolist())
    back = (torch.empty(n, H, W, 3, dtype=torch.uint8), torch.empty(n, H, W, 3, dtype=torch.uint8),
            torch.empty(n, H, W, dtype=torch.int16))
    D.read_cache_batch(paths, (H, W), *back, threads=3)
    assert np.array_equal(back[0].numpy(), left) and np.array_equal(back[1].numpy(), right)
    assert np.array_equal(back[2].numpy().view(np.uint16), bits)


def test_npy_headers_are_padded_as_numpy_pads_them(tmp_path):
    # data of every member starts at a multiple of 64 within the member (numpy.lib.format ARRAY_ALIGN), version 1.0
    H, W = 7, 5
    left, right, bits = _batch(1, H, W, seed=1)
    _write([tmp_path / "a.npz"], H, W, left, right, bits, False)
    with zipfile.ZipFile(tmp_path / "a.npz") as zf:
        for name, nbytes in (("left.npy", H * W * 3), ("right.npy", H * W * 3), ("disparity.npy", H * W * 2)):
            raw = zf.read(name)
            assert raw[:8] == b"\x93NUMPY\x01\x00"
            hlen = int.from_bytes(raw[8:10], "little")
            assert (10 + hlen) % 64 == 0 and raw[10 + hlen - 1:10 + hlen] == b"\n"
            assert len(raw) == 10 + hlen + nbytes


def test_compressed_constant_image_is_smaller(tmp_path):
    H, W = 24, 32
    left = np.full((1, H, W, 3), 17, np.uint8)
    bits = np.full((1, H, W), 0x3C00, np.uint16)
    _write([tmp_path / "s.npz"], H, W, left, left, bits, False)
    _write([tmp_path / "c.npz"], H, W, left, left, bits, True)
    assert (tmp_path / "c.npz").stat().st_size < (tmp_path / "s.npz").stat().st_size
    with np.load(tmp_path / "c.npz") as z:
        assert np.array_equal(z["left"], left[0]) and np.array_equal(z["disparity"].view(np.uint16), bits[0])


def test_writer_failure_reports_first_bad_path_and_leaves_no_debris(tmp_path):
    H, W = 7, 5
    n = 4
    left, right, bits = _batch(n, H, W, seed=9)
    good = tmp_path / "good"
    good.mkdir()
    # index 2: its directory does not exist
    paths = [good / "0.npz", good / "1.npz", tmp_path / "missing" / "2.npz", good / "3.npz"]
    rc, err = _raw_write(paths, H, W, left, right, bits)
    assert rc == 3
    assert str(paths[2]) in err
    assert _all_files(tmp_path) == ["good/0.npz", "good/1.npz", "good/3.npz"]  # the others written, no temporary
    with pytest.raises(OSError, match="missing"):
        _write(paths, H, W, left, right, bits, False)
    # a target that exists and whose temporary name (the target's plus a suffix) is longer than a file name may be:
    # the write fails before anything is created, for any user, and the entry keeps its bytes
    old = good / ("x" * 246 + ".npz")
    old.write_bytes(b"an earlier entry")
    paths = [good / "0.npz", old, good / "3.npz"]
    rc, err = _raw_write(paths, H, W, left, right, bits, compress=1)
    assert rc == 2 and old.name in err
    assert old.read_bytes() == b"an earlier entry"
    assert _all_files(tmp_path) == sorted(["good/0.npz", "good/1.npz", "good/3.npz", f"good/{old.name}"])
    # several failures: the lowest index is the one reported
    rc, err = _raw_write([tmp_path / "missing" / "a.npz", good / "0.npz", tmp_path / "missing" / "b.npz"], H, W, left,
                         right, bits)
    assert rc == 1 and "a.npz" in err
    # an overwrite replaces an entry whole
    _write([good / "0.npz"], H, W, left[3:], right[3:], bits[3:], False)
    with np.load(good / "0.npz") as z:
        assert np.array_equal(z["left"], left[3])
    assert L.load().sd_write_cache_batch(None, 1, H, W, left.ctypes.data, right.ctypes.data, bits.ctypes.data, 0, 1,
                                         None, 0) == -1


def test_writer_under_address_and_ub_sanitizers(tmp_path):
    """cache_io.cpp and a main of its own, compiled with the system C++ compiler and -fsanitize=address,undefined into
    one program, run as a child process: the round trip of both shapes, stored and deflated, read back through
    sd_read_cache_batch, and the failure cases. A host build run on its own; nothing is loaded into this process."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    prog = tmp_path / "cache_io_check"
    # the sanitizer runtimes linked into the program itself: it then runs the same wherever it is started
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if is_clang else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt, "-pthread",
           f"-I{REPO / 'include'}", str(REPO / "stereo_depth_estimation_amd" / "csrc" / "cache_io.cpp"),
           str(REPO / "tests" / "cache_io_check_main.cpp"), "-lz", "-o", str(prog)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    work = tmp_path / "work"
    work.mkdir()
    run = subprocess.run([str(prog), str(work)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "cache_io_check: ok" in run.stdout


# the reference's flags and defaults (reference cache.py:18-47), written out
REFERENCE_FLAGS = {
    "dataset_root": "/home/geoffrey/Reference/OffTopic/Datasets/FoundationStereo",
    "height": 240,
    "width": 320,
    "max_samples": 0,
    "overwrite": False,
    "compress": False,
}


def test_cli_flags_and_defaults():
    p = C.build_parser()
    with pytest.raises(SystemExit):
        p.parse_args([])  # --cache-root is required
    a = vars(p.parse_args(["--cache-root", "/tmp/c"]))
    assert a.pop("cache_root") == "/tmp/c"
    for k, v in REFERENCE_FLAGS.items():
        got = a.pop(k)
        assert got == v and type(got) is type(v), k
    assert a == {"batch_size": 64, "read_threads": 16, "device": "cuda"}
    b = p.parse_args(["--dataset-root", "d", "--cache-root", "c", "--height", "24", "--width", "32", "--max-samples",
                      "5", "--overwrite", "--compress", "--batch-size", "3", "--read-threads", "2"])
    assert (b.dataset_root, b.cache_root, b.height, b.width, b.max_samples, b.overwrite, b.compress, b.batch_size,
            b.read_threads) == ("d", "c", 24, 32, 5, True, True, 3, 2)


def test_device_cpu_is_rejected(tmp_path):
    (tmp_path / "data").mkdir()
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.main(["--dataset-root", str(tmp_path / "data"), "--cache-root", str(tmp_path / "cache"), "--device", "cpu"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.build_cache(tmp_path / "data", tmp_path / "cache", device="cpu")
    assert not (tmp_path / "cache").exists()


def test_empty_root_raises_the_references_message(tmp_path):
    root = tmp_path / "data"
    root.mkdir()
    with pytest.raises(ValueError, match="No samples discovered under: ") as e:
        C.build_cache(root, tmp_path / "cache")
    assert str(e.value) == f"No samples discovered under: {root.resolve()}"
