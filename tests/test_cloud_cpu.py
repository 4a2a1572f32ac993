"""The point-cloud stage without a GPU: the host side of csrc/cloud.hip, csrc/ply_io.cpp and
stereo_depth_estimation_amd/cloud.py.

* sd_cloud_ws_bytes' limits, and every argument rule of sd_cloud_build_n rejected before a launch;
* pinhole_Q gives Z = f B / d in fp64; rescale_Q reprojects a resized pixel to its calibration pixel's point (1e-12
  relative) and is the identity for sx = sy = 1;
* the PLY writer: round trips through read_ply at counts 0, 1 and cap, counts above cap clamped, the header byte for byte,
  and the failure cases of the PNG writer's test;
* ply_io.cpp alone, built with AddressSanitizer and UBSan into a stand-alone program
  (tests/ply_write_check_main.cpp), repeats them in a child process;
* the NumPy restatement tests/cloud_ref.py on the prototype input keeps the counts the issue recorded.
"""

from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cloud_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import cloud as C

REPO = Path(__file__).resolve().parents[1]
INF = float("inf")

HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
          b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
          b"end_header\n")


def test_ws_bytes_limits():
    ws = lambda *a: L.call("sd_cloud_ws_bytes", *a)  # noqa: E731
    assert ws(1, 1, 1, 1) == 256  # one tile count, rounded up to 256 bytes
    assert ws(64, 480, 640, 64) == 64 * ws(1, 480, 640, 1)
    T = C.TILE_PIXELS
    assert ws(1, 1, 64 * T, 1) == 256 and ws(1, 1, 64 * T + 1, 1) == 512  # 4 bytes per tile of TILE_PIXELS
    assert ws(1, 1080, 1920, 1) == -(-4 * -(-1080 * 1920 // T) // 256) * 256
    for bad in ((0, 4, 4, 1), (65, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, -4, 4, 1), (1, 4, 4, 0),
                (1, 4, 4, 65), (1, 65536, 32768, 1), (1, 46341, 46341, 1)):
        assert ws(*bad) == -1, bad
    assert ws(1, 65536, 32767, 1) > 0  # H * W = 2^31 - 65536
    assert C.SCAN_WIDTH >= 1 and C.RECORD == R.RECORD and C.RECORD.itemsize == 16


def test_build_rejects_bad_args_without_launch():
    p = 256  # a non-null, aligned address that is never dereferenced
    ok = dict(n=1, disp=p, color=p, bgr=1, H=4, W=4, Q=p, z_min=0.0, z_max=1.0, stride=1, xyz=p, points=p, cap=16,
              count=p, work=p)

    def call(**kw):
        a = {**ok, **kw}
        L.call("sd_cloud_build_n", a["n"], a["disp"], a["color"], a["bgr"], a["H"], a["W"], a["Q"], a["z_min"],
               a["z_max"], a["stride"], a["xyz"], a["points"], a["cap"], a["count"], a["work"], None)

    nan = float("nan")
    for kw, msg in ((dict(n=0), "n = 0"), (dict(n=65), "n = 65"), (dict(disp=None), "null disp"),
                    (dict(Q=None), "null Qdev"), (dict(bgr=2), "color_bgr"), (dict(H=0), "bad sizes"),
                    (dict(W=-3), "bad sizes"), (dict(H=65536, W=32768), "bad sizes"), (dict(z_min=nan), "NaN"),
                    (dict(z_max=nan), "NaN"), (dict(z_min=2.0, z_max=1.0), "z_min 2 > z_max 1"),
                    (dict(z_min=INF, z_max=-INF), "z_min inf > z_max -inf"), (dict(stride=0), "stride 0"),
                    (dict(stride=65), "stride 65"), (dict(xyz=None, points=None), "no output"),
                    (dict(points=p + 8), "points must be 16-B aligned"), (dict(count=None), "points need count"),
                    (dict(cap=0), "cap 0"), (dict(cap=-5), "cap -5"), (dict(work=None), "work buffer"),
                    (dict(work=p + 2), "work buffer")):
        with pytest.raises(L.StereoHipError, match=msg):
            call(**kw)


def test_pinhole_Q_is_f_B_over_d():
    f, B, cx, cy = 523.75, 0.1203, 319.5, 239.5
    Q = C.pinhole_Q(f, B, cx, cy)
    assert Q.dtype == np.float64
    assert np.array_equal(Q, [[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, 1 / B, 0]])
    rng = np.random.default_rng(0)
    for x, y, d in rng.uniform((0, 0, 0.5), (640, 480, 128), (50, 3)):
        X, Y, Z, Wh = Q @ np.array([x, y, d, 1.0])
        assert Z / Wh == f / (d * (1 / B))  # the matrix form: 1 / B, the product and the quotient are each rounded
        # against f B / d: at most 1.5 ulp on either side (three roundings in the matrix form, two in the formula); X
        # and Y add the rounding of x - cx on both sides
        assert abs(Z / Wh - f * B / d) <= 4 * np.spacing(f * B / d)
        assert abs(X / Wh - (x - cx) * B / d) <= 6 * np.spacing(abs((x - cx) * B / d))
        assert abs(Y / Wh - (y - cy) * B / d) <= 6 * np.spacing(abs((y - cy) * B / d))
    for bad in ((0, 0.1), (-1, 0.1), (500, 0), (INF, 0.1)):
        with pytest.raises(ValueError):
            C.pinhole_Q(*bad, 1, 1)


def test_rescale_Q():
    Q = np.load(REPO / "tests" / "golden" / "sgm_calib.npz")["Q"].astype(np.float64)
    assert np.array_equal(C.rescale_Q(Q, 1.0, 1.0), Q)
    rng = np.random.default_rng(1)
    for sx, sy in ((0.5, 0.5), (2.0, 2.0), (1.5, 0.75), (61 / 640, 45 / 480)):
        Qs = C.rescale_Q(Q, sx, sy)
        for xr, yr, dr in rng.uniform((0, 0, 0.5), (640 * sx, 480 * sy, 64 * sx), (40, 3)):
            # the calibration pixel of a resized pixel, on half-pixel centres
            x, y, d = (xr + 0.5) / sx - 0.5, (yr + 0.5) / sy - 0.5, dr / sx
            a = Qs @ np.array([xr, yr, dr, 1.0])
            b = Q @ np.array([x, y, d, 1.0])
            pa, pb = a[:3] / a[3], b[:3] / b[3]
            assert (np.abs(pa - pb) <= 1e-12 * np.abs(pb).max()).all(), (sx, sy, pa, pb)
    with pytest.raises(ValueError):
        C.rescale_Q(Q, 0.0, 1.0)
    with pytest.raises(ValueError):
        C.rescale_Q(np.eye(3), 1.0, 1.0)


def test_reference_keeps_the_recorded_counts():
    """The prototype input of the issue: both branches of every predicate occur."""
    Q = np.load(REPO / "tests" / "golden" / "sgm_calib.npz")["Q"]
    for hw in ((480, 640), (37, 61)):
        d = R.prototype_disparity(*hw)
        xyz, has = R.reproject(d, Q)
        keep = R.kept_mask(xyz, has, (0.3, 10))
        assert 0 < keep.sum() < has.sum() < d.size  # no value / out of range / kept all occur
        z = xyz[..., 2][has]
        assert (z < np.float32(0.3)).any() and (z > np.float32(10)).any()
        rec = R.records(d, Q, None, True, (0.3, 10), 1)
        assert len(rec) == keep.sum() and np.isnan(R.organized(d, Q, (0.3, 10))[~keep]).all()


def test_write_ply_flag_errors_and_geometry(tmp_path):
    """predict's --write-ply flags are checked before a device is touched."""
    from stereo_depth_estimation_amd import predict as P

    calib = REPO / "tests" / "golden" / "sgm_calib.npz"
    for kw, msg in ((dict(write_ply=True, output_root=None, focal_px=500.0, baseline_m=0.1), "needs --output-root"),
                    (dict(write_ply=True), "needs a geometry"), (dict(write_ply=True, focal_px=500.0), "needs a geometry"),
                    (dict(write_ply=True, baseline_m=0.1), "needs a geometry"),
                    (dict(focal_px=500.0, baseline_m=0.1), "only with --write-ply"),
                    (dict(ply_stride=2), "only with --write-ply"), (dict(calibration=calib), "only with --write-ply"),
                    (dict(write_ply=True, calibration=calib, focal_px=500.0, baseline_m=0.1), "not both"),
                    (dict(write_ply=True, focal_px=500.0, baseline_m=0.1, cx=3.0), "both or neither"),
                    (dict(write_ply=True, focal_px=-1.0, baseline_m=0.1), "focal_px"),
                    (dict(write_ply=True, focal_px=500.0, baseline_m=0.1, ply_stride=0), "--ply-stride"),
                    (dict(write_ply=True, focal_px=500.0, baseline_m=0.1, ply_stride=65), "--ply-stride"),
                    (dict(write_ply=True, focal_px=500.0, baseline_m=0.1, ply_min_depth=3, ply_max_depth=2),
                     "--ply-min-depth")):
        with pytest.raises(ValueError, match=msg):
            P.cloud_options(**{"output_root": tmp_path, **kw})
    np.savez(tmp_path / "noq.npz", image_size=np.array([640, 480]))
    with pytest.raises(ValueError, match="keys Q and image_size"):
        P.cloud_options(True, tmp_path, calibration=tmp_path / "noq.npz")
    assert P.cloud_options(False, None) is None
    # the entry point raises the same way, before it looks for a model or a device
    with pytest.raises(ValueError, match="needs a geometry"):
        P.predict_pairs("ck.pt", tmp_path, tmp_path, tmp_path / "out", write_ply=True)
    assert not (tmp_path / "out").exists()
    # an ideal rig: the principal point defaults to the frame centre; a calibration is rescaled to the frame size
    o = P.cloud_options(True, tmp_path, focal_px=500.0, baseline_m=0.1, ply_stride=4, ply_max_depth=10)
    assert (o.stride, o.z_range) == (4, (-INF, 10.0))
    assert np.array_equal(o.matrix(45, 61), C.pinhole_Q(500.0, 0.1, 30.0, 22.0))
    o = P.cloud_options(True, tmp_path, focal_px=500.0, baseline_m=0.1, cx=3.0, cy=4.0)
    assert np.array_equal(o.matrix(45, 61), C.pinhole_Q(500.0, 0.1, 3.0, 4.0))
    o = P.cloud_options(True, tmp_path, calibration=calib)
    Q = np.load(calib)["Q"]
    assert o.image_size == (640, 480) and np.array_equal(o.matrix(480, 640), Q)
    assert np.array_equal(o.matrix(45, 61), C.rescale_Q(Q, 61 / 640, 45 / 480))
    assert hash(o) == hash(P.cloud_options(True, tmp_path, calibration=calib))  # a key of the predictor's buffers
    a = P.build_parser().parse_args(["--checkpoint", "c", "--dataset-root", "d"])
    assert (a.write_ply, a.calibration, a.focal_px, a.baseline_m, a.cx, a.cy, a.ply_stride, a.ply_min_depth,
            a.ply_max_depth) == (False, None, None, None, None, None, 1, None, None)


# ---------------------------------------------------------------------------------------------- the PLY writer
def _records(n, cap, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, cap, 16), dtype=np.uint8)


def _raw_write(paths, pts, counts, threads=4):
    arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(str(p)) for p in paths])
    err = ctypes.create_string_buffer(1024)
    c = np.asarray(counts, dtype=np.uint32)
    rc = L.load().sd_write_ply_batch(ctypes.cast(arr, ctypes.c_void_p), len(paths), pts.ctypes.data, pts.shape[1],
                                     c.ctypes.data, threads, err, len(err))
    return rc, err.value.decode()


def _all_files(root: Path):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


@pytest.mark.parametrize("cap", [1, 2, 37, 5000])
def test_round_trip(tmp_path, cap):
    counts = [0, 1, cap, cap + 7, 2 ** 32 - 1]  # empty, one point, full, above cap twice (clamped)
    n = len(counts)
    pts = _records(n, cap, seed=cap)
    paths = [tmp_path / f"{i}.ply" for i in range(n)]
    C.write_ply_batch(paths, pts, counts, threads=3)
    assert _all_files(tmp_path) == [p.name for p in paths]  # the files and nothing else (no temporary left)
    for i, p in enumerate(paths):
        k = min(counts[i], cap)
        data = p.read_bytes()
        assert data == HEADER % k + pts[i, :k].tobytes()
        assert C.ply_header(k) == HEADER % k
        got = C.read_ply(p)
        assert got.dtype == C.RECORD and got.shape == (k,)
        assert got.tobytes() == pts[i, :k].tobytes()
    # a RECORD array and a torch tensor are taken too
    import torch

    C.write_ply_batch(paths[2:3], pts[2:3].reshape(1, cap * 16).view(C.RECORD), [cap])
    assert paths[2].read_bytes() == HEADER % cap + pts[2].tobytes()
    C.write_ply_batch(paths[2:3], torch.from_numpy(pts[3:4]), [cap])
    assert paths[2].read_bytes() == HEADER % cap + pts[3].tobytes()


def test_read_ply_refuses_other_files(tmp_path):
    p = tmp_path / "a.ply"
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="header"):
        C.read_ply(p)
    p.write_bytes(HEADER % 2 + bytes(16))  # truncated
    with pytest.raises(ValueError, match="2 vertices"):
        C.read_ply(p)
    p.write_bytes(b"not a ply")
    with pytest.raises(ValueError, match="no PLY header"):
        C.read_ply(p)


def test_failure_reports_first_bad_path_and_leaves_no_debris(tmp_path):
    cap = 9
    pts = _records(4, cap, seed=9)
    counts = [3, 9, 4, 0]
    good = tmp_path / "good"
    good.mkdir()
    paths = [good / "0.ply", good / "1.ply", tmp_path / "missing" / "2.ply", good / "3.ply"]  # 2: no such directory
    rc, err = _raw_write(paths, pts, counts)
    assert rc == 3
    assert str(paths[2]) in err
    assert _all_files(tmp_path) == ["good/0.ply", "good/1.ply", "good/3.ply"]  # the others written, no temporary
    for i in (0, 1, 3):
        assert C.read_ply(paths[i]).tobytes() == pts[i, :counts[i]].tobytes()
    assert paths[3].read_bytes() == HEADER % 0  # an empty cloud is a valid file
    with pytest.raises(OSError, match="missing"):
        C.write_ply_batch(paths, pts, counts)
    # a target whose temporary name would be too long for the file system keeps its earlier bytes
    old = good / ("x" * 246 + ".ply")
    old.write_bytes(b"an earlier file")
    rc, err = _raw_write([good / "0.ply", old, good / "3.ply"], pts, counts)
    assert rc == 2 and old.name in err
    assert old.read_bytes() == b"an earlier file"
    assert _all_files(tmp_path) == sorted(["good/0.ply", "good/1.ply", "good/3.ply", f"good/{old.name}"])
    # several failures: the lowest index is the one reported
    rc, err = _raw_write([tmp_path / "missing" / "a.ply", good / "0.ply", tmp_path / "missing" / "b.ply"], pts, counts)
    assert rc == 1 and "a.ply" in err
    # a target that exists is replaced whole
    (good / "0.ply").write_bytes(b"x" * 100_000)
    C.write_ply_batch([good / "0.ply"], pts[3:], [2])
    assert (good / "0.ply").read_bytes() == HEADER % 2 + pts[3, :2].tobytes()
    # bad arguments
    lib = L.load()
    c = np.asarray(counts, dtype=np.uint32)
    assert lib.sd_write_ply_batch(None, 1, pts.ctypes.data, cap, c.ctypes.data, 1, None, 0) == -1
    arr = (ctypes.c_char_p * 1)(os.fsencode(str(good / "never.ply")))
    err = ctypes.create_string_buffer(256)
    for points, cap_, cnt in ((None, cap, c.ctypes.data), (pts.ctypes.data, 0, c.ctypes.data),
                              (pts.ctypes.data, cap, None)):
        assert lib.sd_write_ply_batch(ctypes.cast(arr, ctypes.c_void_p), 1, points, cap_, cnt, 1, err, len(err)) == -1
        assert b"bad args" in err.value
    assert lib.sd_write_ply_batch(ctypes.cast(arr, ctypes.c_void_p), -1, pts.ctypes.data, cap, c.ctypes.data, 1, err,
                                  len(err)) == -1
    assert not (good / "never.ply").exists()
    with pytest.raises(ValueError, match="records"):
        C.write_ply_batch([good / "never.ply"], pts, counts[:1])  # four clouds, one path
    with pytest.raises(ValueError, match="counts"):
        C.write_ply_batch([good / "never.ply"], pts[:1], counts)
    assert not (good / "never.ply").exists()


def test_writer_under_address_and_ub_sanitizers(tmp_path):
    """ply_io.cpp and a main of its own, compiled with the system C++ compiler and -fsanitize=address,undefined into one
    program, run as a child process: the files byte for byte at counts 0, 1, cap and above, and the failure cases. A
    host build run on its own; nothing is loaded into this process."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    prog = tmp_path / "ply_write_check"
    # the sanitizer runtimes linked into the program itself: it then runs the same wherever it is started
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if is_clang else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt, "-pthread",
           f"-I{REPO / 'include'}", str(REPO / "stereo_depth_estimation_amd" / "csrc" / "ply_io.cpp"),
           str(REPO / "tests" / "ply_write_check_main.cpp"), "-o", str(prog)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    work = tmp_path / "work"
    work.mkdir()
    run = subprocess.run([str(prog), str(work)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "ply_write_check: ok" in run.stdout
