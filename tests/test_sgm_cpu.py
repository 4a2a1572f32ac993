"""The NumPy restatement of the semi-global matcher (tests/sgm_ref.py) against ground truth, and the host logic of
sgm.py. No GPU: the device tests (test_gpu_sgm.py) compare against the restatement, so it has to mean something.

The bound |q - 16 d0| <= 8 on a scene of constant integer disparity d0 follows from the sub-pixel formula, not from a
measurement: with den = S- + S+ - 2 S0 >= 1 and |S- - S+| <= S- + S+ - 2 S0 (S0 is the minimum), the offset
((S- - S+) * 16 + den) / (2 den) lies in [-7, 8].
"""

import ctypes

import numpy as np
import pytest

import sgm_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import live, sgm

H, W, D, BS = 24, 96, 32, 7


# ---------------------------------------------------------------------- ground truth
@pytest.mark.parametrize("d0,minD", [(0, 0), (5, 0), (17, 0), (9, 4)])
def test_shifted_texture_is_recovered_everywhere(d0, minD):
    left, right = R.shifted_scene(np.random.default_rng(d0), H, W, d0)
    p = R.Params(min_disparity=minD, num_disparities=D, block_size=BS)
    q = R.compute(left, right, p).astype(int)
    region = q[:, p.maxD:W - BS]
    assert region.size > 0 and (region != p.invalid).all()
    assert np.abs(region - 16 * d0).max() <= 8


def test_two_planes_are_recovered_away_from_the_seam():
    rng = np.random.default_rng(3)
    Hh = 40
    left = rng.integers(0, 256, (Hh, W), dtype=np.uint8)
    right = rng.integers(0, 256, (Hh, W), dtype=np.uint8)
    seam = Hh // 2
    right[:seam, :W - 4] = left[:seam, 4:]
    right[seam:, :W - 12] = left[seam:, 12:]
    p = R.Params(num_disparities=D, block_size=BS)
    q = R.compute(left, right, p).astype(int)
    top, bottom = q[:seam - BS - 1, p.maxD:W - BS], q[seam + BS + 1:, p.maxD:W - BS]
    assert (top != p.invalid).all() and np.abs(top - 16 * 4).max() <= 8
    assert (bottom != p.invalid).all() and np.abs(bottom - 16 * 12).max() <= 8


def test_band_and_left_right_check():
    """Background at d = 2, a foreground square at d = 10. In the left view the 8 columns left of the square show
    background that the right view does not see (fresh texture): whatever the matcher assigns there points at right
    pixels that a better match already claimed, and the left-right check removes it."""
    rng = np.random.default_rng(8)
    Hh, Ww, bg, fg = 48, 128, 2, 10
    right = rng.integers(0, 256, (Hh, Ww), dtype=np.uint8)
    y0, y1, x0, x1 = 10, 38, 70, 100
    disp = np.full((Hh, Ww), bg)
    disp[y0:y1, x0:x1] = fg
    xs = np.clip(np.arange(Ww)[None, :] - disp, 0, Ww - 1)
    left = right[np.arange(Hh)[:, None], xs]
    left[y0:y1, x0 - (fg - bg):x0] = rng.integers(0, 256, (y1 - y0, fg - bg), dtype=np.uint8)
    p = R.Params(num_disparities=D, block_size=BS, speckle_window_size=0)
    st = R.compute_stages(left, right, p)
    assert (st["q"][:, :p.maxD] == p.invalid).all() and (st["q_raw"][:, :p.maxD] == p.invalid).all()
    # inside the band, away from its corners; not its last bs // 2 columns, whose block window reaches into the
    # square: they may take the foreground's disparity consistently (foreground fattening) and pass the check
    band = (slice(y0 + BS, y1 - BS), slice(x0 - (fg - bg) + 1, x0 - BS // 2))
    assert (st["q_lr"][band] == p.invalid).all()
    assert (st["q_raw"][band] != p.invalid).any()  # it is the left-right check that removed them
    inside = st["q_lr"][y0 + BS:y1 - BS, x0 + BS:x1 - BS].astype(int)
    assert (inside != p.invalid).all() and np.abs(inside - 16 * fg).max() <= 8
    outside = st["q_lr"][:, p.maxD:x0 - (fg - bg) - BS].astype(int)
    assert (outside != p.invalid).all() and np.abs(outside - 16 * bg).max() <= 8


# ---------------------------------------------------------------------- speckle filter
def test_speckle_exact_size_difference_and_diagonal():
    inv, window, rng_range = -16, 12, 2
    q = np.full((20, 30), inv, dtype=np.int16)
    q[1, 1:13] = 100                 # exactly `window` pixels: removed
    q[3, 1:14] = 200                 # window + 1: kept
    q[5, 1:8] = 300
    q[6, 1:8] = 300 + 16 * rng_range      # differs by exactly 16 * range: joined, 14 pixels, kept
    q[8, 1:8] = 500
    q[9, 1:8] = 500 + 16 * rng_range + 1  # one more: split, 7 pixels each, removed
    q[11:14, 1:4] = 700              # two 3 x 3 squares touching at a corner: 9 pixels each, removed
    q[14:17, 4:7] = 700
    out = R.speckle(q, inv, window, rng_range)
    for val, kept in ((100, False), (200, True), (300, True), (332, True), (500, False), (533, False), (700, False)):
        assert ((out[q == val] == val).all() if kept else (out[q == val] == inv).all()), val
    assert np.array_equal(R.speckle(q, inv, 0, rng_range), q)
    q2 = q.copy()
    q2[14, 3] = 700                  # a 4-neighbour bridge joins the squares: 19 pixels, kept
    assert (R.speckle(q2, inv, window, rng_range)[q2 == 700] == 700).all()


@pytest.mark.parametrize("Hs,Ws,window", [(31, 45, 30), (70, 130, 100)])
def test_crafted_speckle_maps_hold_what_they_claim(Hs, Ws, window):
    q = R.crafted_speckle_map(Hs, Ws, -16, window, 2)
    out = R.speckle(q, -16, window, 2)
    assert (q == 160).sum() > window and (out[q == 160] == 160).all()      # the snake
    assert (q == 400).sum() == window and (out[q == 400] == -16).all()
    assert (q == 800).sum() == window + 1 and (out[q == 800] == 800).all()
    assert (out[q == 1000] == 1000).all() and (out[q == 1032] == 1032).all()
    assert (out[q == 2000] == -16).all() and (out[q == 2033] == -16).all()
    assert (q == 3000).sum() > window and (out[q == 3000] == -16).all()    # the diagonal touch does not join
    assert (q >= 5000).sum() > 200 and (out[q >= 5000] >= 5000).all()


# ---------------------------------------------------------------------- post stage of the restatement
def test_post_statement():
    q = np.array([[-16, 0, 16, 40], [800, 8, -16, 160]], dtype=np.int16)
    Q = np.array([[1, 0, 0, -2.0], [0, 1, 0, -1.0], [0, 0, 0, 500.0], [0, 0, 10.0, 0]])
    disp, z, code = R.post(q, Q)
    assert np.isnan(disp[0, 0]) and np.isnan(disp[0, 1]) and disp[0, 2] == 1.0 and disp[1, 0] == 50.0
    assert z[0, 2] == np.float32(50.0) and np.isnan(z[0, 0]) and z[1, 0] == np.float32(1.0)
    assert code[1, 0] == 255 and code[0, 0] == 0 and code[0, 3] == int(2.5 * 255 / 50)
    assert R.center_distance(z, 15) == np.nanmedian(z)
    assert np.isnan(R.center_distance(np.full((4, 4), np.nan, dtype=np.float32), 3))


# ---------------------------------------------------------------------- host logic of sgm.py
def test_parameter_validation():
    with pytest.raises(ValueError, match="--num-disparities must be a multiple of 16."):
        sgm.StereoSGM(num_disparities=100)
    for bs in (4, 1):
        with pytest.raises(ValueError, match="--block-size must be odd and >= 3."):
            sgm.StereoSGM(block_size=bs)
    for kw in (dict(num_disparities=0), dict(num_disparities=272), dict(block_size=13), dict(min_disparity=-1),
               dict(pre_filter_cap=0), dict(P1=10, P2=5), dict(uniqueness_ratio=101), dict(speckle_window_size=-1)):
        with pytest.raises(ValueError):
            sgm.StereoSGM(**kw)
    m = sgm.StereoSGM()
    assert m.params() == (0, 128, 7, 8 * 49, 32 * 49, 1, 10, 100, 2, 31) and m.invalid_value == -16
    assert sgm.StereoSGM(min_disparity=4, num_disparities=16, block_size=3).invalid_value == 48


def test_overflow_bound_is_rejected_not_clamped():
    # 3 * (bs^2 * (2 * cap + 63) + P2) <= 65535
    sgm.StereoSGM(block_size=11)  # 3 * (121 * 125 + 3872) = 56991
    p2_max = 65535 // 3 - 121 * 125
    sgm.StereoSGM(block_size=11, P2=p2_max)
    with pytest.raises(ValueError, match="exceeds 65535"):
        sgm.StereoSGM(block_size=11, P2=p2_max + 1)
    with pytest.raises(ValueError, match="exceeds 65535"):
        sgm.StereoSGM(block_size=11, pre_filter_cap=63)
    # the library refuses the same parameters before any launch
    with pytest.raises(L.StereoHipError, match="exceeds 65535"):
        L.call("sd_sgm_compute", 256, 256, 8, 64, 0, 16, 11, 968, p2_max + 1, 1, 10, 100, 2, 31, 256, 256, None)
    with pytest.raises(L.StereoHipError, match="multiple of 16"):
        L.call("sd_sgm_compute", 256, 256, 8, 64, 0, 20, 7, 392, 1568, 1, 10, 100, 2, 31, 256, 256, None)
    with pytest.raises(L.StereoHipError, match="block_size"):
        L.call("sd_sgm_cost", 256, 256, 256, 256, 8, 64, 0, 16, 13, 256, 512, None)
    with pytest.raises(L.StereoHipError, match="min_disparity"):
        L.call("sd_sgm_aggregate", 256, 8, 64, -1, 16, 8, 32, 0, 256, None)
    with pytest.raises(L.StereoHipError, match="pass"):
        L.call("sd_sgm_aggregate", 256, 8, 64, 0, 16, 8, 32, 2, 256, None)
    with pytest.raises(L.StereoHipError, match="null pointer"):
        L.call("sd_sgm_winner", 256, 256, 8, 64, 0, 16, 8, 32, 10, 1, None, None, None, None)


def test_reprojection_matrix_handling(golden_dir):
    with np.load(golden_dir / "sgm_calib.npz") as d:
        Q = d["Q"]
    rows = sgm.reprojection_rows(Q.astype(np.float32))
    assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.shape == (4, 4)
    assert np.array_equal(rows, Q.astype(np.float32).astype(np.float64))
    assert sgm.reprojection_rows(Q)[2, 3] == Q[2, 3] and sgm.reprojection_rows(Q)[3, 2] == Q[3, 2]
    assert sgm.reprojection_rows(np.asfortranarray(Q)).flags.c_contiguous
    for bad in (Q[:3], np.zeros((4, 4)), np.where(np.eye(4) > 0, np.nan, Q)):
        with pytest.raises(ValueError):
            sgm.reprojection_rows(bad)
    with pytest.raises(ValueError, match="reprojection matrix Q"):
        sgm.ClassicDepth()
    with pytest.raises(ValueError, match="center_window"):
        sgm.ClassicDepth(Q=Q, center_window=64)
    with pytest.raises(ValueError, match="--block-size"):
        sgm.ClassicDepth(Q=Q, block_size=6)
    c = sgm.ClassicDepth(Q=Q, num_disparities=64, colormap="inferno")  # no device touched before the first step
    assert c.matcher.num_disparities == 64 and c.center_window == 15


def test_classic_depth_is_the_one_stream_batch(golden_dir, monkeypatch):
    with np.load(golden_dir / "sgm_calib.npz") as d:
        Q = d["Q"]

    def no_device(*a, **kw):
        raise AssertionError("the constructor touched the device")

    for name in ("empty", "zeros", "full", "as_tensor"):
        monkeypatch.setattr(sgm.torch, name, no_device)
    monkeypatch.setattr(sgm.torch.cuda, "current_device", no_device)
    monkeypatch.setattr(L, "call", no_device)
    for bad in (np.stack([Q]), np.stack([Q] * 2)):  # a batch's [n, 4, 4] is not a single rig's matrix
        with pytest.raises(ValueError, match="Q must be the 4 x 4"):
            sgm.ClassicDepth(Q=bad)
    z1, z2 = np.zeros((48, 64, 2), np.int16), np.zeros((48, 64), np.uint16)
    rect = live.Rectification(z1, z2, z1, z2, (64, 48), 500.0, 0.07)
    c = sgm.ClassicDepth(rectification=rect, Q=Q.astype(np.float32), center_window=9, mode="hh")
    assert c.Q.shape == (4, 4) and c.Q.dtype == np.float64 and np.array_equal(c.Q, Q.astype(np.float32))
    assert c.rectification is rect and c.center_window == 9 and c.matcher.mode == "hh"
    assert c.device == sgm.torch.device("cuda") and c.device.index is None  # resolved by the first step
    assert isinstance(c._batch, sgm.ClassicDepthBatch) and c._batch.streams == 1 and c.matcher is c._batch.matcher
    assert sgm.ClassicBatchResult is sgm.ClassicResult
    with pytest.raises(RuntimeError, match="before the first step"):
        c._readout()


def test_workspace_bytes_match_the_formula():
    lib = L.load()  # loads without a GPU
    assert lib.sd_version() >= 101

    def a(v):
        return (v + 255) // 256 * 256

    for Hh, Ww, Dd in ((480, 640, 128), (9, 40, 16), (33, 201, 48), (1, 1, 256)):
        want = 2 * a(2 * Hh * Ww * Dd) + 2 * a(Hh * Ww) + 2 * a(4 * Hh * Ww)
        assert L.call("sd_sgm_ws_bytes", Hh, Ww, Dd) == want == sgm.ws_bytes(Hh, Ww, Dd)
        assert L.call("sd_sgm_speckle_ws_bytes", Hh, Ww) == 2 * a(4 * Hh * Ww)
    assert 2 * 480 * 640 * 128 == 78643200  # each volume of the app's frame: ~79 MB
    assert isinstance(ctypes.c_longlong(L.call("sd_sgm_ws_bytes", 8192, 4096, 256)).value, int)
    assert L.call("sd_sgm_ws_bytes", 8192, 4096, 256) > 2 ** 33  # no 32-bit overflow
