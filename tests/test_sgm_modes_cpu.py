"""The NumPy restatement of the matcher's 4-, 5- and 8-path modes (tests/sgm_modes_ref.py) against the three-path
restatement, its own symmetries and ground truth, and the host logic of the `mode` parameter. No GPU: the device tests
(test_gpu_sgm_modes.py) compare against this restatement, so it has to mean something.

The ground-truth bounds are test_sgm_cpu.py's (|q - 16 d0| <= 8 from the sub-pixel formula), unchanged.
"""

import numpy as np
import pytest

import sgm_modes_ref as M
import sgm_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import sgm

NEW_MODES = ("hh4", "sgbm", "hh")
H, W, D, BS = 24, 96, 32, 7


@pytest.fixture(scope="module")
def real_volume():
    """The cost volume of the (17, 150, 48, 3, 5) shifted scene with noise, shared and read-only."""
    p = R.Params(min_disparity=3, num_disparities=48, block_size=5, speckle_window_size=12)
    left, right = R.shifted_bgr_scene(np.random.default_rng(17150), 17, 150, 3 + 48 // 3, noise=12)
    gl, gr = R.gray(left), R.gray(right)
    C = R.cost_volume(gl, gr, R.prefilter(gl, p.cap), R.prefilter(gr, p.cap), p)
    for a in (gl, gr, C):
        a.setflags(write=False)
    return p, gl, gr, C


# ---------------------------------------------------------------------- the restatement against itself
def test_three_way_is_the_three_path_restatement(real_volume):
    p, gl, gr, C = real_volume
    assert np.array_equal(M.aggregate(C, p, "3way"), R.aggregate(C, p))
    assert np.array_equal(M.compute(gl, gr, p, "3way"), R.compute(gl, gr, p))
    assert C[:, p.maxD:].any()


def test_vertical_flip_closure(real_volume):
    """hh and hh4 hold the vertical mirror image of every path they hold; sgbm has the downward diagonals only."""
    p, _, _, C = real_volume
    flipped = np.ascontiguousarray(C[::-1])
    for mode in ("hh", "hh4"):
        assert np.array_equal(M.aggregate(flipped, p, mode)[::-1], M.aggregate(C, p, mode))
    assert not np.array_equal(M.aggregate(flipped, p, "sgbm")[::-1], M.aggregate(C, p, "sgbm"))


def test_the_modes_differ_by_the_paths_they_add(real_volume):
    p, _, _, C = real_volume
    S3 = M.aggregate(C, p, "3way").astype(np.int64)
    flipped = np.ascontiguousarray(C[::-1])
    up = M.path(flipped, p, 1, 0)[::-1]  # bottom -> up is top -> down of the flipped volume
    assert np.array_equal(M.aggregate(C, p, "hh4").astype(np.int64) - S3, up)
    assert np.array_equal(M.path(C, p, -1, 0), up)
    diag = M.path(C, p, 1, 1) + M.path(C, p, 1, -1)
    assert np.array_equal(M.aggregate(C, p, "sgbm").astype(np.int64) - S3, diag)
    assert diag.any() and not np.array_equal(M.path(C, p, 1, 1), M.path(C, p, 1, -1))
    # a diagonal's first row and first column start paths: L = C there
    Cv = C[:, p.maxD:].astype(np.int64)
    L = M.path(C, p, 1, 1)[:, p.maxD:]
    assert np.array_equal(L[0], Cv[0]) and np.array_equal(L[:, 0], Cv[:, 0]) and not np.array_equal(L[1:, 1:], Cv[1:, 1:])
    assert [M.npaths(m) for m in ("3way", "hh4", "sgbm", "hh")] == [3, 4, 5, 8]
    assert len(set(M.MODES["hh"][1])) == 8 and (0, 0) not in M.MODES["hh"][1]


# ---------------------------------------------------------------------- ground truth
@pytest.mark.parametrize("mode", NEW_MODES)
@pytest.mark.parametrize("d0,minD", [(0, 0), (5, 0), (17, 0), (9, 4)])
def test_shifted_texture_is_recovered_everywhere(d0, minD, mode):
    left, right = R.shifted_scene(np.random.default_rng(d0), H, W, d0)
    p = R.Params(min_disparity=minD, num_disparities=D, block_size=BS)
    q = M.compute(left, right, p, mode).astype(int)
    region = q[:, p.maxD:W - BS]
    assert region.size > 0 and (region != p.invalid).all()
    assert np.abs(region - 16 * d0).max() <= 8


@pytest.mark.parametrize("mode", NEW_MODES)
def test_two_planes_are_recovered_away_from_the_seam(mode):
    rng = np.random.default_rng(3)
    Hh = 40
    left = rng.integers(0, 256, (Hh, W), dtype=np.uint8)
    right = rng.integers(0, 256, (Hh, W), dtype=np.uint8)
    seam = Hh // 2
    right[:seam, :W - 4] = left[:seam, 4:]
    right[seam:, :W - 12] = left[seam:, 12:]
    p = R.Params(num_disparities=D, block_size=BS)
    q = M.compute(left, right, p, mode).astype(int)
    top, bottom = q[:seam - BS - 1, p.maxD:W - BS], q[seam + BS + 1:, p.maxD:W - BS]
    assert (top != p.invalid).all() and np.abs(top - 16 * 4).max() <= 8
    assert (bottom != p.invalid).all() and np.abs(bottom - 16 * 12).max() <= 8


def _noisy_square(seed):
    rng = np.random.default_rng(seed)
    right = rng.integers(0, 256, (48, 128)).astype(np.float64)
    disp = np.full((48, 128), 2)
    disp[10:38, 70:100] = 10
    xs = np.clip(np.arange(128)[None, :] - disp, 0, 127)
    left = right[np.arange(48)[:, None], xs]
    left = left + rng.normal(0, 70, left.shape)
    right = right + rng.normal(0, 70, right.shape)
    return np.clip(left, 0, 255).astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8), disp


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_eight_paths_beat_three_on_a_noisy_scene(seed):
    """Background at d = 2, a foreground square at d = 10, sigma = 70 noise on both views; no left-right check, no
    uniqueness test, no speckle filter, so every pixel right of maxD gets a value. Wrong: |q - 16 d| > 16.
    Counts of the restatement, 3way / hh, seeds 0-3: 998 / 742, 1313 / 955, 1123 / 786, 1157 / 872."""
    left, right, disp = _noisy_square(seed)
    p = R.Params(num_disparities=32, block_size=3, disp12_max_diff=-1, uniqueness_ratio=0, speckle_window_size=0)
    wrong = {}
    for mode in ("3way", "hh"):
        q = M.compute(left, right, p, mode).astype(int)
        wrong[mode] = int((np.abs(q - 16 * disp)[:, p.maxD:] > 16).sum())
    print(f"seed {seed}: wrong pixels 3way {wrong['3way']}, hh {wrong['hh']}")
    assert wrong["hh"] < wrong["3way"]


# ---------------------------------------------------------------------- host logic
def test_mode_parameter_and_its_bound():
    for bad in ("5way", "HH", None, 4, -1, 2.0, True):
        with pytest.raises(ValueError, match="mode"):
            sgm.StereoSGM(mode=bad)
    # cv2: MODE_SGBM 0, MODE_HH 1, MODE_SGBM_3WAY 2, MODE_HH4 3
    for const, name in ((0, "sgbm"), (1, "hh"), (2, "3way"), (3, "hh4")):
        m = sgm.StereoSGM(block_size=7, mode=const)
        assert m.mode == name and m.mode_id == const == M.MODES[name][0]
        assert sgm.StereoSGM(block_size=7, mode=name).mode_id == const
        assert sgm.MODES[name][1] == M.npaths(name)
    assert sgm.StereoSGM().mode == "3way"
    assert (L.SD_SGM_MODE_SGBM, L.SD_SGM_MODE_HH, L.SD_SGM_MODE_3WAY, L.SD_SGM_MODE_HH4) == (0, 1, 2, 3)
    # npaths * (bs^2 * (2 * cap + 63) + P2) <= 65535 with P2 = 32 bs^2, cap = 31: 157 bs^2 npaths
    with pytest.raises(ValueError, match="65535") as e:
        sgm.StereoSGM(block_size=9, mode="hh")  # 8 * 157 * 81 = 101736
    assert "8 * " in str(e.value) and "101736" in str(e.value)
    sgm.StereoSGM(block_size=7, mode="hh")      # 61544
    sgm.StereoSGM(block_size=9, mode="sgbm")    # 63585
    sgm.StereoSGM(block_size=9, mode="hh4")     # 50868
    sgm.StereoSGM(block_size=11)                # 56991
    for mode in ("sgbm", "hh4"):
        with pytest.raises(ValueError, match="65535"):
            sgm.StereoSGM(block_size=11, mode=mode)
    # the keyword reaches ClassicDepth's matcher
    c = sgm.ClassicDepth(Q=np.array([[1, 0, 0, -2.0], [0, 1, 0, -1.0], [0, 0, 0, 500.0], [0, 0, 10.0, 0]]), mode="hh")
    assert c.matcher.mode == "hh" and c.matcher.params() == sgm.StereoSGM().params()


def test_the_library_has_the_mode_entry_points():
    lib = L.load()  # loads without a GPU
    assert lib.sd_version() >= 102
    assert {"sd_sgm_aggregate_dir", "sd_sgm_compute_mode"} <= set(L.exported_symbols())
    # refused before any launch: the per-mode bound, an unknown mode, the right -> left direction
    args = (256, 256, 8, 64, 0, 16, 9, 648, 2592, 1, 10, 100, 2, 31)
    with pytest.raises(L.StereoHipError, match="8 \\* .* exceeds 65535"):
        L.call("sd_sgm_compute_mode", *args, L.SD_SGM_MODE_HH, 256, 256, None)
    with pytest.raises(L.StereoHipError, match="mode 7"):
        L.call("sd_sgm_compute_mode", *args, 7, 256, 256, None)
    with pytest.raises(L.StereoHipError, match="sd_sgm_winner"):
        L.call("sd_sgm_aggregate_dir", 256, 8, 64, 0, 16, 8, 32, 0, -1, 0, 256, None)
    for dy, dx in ((0, 0), (2, 0), (1, 2), (-1, -2)):
        with pytest.raises(L.StereoHipError, match="direction"):
            L.call("sd_sgm_aggregate_dir", 256, 8, 64, 0, 16, 8, 32, dy, dx, 0, 256, None)
    with pytest.raises(L.StereoHipError, match="accumulate"):
        L.call("sd_sgm_aggregate_dir", 256, 8, 64, 0, 16, 8, 32, 1, 1, 2, 256, None)
