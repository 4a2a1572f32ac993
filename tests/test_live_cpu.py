"""The live frame path's host side (no GPU): rectify_maps, the calibration helpers against the reference's recorded
results (tests/golden/live_post.npz), the colormap table, and the new C-ABI entries' exports and argument validation."""

import ctypes
import math

import numpy as np
import pytest

import live_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import live

P16 = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced: validation fails before any launch


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(golden_dir / "live_post.npz"))


def _K(f=100.0, cx=20.0, cy=15.0):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float64)


def _P(f=100.0, cx=20.0, cy=15.0):
    return np.hstack([_K(f, cx, cy), np.zeros((3, 1))])


def test_rectify_maps_identity_is_the_pixel_grid():
    map1, map2 = live.rectify_maps(_K(), np.zeros(5), np.eye(3), _P(), (40, 30))
    assert map1.shape == (30, 40, 2) and map1.dtype == np.int16 and map2.shape == (30, 40) and map2.dtype == np.uint16
    x, y = np.meshgrid(np.arange(40), np.arange(30))
    assert np.array_equal(map1[..., 0], x) and np.array_equal(map1[..., 1], y)
    assert not map2.any()


def test_rectify_maps_principal_point_shift():
    map1, map2 = live.rectify_maps(_K(cx=22.25), None, None, _P(cx=20.0), (40, 30))
    x, y = np.meshgrid(np.arange(40), np.arange(30))
    assert np.array_equal(map1[..., 0], x + 2) and np.array_equal(map1[..., 1], y)
    assert np.all(map2 == 8)  # fx5 = 0.25 * 32, fy5 = 0


def test_rectify_maps_radial_matches_the_plain_statement():
    dist = np.array([-0.28, 0.07, 0.001, -0.002, 0.01])
    c, s = math.cos(0.02), math.sin(0.02)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    args = (_K(95.0, 19.5, 14.25), dist, rot, _P(90.0, 21.0, 15.5), (40, 30))
    got, want = live.rectify_maps(*args), R.rectify_maps(*args)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(np.unique(got[1])) > 100  # the fractions are exercised
    k1 = (_K(), np.array([0.2]), None, _P(), (40, 30))  # k1 alone
    got, want = live.rectify_maps(*k1), R.rectify_maps(*k1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1].any()


def _same(a, b):
    return (math.isnan(a) and (b is None or math.isnan(b))) or a == b


def test_estimate_baseline_against_the_reference(gold):
    P1, P2, T = gold["calib/P1"], gold["calib/P2"], gold["calib/T"]
    assert live.estimate_baseline_m(P1, P2, T) == float(gold["baseline/p"])
    assert live.estimate_baseline_m(None, None, T) == float(gold["baseline/t"])
    assert live.estimate_baseline_m(None, None, None) is None and math.isnan(float(gold["baseline/none"]))
    assert live.estimate_baseline_m(P1, P1, T) == float(gold["baseline/p_zero_tx"])  # tx = 0: falls back to |T|


def test_load_calibration_against_the_reference(gold, tmp_path):
    full = tmp_path / "full.npz"
    np.savez(full, P1=gold["calib/P1"], P2=gold["calib/P2"], T=gold["calib/T"], image_size=gold["calib/image_size"],
             mtx_l=gold["calib/mtx_l"])
    bare = tmp_path / "bare.npz"
    np.savez(bare, mtx_l=gold["calib/mtx_l"], T=gold["calib/T"])
    for path, key in ((full, "calib/full/geometry"), (bare, "calib/bare/geometry")):
        c = live.load_calibration(path)
        f, b, w = (float(v) for v in gold[key])
        assert _same(f, c.focal_length_px) and _same(b, c.baseline_m) and _same(w, c.calibration_width_px)
        assert c.rectification is None  # no distortion / rotation keys: geometry only
    # with every key the maps are built and define the geometry
    K = gold["calib/mtx_l"]
    allk = tmp_path / "all.npz"
    np.savez(allk, mtx_l=K, dist_l=np.zeros(5), mtx_r=K, dist_r=np.zeros(5), R1=np.eye(3), R2=np.eye(3),
             P1=gold["calib/P1"], P2=gold["calib/P2"], T=gold["calib/T"], image_size=np.array([64, 48]))
    c = live.load_calibration(allk)
    r = c.rectification
    assert r is not None and r.image_size == (64, 48) and r.map_l_1.shape == (48, 64, 2) and r.map_r_2.shape == (48, 64)
    assert c.focal_length_px == float(gold["calib/P1"][0, 0]) and c.calibration_width_px == 64
    assert c.baseline_m == float(gold["baseline/p"])
    assert live.load_calibration(allk, rectify=False).rectification is None


def test_live_ref_post_stage_equals_the_reference(gold):
    """tests/live_ref.py's numpy post stage (the GPU tests' reference off the fixture's shapes, and the host path of
    tools/live_bench.py) reproduces the reference's recorded results."""
    fm, bl = float(gold["focal_model"]), float(gold["baseline"])
    depth = R.depth_from_disparity(gold["disp"], fm, bl)
    assert np.array_equal(depth, gold["depth"], equal_nan=True)
    assert np.array_equal(R.contour_mask(depth, 0.5, 0.0, 10.0), gold["contour"])
    assert np.array_equal(R.contour_mask(gold["invalid"], 0.5, 0.0, 10.0), gold["invalid_contour"])
    assert np.array_equal(R.codes(depth, 0.0, 10.0), gold["depth_code"])
    assert np.array_equal(R.codes(gold["conf"], 0.0, 5.0), gold["conf_code"])
    for name in ("disp", "dup", "one", "two"):
        lo, hi = gold[f"auto/{name}/lohi"]
        assert np.array_equal(R.codes(gold[f"auto/{name}/in"], lo, hi), gold[f"auto/{name}/code"]), name
    assert not gold["auto/invalid/code"].any()
    for name in ("odd", "even", "small", "zero", "clipped", "empty"):
        window, want, _ = gold[f"center/{name}/window_median_count"]
        assert _same(R.center_median(gold[f"center/{name}/in"], int(window)), float(want)), name


def test_depth_is_enabled_as_in_the_reference():
    class M:
        in_channels = 6

    assert live.LiveDepth(M(), (48, 32), focal_length_px=800.0, baseline_m=0.1, calibration_width_px=640).depth_enabled
    ld = live.LiveDepth(M(), (48, 32), focal_length_px=800.0, baseline_m=0.1, calibration_width_px=640)
    assert ld.focal_length_px_model == 800.0 * (48 / 640.0)
    assert not live.LiveDepth(M(), (48, 32), focal_length_px=800.0, baseline_m=0.1).depth_enabled  # no width
    assert not live.LiveDepth(M(), (48, 32), focal_length_px=800.0, calibration_width_px=640).depth_enabled
    assert not live.LiveDepth(M(), (48, 32)).depth_enabled
    with pytest.raises(ValueError, match="center_window"):
        live.LiveDepth(M(), (48, 32), center_window=64)
    with pytest.raises(ValueError, match="ema_alpha"):
        live.LiveDepth(M(), (48, 32), ema_alpha=1.5)


def test_colormap_file():
    assert live.COLORMAP_FILE.suffix == ".json" and live.COLORMAP_FILE.exists()
    luts = live.load_colormaps()
    assert luts.shape == (4, 256, 3) and luts.dtype == np.uint8
    assert live.COLORMAP_NAMES == ("turbo", "inferno", "magma", "viridis")
    # BGR: viridis runs from dark purple (68, 1, 84 in RGB) to yellow (253, 231, 37)
    v = live.colormap_lut("viridis")
    assert tuple(v[0]) == (84, 1, 68) and tuple(v[255]) == (37, 231, 253)
    assert len({luts[i].tobytes() for i in range(4)}) == 4
    with pytest.raises(ValueError):
        live.colormap_lut("jet")


NEW = ("sd_live_frontend", "sd_live_rectify", "sd_live_post", "sd_live_contours", "sd_live_select_ws_bytes",
       "sd_live_select", "sd_live_center", "sd_live_compose")


def test_live_entries_are_exported():
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and name in L.exported_symbols(), name
    assert L.call("sd_live_select_ws_bytes") >= (2048 + 4 * 2048 + 4 * 512) * 4


def test_live_entries_reject_bad_args_without_launch():
    p = P16
    fe = lambda *a: L.call("sd_live_frontend", *a)  # noqa: E731
    with pytest.raises(L.StereoHipError, match="null pointer"):
        fe(L.SD_F32, None, p, 8, 8, None, None, None, None, 16, 16, p, None, None, 0, -1, None)
    with pytest.raises(L.StereoHipError, match="null pointer"):
        fe(L.SD_F32, p, p, 8, 8, None, None, None, None, 16, 16, None, None, None, 0, -1, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        fe(L.SD_F32, p, p, 8, 8, None, None, None, None, 0, 16, p, None, None, 0, -1, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        fe(L.SD_F32, p, p, 8, 0, None, None, None, None, 16, 16, p, None, None, 0, -1, None)
    with pytest.raises(L.StereoHipError, match="go together"):
        fe(L.SD_F32, p, p, 8, 8, p, None, None, None, 16, 16, p, None, None, 0, -1, None)
    with pytest.raises(L.StereoHipError, match="slot 1 clear 1"):
        fe(L.SD_BF16, p, p, 8, 8, None, None, None, None, 16, 16, p, None, p, 1, 1, None)
    with pytest.raises(L.StereoHipError, match="dtype"):
        fe(7, p, p, 8, 8, None, None, None, None, 16, 16, p, None, None, 0, -1, None)
    with pytest.raises(L.StereoHipError, match="null pointer"):
        L.call("sd_live_rectify", p, 8, 8, None, p, p, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        L.call("sd_live_rectify", p, 0, 8, p, p, p, None)
    post = lambda *a: L.call("sd_live_post", *a)  # noqa: E731
    with pytest.raises(L.StereoHipError, match="null pointer"):
        post(None, None, 8, 8, p, 1, 0.0, 1.0, 0, 0.0, None, None, None, 0.0, 1.0, None, 0.0, 1.0, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        post(p, None, 8, 0, p, 1, 0.0, 1.0, 0, 0.0, None, None, None, 0.0, 1.0, None, 0.0, 1.0, None)
    with pytest.raises(L.StereoHipError, match="without a depth buffer"):
        post(p, None, 8, 8, p, 1, 0.0, 1.0, 1, 40.0, None, None, None, 0.0, 1.0, None, 0.0, 1.0, None)
    with pytest.raises(L.StereoHipError, match="without a confidence buffer"):
        post(p, p, 8, 8, p, 1, 0.0, 1.0, 0, 0.0, None, None, None, 0.0, 1.0, None, 0.0, 1.0, None)
    with pytest.raises(L.StereoHipError, match="null pointer"):
        L.call("sd_live_contours", p, 8, 8, 0.0, 10.0, 0.5, None, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        L.call("sd_live_contours", p, 0, 8, 0.0, 10.0, 0.5, p, None)
    with pytest.raises(L.StereoHipError, match="bad range"):
        L.call("sd_live_contours", p, 8, 8, 0.0, 10.0, 0.0, p, None)
    with pytest.raises(L.StereoHipError, match="null pointer"):
        L.call("sd_live_select", p, 8, 8, None, p, None, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        L.call("sd_live_select", p, 8, 0, p, p, None, None)
    with pytest.raises(L.StereoHipError, match="window 64"):
        L.call("sd_live_center", p, None, None, 8, 8, 64, p, None)
    with pytest.raises(L.StereoHipError, match="null pointer"):
        L.call("sd_live_center", None, None, None, 8, 8, 15, p, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        L.call("sd_live_center", p, None, None, 0, 8, 15, p, None)
    comp = lambda *a: L.call("sd_live_compose", *a)  # noqa: E731
    with pytest.raises(L.StereoHipError, match="nothing to do"):
        comp(None, None, None, None, None, None, None, None, None, 8, 8, 8, 8, None)
    with pytest.raises(L.StereoHipError, match="image a"):
        comp(p, None, p, None, None, None, None, None, None, 8, 8, 8, 8, None)
    with pytest.raises(L.StereoHipError, match="image b"):
        comp(None, None, None, p, p, None, None, None, None, 8, 8, 8, 8, None)
    with pytest.raises(L.StereoHipError, match=r"\(view\)"):
        comp(None, None, None, None, None, None, None, None, p, 8, 8, 8, 8, None)
    with pytest.raises(L.StereoHipError, match="bad sizes"):
        comp(p, p, p, None, None, None, None, None, None, 8, 8, 0, 8, None)
