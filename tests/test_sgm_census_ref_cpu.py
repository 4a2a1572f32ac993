"""The census / Hamming cost's restatement (tests/sgm_census_ref.py) against hand-computed values and against the
property it exists for, and the host side of the feature: StereoSGM's constructor and the adapt tool's options. No GPU.
"""

import numpy as np
import pytest

import sgm_census_ref as CR
import sgm_ref as R
from stereo_depth_estimation_amd import adapt as A
from stereo_depth_estimation_amd import sgm


# ---------------------------------------------------------------------- step 2c by hand
def test_descriptors_of_a_3x3_image_by_hand():
    """Window (3, 3): bit 0 (-1,-1), 1 (-1,0), 2 (-1,+1), 3 (0,-1), 4 (0,+1), 5 (+1,-1), 6 (+1,0), 7 (+1,+1); a bit is
    set where the neighbour, taken from the nearest pixel inside the image, is strictly below the centre."""
    g = np.array([[5, 3, 8],
                  [2, 5, 9],
                  [7, 1, 5]], dtype=np.uint8)
    want = np.array([
        # (0,0) c=5: (-1,+1)->3, (0,+1)=3, (+1,-1)->2, (+1,0)=2        -> bits 2,4,5,6
        # (0,1) c=3: (+1,-1)=2                                          -> bit 5
        # (0,2) c=8: (-1,-1)->3, (0,-1)=3, (+1,-1)=5                    -> bits 0,3,5
        [4 + 16 + 32 + 64, 32, 1 + 8 + 32],
        # (1,0) c=2: (+1,+1)=1                                          -> bit 7
        # (1,1) c=5: (-1,0)=3, (0,-1)=2, (+1,0)=1 (the two 5s are ties) -> bits 1,3,6
        # (1,2) c=9: all but (0,+1), which is the pixel itself          -> all but bit 4
        [128, 2 + 8 + 64, 255 - 16],
        # (2,0) c=7: (-1,-1)->2, (-1,0)=2, (-1,+1)=5, (0,+1)=1, (+1,+1)->1 -> bits 0,1,2,4,7
        # (2,1) c=1: nothing is below 1                                 -> 0
        # (2,2) c=5: (0,-1)=1, (+1,-1)->1                               -> bits 3,5
        [1 + 2 + 4 + 16 + 128, 0, 8 + 32]], dtype=np.uint64)
    assert np.array_equal(CR.census(g, 3, 3), want)


def test_corner_descriptors_of_a_ramp_with_the_7x9_window():
    """g = 10 y + x, strictly increasing along both axes. Top-left corner: nothing is below it, 0. Bottom-right corner:
    every position with dy < 0 or dx < 0 is below it, every other one is the corner itself (replicated). Positions are
    numbered (dy + 3) * 9 + (dx + 4), the centre is number 31 and takes no bit, so the later ones move down by one:
    rows dy < 0 are bits 0..26, dy = 0 gives dx < 0 = bits 27..30, and rows dy = 1, 2, 3 give bits 35..38, 44..47,
    53..56."""
    H, W = 8, 12
    g = (10 * np.arange(H)[:, None] + np.arange(W)[None, :]).astype(np.uint8)
    d = CR.census(g, 7, 9)
    assert d[0, 0] == 0
    assert int(d[H - 1, W - 1]) == (1 << 31) - 1 | 0xF << 35 | 0xF << 44 | 0xF << 53
    assert (d >> np.uint64(62) == 0).all()  # bits >= nbits are zero
    # an interior pixel sees its whole window, and a neighbour is below it exactly when 10 dy + dx < 0: with |dx| <= 4
    # that is every position before the centre in row-major order and none after it, bits 0..30
    assert int(d[4, 6]) == (1 << 31) - 1


def test_a_constant_image_has_zero_descriptors_and_zero_cost():
    """The comparison is strict: ties set no bit."""
    g = np.full((9, 40), 77, dtype=np.uint8)
    p = CR.Params(window=(5, 5), num_disparities=16, block_size=3)
    st = CR.compute_stages(g, g, p)
    assert not st["desc_l"].any() and not st["desc_r"].any() and not st["C"].any()


def test_popcount_against_python():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 4096, dtype=np.uint64)
    x[:4] = np.array([0, 1, (1 << 64) - 1, 1 << 63], dtype=np.uint64)
    assert np.array_equal(CR.popcount(x), [bin(int(v)).count("1") for v in x])
    assert CR.popcount(x).max() == 64


def test_pixel_cost_is_the_hamming_distance():
    rng = np.random.default_rng(1)
    gl, gr = R.shifted_scene(rng, 6, 40, 5)
    p = CR.Params(window=(3, 3), min_disparity=2, num_disparities=16, block_size=3)
    cl, cr = CR.census(gl, 3, 3), CR.census(gr, 3, 3)
    cost = CR.pixel_cost(cl, cr, p)
    assert cost.shape == (6, 40 - 18, 16) and cost.min() >= 0 and cost.max() <= 8
    for y, x, d in ((0, 18, 0), (3, 25, 7), (5, 39, 15)):
        assert cost[y, x - 18, d] == bin(int(cl[y, x]) ^ int(cr[y, x - d - 2])).count("1")
    assert (cost[:, :, 3] == 0).mean() > 0.9  # d = 3 + minD = 5 is the scene's shift


# ---------------------------------------------------------------------- the property
invariance_scene, INVARIANCE_KW = CR.invariance_scene, CR.INVARIANCE_KW


def test_the_tables_are_strictly_increasing_and_differ():
    _, _, f, h = invariance_scene()
    assert len(f) == len(h) == 86 and (np.diff(f.astype(int)) > 0).all() and (np.diff(h.astype(int)) > 0).all()
    assert not np.array_equal(f, h) and (f != np.arange(86)).any()


@pytest.mark.parametrize("window", [(3, 3), (5, 5), (7, 9)], ids=lambda w: "%dx%d" % w)
def test_census_is_invariant_to_monotone_intensity_maps(window):
    gl, gr, f, h = invariance_scene()
    p = CR.Params(window=window, **INVARIANCE_KW)
    q = CR.compute(gl, gr, p)
    assert (q[:, p.maxD:] != p.invalid).mean() > 0.5  # the scene is matched
    assert np.array_equal(CR.census(f[gl], *window), CR.census(gl, *window))
    assert np.array_equal(CR.compute(f[gl], h[gr], p), q)


def test_birchfield_tomasi_is_not():
    gl, gr, f, h = invariance_scene()
    p = R.Params(**INVARIANCE_KW)
    assert not np.array_equal(R.compute(f[gl], h[gr], p), R.compute(gl, gr, p))


# ---------------------------------------------------------------------- StereoSGM's constructor (no device)
def test_constructor_checks_cost_and_window():
    m = sgm.StereoSGM()
    assert (m.cost, m.census_window, m.nbits, m.cost_id) == ("bt", None, None, 0)
    m = sgm.StereoSGM(cost="census")
    assert (m.cost, m.census_window, m.nbits, m.cost_id) == ("census", (7, 9), 62, 1)
    assert m.P1 == 8 * 49 and m.P2 == 32 * 49  # the application's defaults
    for w, bits in (((3, 3), 8), ((5, 5), 24), ((7, 7), 48), ((7, 9), 62), ("5x5", 24), ([7, 7], 48)):
        m = sgm.StereoSGM(cost="census", census_window=w)
        assert m.nbits == bits and m.census_window == (tuple(int(v) for v in w.split("x")) if isinstance(w, str) else tuple(w))
    with pytest.raises(ValueError, match="cost must be one of"):
        sgm.StereoSGM(cost="sad")
    for w in ((9, 7), (7, 11), (4, 4), (7,), "7by9", 7):
        with pytest.raises(ValueError, match="census_window must be one of 3x3, 5x5, 7x7, 7x9"):
            sgm.StereoSGM(cost="census", census_window=w)
    with pytest.raises(ValueError, match="census_window .* cost='census'"):
        sgm.StereoSGM(cost="bt", census_window=(7, 9))
    with pytest.raises(ValueError, match="pre_filter_cap"):  # checked as before, though unused
        sgm.StereoSGM(cost="census", pre_filter_cap=64)


def test_constructor_applies_the_census_bound():
    # 8 * (121 * 62 + 32 * 121) = 90992 > 65535
    with pytest.raises(ValueError, match=r"8 \* \(block_size\^2 \* nbits \+ P2\) = 90992 exceeds 65535 \(nbits = 62"):
        sgm.StereoSGM(cost="census", mode="hh", block_size=11)
    assert sgm.StereoSGM(cost="census", mode="hh", block_size=9).nbits == 62      # 8 * (81 * 94) = 60912
    assert sgm.StereoSGM(cost="census", mode="3way", block_size=11).nbits == 62   # 3 * (121 * 94) = 34122
    for mode in ("3way", "hh4", "sgbm"):  # (7, 9) admits every block size in the modes of up to five paths
        for bs in (3, 5, 7, 9, 11):
            sgm.StereoSGM(cost="census", mode=mode, block_size=bs)
    # the Birchfield-Tomasi bound is what it was: bs = 11 does not fit four paths there, and does with the census cost
    with pytest.raises(ValueError, match=r"2 \* pre_filter_cap \+ 63"):
        sgm.StereoSGM(mode="hh4", block_size=11)
    with pytest.raises(ValueError, match="nbits = 62"):
        sgm.StereoSGM(cost="census", block_size=11, P2=21000)
    assert sgm.ws_bytes(480, 640, 128, "census") - sgm.ws_bytes(480, 640, 128) == 2 * 8 * 480 * 640
    with pytest.raises(AssertionError):
        CR.Params(mode="hh", block_size=11)
    CR.Params(mode="hh", block_size=9)


# ---------------------------------------------------------------------- adapt's options
def test_adapt_proxy_cost_options(tmp_path):
    good = dict(left_dir=tmp_path, right_dir=tmp_path, output_dir=tmp_path / "out")
    with pytest.raises(ValueError, match="--proxy-cost: .* need a positive --proxy-weight"):
        A.adapt_options(**good, proxy_cost="census")
    with pytest.raises(ValueError, match="--proxy-census-window: .* need a positive --proxy-weight"):
        A.adapt_options(**good, proxy_census_window="5x5")
    on = A.adapt_options(**good, proxy_weight=0.5, proxy_cost="census", height=32, width=80)
    assert (on["proxy_cost"], on["proxy_census_window"]) == ("census", "7x9")
    assert A.adapt_options(**on) == on  # the result is its own argument set
    on = A.adapt_options(**good, proxy_weight=0.5, proxy_cost="census", proxy_census_window="5x5")
    assert (on["proxy_cost"], on["proxy_census_window"]) == ("census", "5x5")
    assert "proxy_cost" not in A.adapt_options(**good, proxy_weight=0.5)  # bt, the default: the options are what they were
    assert A.PROXY_DEFAULTS["proxy_cost"] == "bt"
    for kw, msg in ((dict(proxy_cost="sad"), "cost must be one of"), (dict(proxy_census_window="5x5"), "cost='census'"),
                    (dict(proxy_cost="census", proxy_census_window="9x9"), "census_window must be one of"),
                    (dict(proxy_cost="census", proxy_mode="hh", proxy_block_size=11), "nbits = 62")):
        with pytest.raises(ValueError, match=msg):
            A.adapt_options(**good, proxy_weight=1.0, **kw)
    a = A.build_parser().parse_args(["--checkpoint", "c", "--dataset-root", "d", "--output-dir", "o", "--proxy-weight", "1",
                                     "--proxy-cost", "census", "--proxy-census-window", "7x7"])
    assert (a.proxy_cost, a.proxy_census_window) == ("census", "7x7")
    a = A.build_parser().parse_args(["--checkpoint", "c", "--dataset-root", "d", "--output-dir", "o"])
    assert (a.proxy_cost, a.proxy_census_window) == (None, None)
