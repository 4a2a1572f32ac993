"""The multi-rig classical loop's host side (no GPU): the batched matcher entries' exports and argument validation
(every check fails before any launch), the workspace size, ClassicDepthBatch's constructor checks."""

import ctypes

import numpy as np
import pytest

from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import sgm

P256 = ctypes.c_void_p(256)  # a non-null, 256-B aligned pointer that is never dereferenced
p = P256

NEW = ("sd_sgm_ws_bytes_n", "sd_sgm_compute_n", "sd_sgm_speckle_n", "sd_sgm_post_n", "sd_sgm_center_n")
LAUNCHING = NEW[1:]


def test_batched_entries_are_exported():
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and name in L.PROTOTYPES and name in L.exported_symbols(), name
    assert lib.sd_version() >= 104


@pytest.mark.parametrize("size", [(480, 640, 128), (9, 41, 16), (33, 200, 48)], ids=str)
def test_workspace_is_n_slices_of_the_single_stream_one(size):
    one = L.call("sd_sgm_ws_bytes", *size)
    assert one == sgm.ws_bytes(*size) and one % 256 == 0  # every slice keeps the base pointer's 256-B alignment
    for n in (1, 3, 64):
        assert L.call("sd_sgm_ws_bytes_n", n, *size) == n * one
    assert L.call("sd_sgm_ws_bytes_n", 0, *size) < 0 and L.call("sd_sgm_ws_bytes_n", 65, *size) < 0
    if size == (480, 640, 128):  # the documented figure: n x 160.4 MB, 157.3 MB of it the two volumes
        assert one == 2 * 78643200 + 2 * 307200 + 2 * 1228800 == 160358400


def _args(name, n=1, **kw):
    a = {
        "sd_sgm_compute_n": dict(n=n, gray_l=p, gray_r=p, H=16, W=64, min_disparity=0, num_disparities=16, block_size=5,
                                 P1=200, P2=800, disp12_max_diff=1, uniqueness_ratio=10, speckle_window=10,
                                 speckle_range=2, pre_filter_cap=31, mode=L.SD_SGM_MODE_3WAY, work=p, q=p, s=None),
        "sd_sgm_speckle_n": dict(n=n, q=p, H=16, W=64, invalid_value=-16, window=10, range=2, work=p, s=None),
        "sd_sgm_post_n": dict(n=n, q=p, H=16, W=64, Qdev=p, disp=p, z=p, code=p, minmax=p, s=None),
        "sd_sgm_center_n": dict(n=n, z=p, H=16, W=64, window=15, out=p, s=None),
    }[name]
    for k, v in kw.items():
        assert k in a, (name, k)
        a[k] = v
    return list(a.values())


@pytest.mark.parametrize("name", LAUNCHING)
def test_stream_count_is_checked_first(name):
    for n in (0, 65, -1):
        with pytest.raises(L.StereoHipError, match=rf"{name}: n = {n} streams"):
            L.call(name, *_args(name, n=n))
    # first: before a null pointer, a bad size or a bad mode is looked at
    with pytest.raises(L.StereoHipError, match=r"sd_sgm_compute_n: n = 65 streams"):
        L.call("sd_sgm_compute_n", *_args("sd_sgm_compute_n", n=65, gray_l=None, mode=7, H=-1))


NULLS = {
    "sd_sgm_compute_n": ["gray_l", "gray_r", "work", "q"],
    "sd_sgm_speckle_n": ["q", "work"],
    "sd_sgm_post_n": ["q", "Qdev", "disp", "z", "code", "minmax"],
    "sd_sgm_center_n": ["z", "out"],
}


@pytest.mark.parametrize("name", LAUNCHING)
def test_null_pointers_are_named(name):
    for arg in NULLS[name]:
        word = "Q" if arg == "Qdev" else arg
        with pytest.raises(L.StereoHipError, match=rf"{name}: null pointer.*\b{word}\b"):
            L.call(name, *_args(name, n=3, **{arg: None}))


def test_compute_n_rejects_what_compute_rejects():
    name = "sd_sgm_compute_n"
    with pytest.raises(L.StereoHipError, match=f"{name}: work must be 256-B aligned"):
        L.call(name, *_args(name, 3, work=ctypes.c_void_p(128)))
    with pytest.raises(L.StereoHipError, match=f"{name}: mode 7"):
        L.call(name, *_args(name, 3, mode=7))
    with pytest.raises(L.StereoHipError, match="multiple of 16"):
        L.call(name, *_args(name, 3, num_disparities=24))
    with pytest.raises(L.StereoHipError, match="block_size"):
        L.call(name, *_args(name, 3, block_size=4))
    with pytest.raises(L.StereoHipError, match="min_disparity"):
        L.call(name, *_args(name, 3, min_disparity=-1))
    with pytest.raises(L.StereoHipError, match="pre_filter_cap"):
        L.call(name, *_args(name, 3, pre_filter_cap=64))
    with pytest.raises(L.StereoHipError, match="0 <= P1 <= P2"):
        L.call(name, *_args(name, 3, P1=900))
    with pytest.raises(L.StereoHipError, match="uniqueness_ratio"):
        L.call(name, *_args(name, 3, uniqueness_ratio=101))
    with pytest.raises(L.StereoHipError, match="speckle"):
        L.call(name, *_args(name, 3, speckle_range=2000))
    with pytest.raises(L.StereoHipError, match=r"8 \* .* exceeds 65535"):  # the bound follows the mode's path count
        L.call(name, *_args(name, 3, block_size=9, P1=648, P2=2592, mode=L.SD_SGM_MODE_HH))
    with pytest.raises(L.StereoHipError, match=f"{name}: bad sizes"):
        L.call(name, *_args(name, 3, W=4097))
    with pytest.raises(L.StereoHipError, match=f"{name}: bad sizes"):
        L.call(name, *_args(name, 3, H=0))


def test_the_other_stages_reject_bad_arguments():
    with pytest.raises(L.StereoHipError, match="sd_sgm_speckle_n: window -1 range 2"):
        L.call("sd_sgm_speckle_n", *_args("sd_sgm_speckle_n", 2, window=-1))
    with pytest.raises(L.StereoHipError, match="sd_sgm_speckle_n: work must be 4-B aligned"):
        L.call("sd_sgm_speckle_n", *_args("sd_sgm_speckle_n", 2, work=ctypes.c_void_p(258)))
    with pytest.raises(L.StereoHipError, match="sd_sgm_speckle_n: bad sizes"):
        L.call("sd_sgm_speckle_n", *_args("sd_sgm_speckle_n", 2, W=0))
    with pytest.raises(L.StereoHipError, match="sd_sgm_post_n: bad sizes"):
        L.call("sd_sgm_post_n", *_args("sd_sgm_post_n", 2, H=0))
    with pytest.raises(L.StereoHipError, match=r"sd_sgm_center_n: window 64"):
        L.call("sd_sgm_center_n", *_args("sd_sgm_center_n", 2, window=64))
    # the single-stream forms keep their names in the messages
    with pytest.raises(L.StereoHipError, match="sd_sgm_center: null pointer"):
        L.call("sd_sgm_center", None, 16, 64, 15, p, None)
    with pytest.raises(L.StereoHipError, match="sd_sgm_post: null pointer"):
        L.call("sd_sgm_post", p, 16, 64, None, p, p, p, p, None)


class _Rect:
    def __init__(self, size=(64, 48)):
        self.image_size = size
        self.map_l_1 = self.map_r_1 = np.zeros((size[1], size[0], 2), dtype=np.int16)
        self.map_l_2 = self.map_r_2 = np.zeros((size[1], size[0]), dtype=np.uint16)


def test_classic_depth_batch_constructor_checks():
    Q = np.eye(4)
    for n in (0, 65, -1):
        with pytest.raises(ValueError, match="streams must be in"):
            sgm.ClassicDepthBatch(n, Q=Q)
    with pytest.raises(ValueError, match="reprojection matrix Q"):
        sgm.ClassicDepthBatch(2)
    with pytest.raises(ValueError, match=r"Q must be \[4, 4\] or \[n = 3, 4, 4\]"):
        sgm.ClassicDepthBatch(3, Q=np.stack([Q] * 2))
    with pytest.raises(ValueError, match="Q must be the 4 x 4"):
        sgm.ClassicDepthBatch(3, Q=np.eye(3))
    bad = np.stack([Q] * 3)
    bad[1, 3] = 0.0
    with pytest.raises(ValueError, match="last row is zero"):
        sgm.ClassicDepthBatch(3, Q=bad)
    with pytest.raises(ValueError, match=r"one entry per stream \(3\), got 2"):
        sgm.ClassicDepthBatch(3, rectification=[_Rect(), _Rect()], Q=Q)
    with pytest.raises(ValueError, match="no None entries"):
        sgm.ClassicDepthBatch(2, rectification=[_Rect(), None], Q=Q)
    with pytest.raises(ValueError, match="one image_size"):
        sgm.ClassicDepthBatch(2, rectification=[_Rect(), _Rect((32, 48))], Q=Q)
    with pytest.raises(ValueError, match="center_window"):
        sgm.ClassicDepthBatch(2, Q=Q, center_window=64)
    with pytest.raises(ValueError, match="--block-size"):
        sgm.ClassicDepthBatch(2, Q=Q, block_size=4)
    with pytest.raises(ValueError, match="mode"):
        sgm.ClassicDepthBatch(2, Q=Q, mode="nine")
    # what is accepted: one Q for all or one per stream, shared or per-stream maps
    c = sgm.ClassicDepthBatch(3, Q=Q, mode="hh", num_disparities=16, block_size=5)
    assert c.Q.shape == (3, 4, 4) and c.Q.dtype == np.float64 and c.matcher.mode == "hh" and c.shared_maps
    Qs = np.stack([Q * (i + 1) for i in range(3)])
    c = sgm.ClassicDepthBatch(3, rectification=[_Rect()] * 3, Q=Qs)
    assert np.array_equal(c.Q, Qs) and not c.shared_maps and c.image_size == (64, 48)
    assert sgm.ClassicDepthBatch(3, rectification=_Rect(), Q=Q).shared_maps
    with pytest.raises(RuntimeError, match="before the first step"):
        c._readout()
