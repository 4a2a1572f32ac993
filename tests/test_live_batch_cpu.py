"""The multi-stream live frame path's host side (no GPU): the batched C-ABI entries' exports and argument validation
(every check fails before any launch), LiveDepthBatch's constructor checks, forward_packed's batch parameter."""

import ctypes
import inspect

import numpy as np
import pytest

from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import engine, live

P16 = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced: validation fails before any launch

NEW = ("sd_live_frontend_n", "sd_live_rectify_n", "sd_live_post_n", "sd_live_contours_n", "sd_live_select_n_ws_bytes",
       "sd_live_select_n", "sd_live_center_n", "sd_live_compose_n")


def test_batched_entries_are_exported():
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and name in L.PROTOTYPES and name in L.exported_symbols(), name
    assert lib.sd_version() >= 103
    one = L.call("sd_live_select_ws_bytes")
    for n in (1, 3, 64):
        assert L.call("sd_live_select_n_ws_bytes", n) == n * one
    assert L.call("sd_live_select_n_ws_bytes", 0) < 0 and L.call("sd_live_select_n_ws_bytes", 65) < 0


# name -> a builder of a valid argument list for n streams of 8 x 8 frames and maps, with keyword overrides by position
p = P16


def _args(name, n=1, **kw):
    a = {
        "sd_live_frontend_n": dict(n=n, dtype=L.SD_F32, left=p, right=p, Hc=8, Wc=8, map1_l=None, map2_l=None,
                                   map1_r=None, map2_r=None, map_stride=0, H=16, W=16, xin=p, nchw=None, amax=None,
                                   slot=0, clear=-1, s=None),
        "sd_live_rectify_n": dict(n=n, frames=p, Hc=8, Wc=8, map1=p, map2=p, map_stride=0, views=p, s=None),
        "sd_live_post_n": dict(n=n, disp=p, logvar=None, H=8, W=8, state=p, copy_mask=0, hold_mask=0, alpha=0.0,
                               one_minus_alpha=1.0, depth_on=0, focal_baseline=None, depth=None, conf=None,
                               depth_code=None, depth_lo=0.0, depth_scale=1.0, conf_code=None, conf_lo=0.0,
                               conf_scale=1.0, s=None),
        "sd_live_contours_n": dict(n=n, depth=p, H=8, W=8, min_depth=0.0, max_depth=10.0, step=0.5, edge=p,
                                   hold_mask=0, s=None),
        "sd_live_select_n": dict(n=n, values=p, H=8, W=8, work=p, sel=p, code=None, hold_mask=0, s=None),
        "sd_live_center_n": dict(n=n, disp=p, depth=None, conf=None, H=8, W=8, window=15, out3=p, hold_mask=0, s=None),
        "sd_live_compose_n": dict(n=n, code_a=p, lut_a=p, vis_a=p, code_b=None, lut_b=None, vis_b=None, edge=None,
                                  view=None, left_view=None, H=8, W=8, Hc=8, Wc=8, hold_mask=0, s=None),
    }[name]
    for k, v in kw.items():
        assert k in a, (name, k)
        a[k] = v
    return list(a.values())


LAUNCHING = [name for name in NEW if name != "sd_live_select_n_ws_bytes"]


@pytest.mark.parametrize("name", LAUNCHING)
def test_stream_count_is_checked_first(name):
    for n in (0, 65, -1):
        with pytest.raises(L.StereoHipError, match=rf"{name}: n = {n} streams"):
            L.call(name, *_args(name, n=n))


NULLS = {
    "sd_live_frontend_n": [("left", "left"), ("right", "right"), ("xin", "xin")],
    "sd_live_rectify_n": [("frames", "frames"), ("views", "views"), ("map1", "map1"), ("map2", "map2")],
    "sd_live_post_n": [("disp", "disp"), ("state", "state")],
    "sd_live_contours_n": [("depth", "depth"), ("edge", "edge")],
    "sd_live_select_n": [("values", "values"), ("work", "work"), ("sel", "sel")],
    "sd_live_center_n": [("disp", "disp"), ("out3", "out3")],
    "sd_live_compose_n": [("lut_a", "lut_a"), ("vis_a", "vis_a")],
}


@pytest.mark.parametrize("name", LAUNCHING)
def test_null_pointers_are_named(name):
    for arg, word in NULLS[name]:
        with pytest.raises(L.StereoHipError, match=rf"{name}: null pointer.*\b{word}\b"):
            L.call(name, *_args(name, n=3, **{arg: None}))


def test_null_pointers_of_the_optional_groups():
    with pytest.raises(L.StereoHipError, match="depth enabled without a depth buffer or focal_baseline"):
        L.call("sd_live_post_n", *_args("sd_live_post_n", 2, depth_on=1, depth=p))
    with pytest.raises(L.StereoHipError, match="depth enabled without a depth buffer or focal_baseline"):
        L.call("sd_live_post_n", *_args("sd_live_post_n", 2, depth_on=1, focal_baseline=p))
    with pytest.raises(L.StereoHipError, match="logvar without a confidence buffer"):
        L.call("sd_live_post_n", *_args("sd_live_post_n", 2, logvar=p))
    with pytest.raises(L.StereoHipError, match="image b: lut_b, vis_b"):
        L.call("sd_live_compose_n", *_args("sd_live_compose_n", 2, code_b=p, lut_b=p))
    with pytest.raises(L.StereoHipError, match=r"null pointer \(view\)"):
        L.call("sd_live_compose_n", *_args("sd_live_compose_n", 2, left_view=p))
    with pytest.raises(L.StereoHipError, match="nothing to do"):
        L.call("sd_live_compose_n", *_args("sd_live_compose_n", 2, code_a=None, lut_a=None, vis_a=None))


def test_maps_go_together_and_the_stride_is_checked():
    fe = "sd_live_frontend_n"
    for kw in (dict(map1_l=p), dict(map2_l=p), dict(map1_r=p), dict(map2_r=p), dict(map1_l=p, map2_l=p, map1_r=p)):
        with pytest.raises(L.StereoHipError, match="map1 and map2 go together"):
            L.call(fe, *_args(fe, 3, **kw))
    with pytest.raises(L.StereoHipError, match="map1 and map2 go together"):
        L.call("sd_live_rectify_n", *_args("sd_live_rectify_n", 3, map2=None))
    for name in (fe, "sd_live_rectify_n"):
        for stride in (1, 63, 8 * 8 * 2, -64):  # 0 (shared) or Hc * Wc = 64 (per stream)
            with pytest.raises(L.StereoHipError, match=rf"map_stride {stride} "):
                L.call(name, *_args(name, 3, map_stride=stride))


MASKS = [("sd_live_post_n", "copy_mask"), ("sd_live_post_n", "hold_mask"), ("sd_live_contours_n", "hold_mask"),
         ("sd_live_select_n", "hold_mask"), ("sd_live_center_n", "hold_mask"), ("sd_live_compose_n", "hold_mask")]


@pytest.mark.parametrize("name,mask", MASKS)
def test_a_mask_bit_at_or_above_n_is_rejected(name, mask):
    for n, bad in ((1, 0b10), (3, 0b1000), (3, 1 << 63), (63, 1 << 63), (5, 0b100001)):
        with pytest.raises(L.StereoHipError, match=rf"{name}: {mask} 0x{bad:x} has a bit at or above n = {n}"):
            L.call(name, *_args(name, n, **{mask: bad}))


@pytest.mark.parametrize("name", LAUNCHING)
def test_the_single_stream_checks_are_kept(name):
    size = {"sd_live_frontend_n": "H", "sd_live_rectify_n": "Hc"}.get(name, "W")
    with pytest.raises(L.StereoHipError, match=f"{name}: bad sizes"):
        L.call(name, *_args(name, 2, **{size: 0}))
    if name == "sd_live_center_n":
        with pytest.raises(L.StereoHipError, match="window 64"):
            L.call(name, *_args(name, 2, window=64))
    if name == "sd_live_contours_n":
        with pytest.raises(L.StereoHipError, match="bad range"):
            L.call(name, *_args(name, 2, step=0.0))
    if name == "sd_live_frontend_n":
        with pytest.raises(L.StereoHipError, match="dtype 7"):
            L.call(name, *_args(name, 2, dtype=7))
        with pytest.raises(L.StereoHipError, match="slot 1 clear 1"):
            L.call(name, *_args(name, 2, amax=p, slot=1, clear=1))
        with pytest.raises(L.StereoHipError, match="16-B aligned"):
            L.call(name, *_args(name, 2, xin=ctypes.c_void_p(8)))


# ---------------------------------------------------------------------- LiveDepthBatch's constructor
class M:
    in_channels = 6


def _rect(size=(40, 30), focal=800.0, baseline=0.1):
    w, h = size
    z1, z2 = np.zeros((h, w, 2), np.int16), np.zeros((h, w), np.uint16)
    return live.Rectification(z1, z2, z1, z2, size, focal, baseline)


def test_streams_range():
    for n in (0, 65, -3):
        with pytest.raises(ValueError, match=r"streams must be in \[1, 64\]"):
            live.LiveDepthBatch(M(), n, (48, 32))
    assert live.LiveDepthBatch(M(), 1, (48, 32)).streams == 1
    assert live.LiveDepthBatch(M(), 64, (48, 32)).streams == 64


def test_sequence_lengths():
    for kw, name in ((dict(focal_length_px=[800.0, 800.0]), "focal_length_px"),
                     (dict(baseline_m=(0.1,)), "baseline_m"),
                     (dict(calibration_width_px=np.array([640, 640, 640, 640])), "calibration_width_px"),
                     (dict(rectification=[_rect(), _rect()]), "rectification")):
        with pytest.raises(ValueError, match=rf"{name}: a sequence must have one entry per stream \(3\)"):
            live.LiveDepthBatch(M(), 3, (48, 32), **kw)
    with pytest.raises(ValueError, match="no None entries"):
        live.LiveDepthBatch(M(), 2, (48, 32), rectification=[_rect(), None])


def test_depth_is_enabled_per_stream_and_never_mixed():
    ld = live.LiveDepthBatch(M(), 3, (48, 32), focal_length_px=[800.0, 400.0, 200.0], baseline_m=0.1,
                             calibration_width_px=640)
    assert ld.depth_enabled and ld.focal_length_px_model == [f * (48 / 640.0) for f in (800.0, 400.0, 200.0)]
    assert ld.baseline_m == [0.1] * 3
    assert not live.LiveDepthBatch(M(), 3, (48, 32)).depth_enabled
    assert not live.LiveDepthBatch(M(), 3, (48, 32), focal_length_px=800.0, baseline_m=0.1).depth_enabled  # no width
    for kw in (dict(focal_length_px=800.0, baseline_m=[0.1, None, 0.1], calibration_width_px=640),
               dict(focal_length_px=[800.0, 800.0, None], baseline_m=0.1, calibration_width_px=640),
               dict(focal_length_px=800.0, baseline_m=0.1, calibration_width_px=[640, 0, 640]),
               dict(rectification=[_rect(), _rect(baseline=None), _rect()])):
        with pytest.raises(ValueError, match="enabled for some streams and not for others"):
            live.LiveDepthBatch(M(), 3, (48, 32), **kw)
    # a rectification defines the geometry, shared or per stream
    ld = live.LiveDepthBatch(M(), 2, (48, 32), rectification=_rect(focal=500.0), focal_length_px=1.0)
    assert ld.shared_maps and ld.depth_enabled and ld.focal_length_px_model == [500.0 * (48 / 40.0)] * 2
    ld = live.LiveDepthBatch(M(), 2, (48, 32), rectification=[_rect(focal=500.0), _rect(focal=250.0, baseline=0.2)])
    assert not ld.shared_maps and ld.baseline_m == [0.1, 0.2]
    assert ld.focal_length_px_model == [500.0 * (48 / 40.0), 250.0 * (48 / 40.0)]


def test_one_image_size():
    with pytest.raises(ValueError, match="one image_size"):
        live.LiveDepthBatch(M(), 2, (48, 32), rectification=[_rect((40, 30)), _rect((30, 40))])
    assert live.LiveDepthBatch(M(), 2, (48, 32), rectification=[_rect(), _rect()]).image_size == (40, 30)


def test_stream_rectification():
    """What LiveDepthBatch and ClassicDepthBatch both make of their rectification argument."""
    assert live.stream_rectification(None, 3) == (None, True, None)
    r = _rect()
    rects, shared, size = live.stream_rectification(r, 3)
    assert shared and size == (40, 30) and len(rects) == 3 and all(x is r for x in rects)
    three = [_rect(), _rect(), _rect()]
    for seq in (three, tuple(three)):
        rects, shared, size = live.stream_rectification(seq, 3)
        assert not shared and size == (40, 30) and all(x is y for x, y in zip(rects, three))
    rects, shared, _ = live.stream_rectification([r], 1)  # one stream with a list of one: per-stream maps
    assert rects == [r] and not shared
    with pytest.raises(ValueError, match=r"rectification: a sequence must have one entry per stream \(3\), got 2"):
        live.stream_rectification(three[:2], 3)
    with pytest.raises(ValueError, match="no None entries"):
        live.stream_rectification([three[0], None, three[2]], 3)
    with pytest.raises(ValueError, match=r"one image_size, got \[\(30, 40\), \(40, 30\)\]"):
        live.stream_rectification([_rect(), _rect((30, 40)), _rect()], 3)


def test_upload_maps_checks_and_stacks():
    rng = np.random.default_rng(0)
    rects = []
    for _ in range(2):
        r = _rect()
        r.map_l_1 = rng.integers(-100, 100, (30, 40, 2)).astype(np.int16)
        r.map_l_2 = rng.integers(0, 65536, (30, 40)).astype(np.uint16)  # values above 32767: the bits are kept
        r.map_r_1 = np.asfortranarray(r.map_l_1 + 1)
        rects.append(r)
    m1, m2 = live.upload_maps(rects, "l", 30, 40, "cpu")
    assert m1.dtype == m2.dtype == live.torch.int16
    assert tuple(m1.shape) == (2, 30, 40, 2) and tuple(m2.shape) == (2, 30, 40)
    assert m1.is_contiguous() and m2.is_contiguous()
    for i, r in enumerate(rects):
        assert np.array_equal(m1[i].numpy(), r.map_l_1) and np.array_equal(m2[i].numpy().view(np.uint16), r.map_l_2)
    m1r, _ = live.upload_maps(rects[:1], "r", 30, 40, "cpu")  # the other side, made contiguous
    assert tuple(m1r.shape) == (1, 30, 40, 2) and np.array_equal(m1r[0].numpy(), rects[0].map_r_1)
    for attr, bad in (("map_l_1", rects[1].map_l_1.astype(np.int32)), ("map_l_2", rects[1].map_l_2.view(np.int16)),
                      ("map_l_2", rects[1].map_l_2.astype(np.float32)), ("map_l_1", rects[1].map_l_1[:, :, :1]),
                      ("map_l_2", rects[1].map_l_2[:29])):
        good = getattr(rects[1], attr)
        setattr(rects[1], attr, bad)
        with pytest.raises(ValueError, match=r"rectification maps: map1 int16 \[H, W, 2\] and map2 uint16 \[H, W\]"):
            live.upload_maps(rects, "l", 30, 40, "cpu")
        setattr(rects[1], attr, good)
    with pytest.raises(ValueError, match="rectification maps"):  # the frame's size, not the maps' own
        live.upload_maps(rects, "l", 40, 30, "cpu")
    live.upload_maps(rects, "l", 30, 40, "cpu")


def test_colormap_table():
    assert np.array_equal(live.colormap_table("magma"), live.colormap_lut("magma"))
    own = np.asfortranarray(np.arange(768, dtype=np.uint8).reshape(256, 3))
    got = live.colormap_table(own)
    assert got.flags.c_contiguous and np.array_equal(got, own)
    for bad in (own.astype(np.float32), own[:255], own.T):
        with pytest.raises(ValueError, match=r"colormap: a name or a \[256, 3\] uint8 BGR table"):
            live.colormap_table(bad)
    with pytest.raises(ValueError, match="unknown colormap"):
        live.colormap_table("jet")


def test_the_other_checks_are_live_depths():
    with pytest.raises(ValueError, match="center_window"):
        live.LiveDepthBatch(M(), 2, (48, 32), center_window=64)
    with pytest.raises(ValueError, match="ema_alpha"):
        live.LiveDepthBatch(M(), 2, (48, 32), ema_alpha=1.5)
    with pytest.raises(ValueError, match="unknown colormap"):
        live.LiveDepthBatch(M(), 2, (48, 32), colormap="jet")
    with pytest.raises(ValueError, match=r"\[256, 3\] uint8"):
        live.LiveDepthBatch(M(), 2, (48, 32), colormap=np.zeros((256, 3), np.float32))
    with pytest.raises(ValueError, match="multiples of 16"):
        live.LiveDepthBatch(M(), 2, (50, 32))

    class Mono:
        in_channels = 3

    with pytest.raises(ValueError, match="in_channels 6"):
        live.LiveDepthBatch(Mono(), 2, (48, 32))
    ld = live.LiveDepthBatch(M(), 3, (48, 32))
    with pytest.raises(ValueError, match="stream must be in"):
        ld.reset(3)
    ld._first = [False] * 3
    ld.reset(1)
    assert ld._first == [False, True, False]
    ld.reset()
    assert ld._first == [True] * 3


def test_forward_packed_takes_a_batch():
    sig = inspect.signature(engine.UNetEngine.forward_packed)
    assert "batch" in sig.parameters and sig.parameters["batch"].default == 1
    assert list(sig.parameters)[:4] == ["self", "H", "W", "pack"]
