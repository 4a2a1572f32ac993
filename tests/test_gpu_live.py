"""The live frame path on the device (csrc/live.hip, live.py; needs an MI355X), B = 1 throughout.

Front end against tests/live_ref.py (float64): |delta| <= 4 * max(Hc, Wc) * 2^-23 + 1e-6, i.e. fp32 rounding of a source
coordinate of that size times a value range of 1; the packed engine input bit-equal to sd_pack_input of the NCHW
output. Post stage, select, centre medians against the reference's own numpy results (tests/golden/live_post.npz):
bit-equal except exp (4 ulp: device expf and numpy's exp carry about 1 ulp each) and the percentile interpolation
(1 ulp: numpy's internal rounding order). Compose within 1 code of the float64 statement, exact at equal sizes.
Whole path: LiveDepth.step bit-equal to model(x) fed the front end's NCHW output, in fp32, bf16 and fp8.
"""

import numpy as np
import pytest
import torch

import live_ref as R
from oracle import unet_ref as U
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import live

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 32, 48


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(golden_dir / "live_post.npz"))


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.as_tensor(a).to(DEV)


def _s():
    return L.stream_handle()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bit_equal(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _ulp_diff(got, want):
    """max distance in float32 steps over the non-NaN values (NaN positions must agree)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    a = got[~nan].view(np.int32).astype(np.int64)
    b = want[~nan].view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def _frames(rng, Hc, Wc):
    return rng.integers(0, 256, (Hc, Wc, 3), dtype=np.uint8), rng.integers(0, 256, (Hc, Wc, 3), dtype=np.uint8)


def _front(left, right, maps_l, maps_r, dtype=L.SD_F32, amax=None, slot=0, clear=-1, h=H, w=W):
    """(xin raw tensor, nchw [1, 6, h, w]) of sd_live_frontend."""
    Hc, Wc = left.shape[:2]
    keep = [_dev(left), _dev(right)] + [_dev(m) for m in (maps_l or (None, None)) + (maps_r or (None, None))]
    xin = torch.empty(h * w * 8, dtype=torch.bfloat16 if dtype == L.SD_BF16 else torch.float32, device=DEV)
    nchw = torch.empty(1, 6, h, w, dtype=torch.float32, device=DEV)
    L.call("sd_live_frontend", dtype, keep[0].data_ptr(), keep[1].data_ptr(), Hc, Wc, *[L.ptr(m) for m in keep[2:]],
           h, w, xin.data_ptr(), nchw.data_ptr(), L.ptr(amax), slot, clear, _s())
    torch.cuda.synchronize()
    return xin, nchw


# ---------------------------------------------------------------------- front end
SIZES = [(37, 53), (32, 48), (64, 96), (16, 24)]


@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("Hc,Wc", SIZES)
def test_front_end_matches_the_reference_statement(Hc, Wc, with_maps):
    rng = np.random.default_rng(Hc * 100 + Wc + with_maps)
    left, right = _frames(rng, Hc, Wc)
    ml = R.random_maps(rng, Hc, Wc) if with_maps else None
    mr = R.random_maps(rng, Hc, Wc) if with_maps else None
    if with_maps:
        x, y = ml[0][..., 0].astype(int), ml[0][..., 1].astype(int)
        out = (x < 0) | (x >= Wc - 1) | (y < 0) | (y >= Hc - 1)
        assert 0.05 < out.mean() < 0.25 and (x == -1).any() and (x == Wc).any()
    want = R.front_end(left, right, ml, mr, H, W)
    bound = 4 * max(Hc, Wc) * 2.0 ** -23 + 1e-6
    for dtype, tdt in ((L.SD_F32, torch.float32), (L.SD_BF16, torch.bfloat16)):
        amax = torch.tensor([0, 123, 456], dtype=torch.int32, device=DEV)
        xin, nchw = _front(left, right, ml, mr, dtype, amax=amax, slot=0, clear=1)
        b = nchw.cpu().numpy()[0].astype(np.float64)
        err = np.abs(b - want).max()
        print(f"front end {Hc}x{Wc} maps={with_maps} dtype={dtype}: max |delta| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        # (a) is sd_pack_input / sd_pack_input_amax of (b), bit for bit, and carries the amax protocol
        ref = torch.empty_like(xin)
        L.call("sd_pack_input", dtype, nchw.data_ptr(), 1, 6, H, W, 8, ref.data_ptr(), _s())
        ref2 = torch.empty_like(xin)
        amax2 = torch.tensor([0, 123, 456], dtype=torch.int32, device=DEV)
        L.call("sd_pack_input_amax", dtype, nchw.data_ptr(), 1, 6, H, W, 8, ref2.data_ptr(), amax2.data_ptr(), 0, 1, _s())
        torch.cuda.synchronize()
        iv = torch.int16 if dtype == L.SD_BF16 else torch.int32
        assert torch.equal(xin.view(iv), ref.view(iv)) and torch.equal(xin.view(iv), ref2.view(iv))
        assert torch.equal(amax, amax2)
        a = amax.cpu().numpy()
        assert a[:1].view(np.float32)[0] == np.float32(nchw.abs().max().item()) and a[1] == 0 and a[2] == 456
        # without amax: nothing but the pack
        xin3, _ = _front(left, right, ml, mr, dtype)
        assert torch.equal(xin3.view(iv), xin.view(iv))
    if (Hc, Wc) == (H, W) and not with_maps:  # identity: the bytes / 255
        x8 = np.concatenate([left[..., ::-1], right[..., ::-1]], axis=-1).transpose(2, 0, 1).astype(np.float32)
        assert np.array_equal(nchw.cpu().numpy()[0], x8 / np.float32(255.0))
    if (Hc, Wc) == (64, 96) and not with_maps:  # exact 2x reduction: the mean of 2 x 2 pixels
        m = left.astype(np.float64).reshape(32, 2, 48, 2, 3).mean(axis=(1, 3))[..., ::-1].transpose(2, 0, 1) / 255.0
        assert np.abs(nchw.cpu().numpy()[0, :3] - m).max() <= bound


@pytest.mark.parametrize("Hc,Wc", [(37, 53), (16, 24)])
def test_rectified_view(Hc, Wc):
    rng = np.random.default_rng(7 + Hc)
    frame, _ = _frames(rng, Hc, Wc)
    x, y = np.meshgrid(np.arange(Wc, dtype=np.float64), np.arange(Hc, dtype=np.float64))
    for m1, m2, exact in (R.random_maps(rng, Hc, Wc) + (False,), live.quantize_maps(x, y) + (True,)):
        view = torch.empty(Hc, Wc, 3, dtype=torch.uint8, device=DEV)
        d = [_dev(frame), _dev(m1), _dev(m2)]
        L.call("sd_live_rectify", d[0].data_ptr(), Hc, Wc, d[1].data_ptr(), d[2].data_ptr(), view.data_ptr(), _s())
        got = view.cpu().numpy().astype(int)
        want = R.view_u8(frame, m1, m2).astype(int)
        assert np.abs(got - want).max() <= 1
        if exact:
            assert np.array_equal(got, frame.astype(int))


# ---------------------------------------------------------------------- post stage
def _post(disp, logvar=None, state=None, copy=1, alpha=0.0, fb=None):
    H, W = disp.shape
    disp_d, lv_d = _dev(disp), _dev(logvar)
    state = torch.empty(H, W, device=DEV) if state is None else state
    on = fb is not None
    depth = torch.empty(H, W, device=DEV)
    conf = torch.empty(H, W, device=DEV)
    dcode = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    ccode = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    L.call("sd_live_post", disp_d.data_ptr(), L.ptr(lv_d), H, W, state.data_ptr(), copy, float(np.float32(alpha)),
           float(np.float32(1.0 - alpha)), int(on), float(np.float32(fb)) if on else 0.0,
           depth.data_ptr() if on else None, conf.data_ptr() if lv_d is not None else None,
           dcode.data_ptr() if on else None, 0.0, float(np.float32(max(10.0 - 0.0, 1e-6))),
           ccode.data_ptr() if lv_d is not None else None, 0.0, float(np.float32(max(5.0 - 0.0, 1e-6))), _s())
    torch.cuda.synchronize()
    return {"state": state, "depth": depth, "conf": conf, "dcode": dcode, "ccode": ccode}


def _contours(depth_t):
    H, W = depth_t.shape
    edge = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    L.call("sd_live_contours", depth_t.data_ptr(), H, W, 0.0, 10.0, 0.5, edge.data_ptr(), _s())
    return edge.cpu().numpy()


def test_post_stage_equals_the_reference(gold):
    fb = float(gold["focal_model"]) * float(gold["baseline"])
    out = _post(gold["disp"], gold["logvar"], fb=fb)
    _assert_bit_equal(out["state"].cpu().numpy(), gold["disp"])  # no EMA: the prediction itself
    _assert_bit_equal(out["depth"].cpu().numpy(), gold["depth"])
    assert np.isnan(gold["depth"]).sum() > 50 and np.isnan(gold["depth"][3, 2])  # the 1e-6 threshold is invalid
    assert np.array_equal(out["dcode"].cpu().numpy(), gold["depth_code"])
    edge = _contours(out["depth"])
    assert np.array_equal(edge, gold["contour"]) and 0 < (edge > 0).mean() < 1
    ulp = _ulp_diff(out["conf"].cpu().numpy(), gold["conf"])
    print("confidence: max ulp distance", ulp)
    assert ulp <= 4
    assert np.array_equal(out["ccode"].cpu().numpy(), gold["conf_code"])
    # an all-invalid map
    bad = _dev(gold["invalid"])
    assert np.array_equal(_contours(bad), gold["invalid_contour"]) and not gold["invalid_contour"].any()


@pytest.mark.parametrize("h,w", [(5, 7), (6, 10), (3, 8)])
def test_post_stage_at_sizes_off_the_vector_path(gold, h, w):
    """32 x 48 takes the four-elements-per-thread kernels; 5 x 7 (odd count) takes the one-element ones everywhere,
    6 x 10 the vector post with the scalar contour kernel (W % 4 != 0), 3 x 8 rows of two vectors. The reference is
    tests/live_ref.py's numpy float32 post stage, which test_live_cpu holds equal to the fixture."""
    fb = float(gold["focal_model"]) * float(gold["baseline"])
    disp = np.ascontiguousarray(gold["disp"][1:1 + h, 1:1 + w])  # the rows with the bin edges and the 1e-6 threshold
    logvar = np.ascontiguousarray(gold["logvar"][1:1 + h, 1:1 + w])
    prev = np.ascontiguousarray(gold["ema/in1"][:h, :w])
    alpha = float(gold["alpha"])
    state = _dev(prev).clone()
    out = _post(disp, logvar, state=state, copy=0, alpha=alpha, fb=fb)
    with np.errstate(all="ignore"):
        s_want = alpha * disp + (1.0 - alpha) * prev
        conf_want = np.exp(-0.5 * logvar)
    _assert_bit_equal(out["state"].cpu().numpy(), s_want)
    depth_want = R.depth_from_disparity(s_want, float(gold["focal_model"]), float(gold["baseline"]))
    _assert_bit_equal(out["depth"].cpu().numpy(), depth_want)
    assert np.array_equal(out["dcode"].cpu().numpy(), R.codes(depth_want, 0.0, 10.0))
    assert np.array_equal(_contours(out["depth"]), R.contour_mask(depth_want, 0.5, 0.0, 10.0))
    conf = out["conf"].cpu().numpy()
    assert _ulp_diff(conf, conf_want) <= 4
    assert np.array_equal(out["ccode"].cpu().numpy(), R.codes(conf, 0.0, 5.0))
    # no EMA: the depth of the slice itself, with its contour edges
    out = _post(disp, fb=fb)
    _assert_bit_equal(out["depth"].cpu().numpy(), np.ascontiguousarray(gold["depth"][1:1 + h, 1:1 + w]))
    edge = _contours(out["depth"])
    assert np.array_equal(edge, R.contour_mask(gold["depth"][1:1 + h, 1:1 + w], 0.5, 0.0, 10.0)) and edge.any()
    _check_select(disp, _percentiles64(disp))


def test_ema_sequence_equals_the_reference(gold):
    alpha = float(gold["alpha"])
    state = torch.zeros(H, W, device=DEV)
    for i in range(3):
        out = _post(gold[f"ema/in{i}"], state=state, copy=int(i == 0), alpha=alpha)
        _assert_bit_equal(out["state"].cpu().numpy(), gold[f"ema/out{i}"])
    assert not np.array_equal(gold["ema/out2"], gold["ema/in2"])


# ---------------------------------------------------------------------- select
def _select(m):
    h, w = m.shape
    work = torch.zeros(L.call("sd_live_select_ws_bytes") // 4, dtype=torch.int32, device=DEV)
    sel = torch.zeros(8, device=DEV)
    code = torch.empty(h, w, dtype=torch.uint8, device=DEV)
    md = _dev(m)
    for _ in range(2):  # the second call starts from the work buffer the first one left
        L.call("sd_live_select", md.data_ptr(), h, w, work.data_ptr(), sel.data_ptr(), code.data_ptr(), _s())
    torch.cuda.synchronize()
    assert not work.any()
    s = sel.cpu().numpy()
    return int(s[:1].view(np.uint32)[0]), s[1:5], s[5:7], code.cpu().numpy()


def _percentiles64(m):
    """lo, hi as the select defines them: float32 of the fp64 linear interpolation between the order statistics
    around (n - 1) * q. (np.percentile of a float32 array computes (n - 1) * q in float32, which at tens of thousands
    of values moves the interpolation weight by up to 2^-9: it is the reference only on the fixture's small maps.)"""
    v = np.sort(m[np.isfinite(m) & (m > 0.0)]).astype(np.float64)
    out = []
    for q in (0.02, 0.98):
        vi = (v.size - 1) * q
        k = int(np.floor(vi))
        a, b = v[k], v[min(k + 1, v.size - 1)]
        out.append(a + (b - a) * (vi - k))
    return np.asarray(out, dtype=np.float32)


def _check_select(m, lohi_want):
    n, stats, lohi, code = _select(m)
    v = np.sort(m[np.isfinite(m) & (m > 0.0)])
    assert n == v.size
    if n == 0:
        assert np.isnan(stats).all() and np.isnan(lohi).all() and not code.any()
        return
    idx = []
    for q in (0.02, 0.98):
        k = int(np.floor((n - 1) * q))
        idx += [k, min(k + 1, n - 1)]
    _assert_bit_equal(stats, v[idx])
    assert _ulp_diff(lohi, lohi_want) <= 1
    assert np.array_equal(code, R.codes(m, lohi[0], lohi[1]))


@pytest.mark.parametrize("name", ["disp", "dup", "invalid", "one", "two"])
def test_select_on_the_fixture(gold, name):
    m = gold[f"auto/{name}/in"]
    n_valid = int((np.isfinite(m) & (m > 0.0)).sum())
    assert {"invalid": 0, "one": 1, "two": 2}.get(name, n_valid) == n_valid
    if name == "dup":  # duplicates around both percentiles
        v = np.sort(m[np.isfinite(m) & (m > 0.0)])
        for q in (0.02, 0.98):
            k = int(np.floor((v.size - 1) * q))
            assert v[k - 1] == v[k] == v[k + 1]
    _check_select(m, gold[f"auto/{name}/lohi"])


def test_select_many_blocks():
    """More values than one block takes (160 x 200 = 31 blocks), a wide dynamic range and a narrow one (all four
    ranks inside one level-1 bin: the shared-histogram path)."""
    rng = np.random.default_rng(3)
    for m in (np.exp(rng.normal(0.0, 3.0, (160, 200))).astype(np.float32),
              (5.0 + 1e-4 * rng.random((160, 200))).astype(np.float32)):
        m[rng.random(m.shape) < 0.05] = np.nan
        _check_select(m, _percentiles64(m))


# ---------------------------------------------------------------------- centre medians
@pytest.mark.parametrize("name", ["odd", "even", "small", "zero", "clipped", "empty"])
def test_center_medians_equal_the_reference(gold, name):
    m = gold[f"center/{name}/in"]
    window, want, count = gold[f"center/{name}/window_median_count"]
    md = _dev(m)
    out = torch.zeros(3, device=DEV)
    L.call("sd_live_center", md.data_ptr(), None, md.data_ptr(), H, W, int(window), out.data_ptr(), _s())
    got = out.cpu().numpy()
    assert np.isnan(got[1])  # no depth map
    if count == 0:
        assert np.isnan(want) and np.isnan(got[0]) and np.isnan(got[2])
    else:
        assert got[0] == np.float32(want) and got[2] == np.float32(want) and float(np.float32(want)) == want


# ---------------------------------------------------------------------- compose
def _compose(code_a, lut_a, code_b, lut_b, edge, view, Hc, Wc):
    d = {k: _dev(v) for k, v in dict(ca=code_a, la=lut_a, cb=code_b, lb=lut_b, e=edge, v=view).items()}
    va, vb, lv = (torch.zeros(Hc, Wc, 3, dtype=torch.uint8, device=DEV) for _ in range(3))
    L.call("sd_live_compose", L.ptr(d["ca"]), L.ptr(d["la"]), va.data_ptr() if code_a is not None else None,
           L.ptr(d["cb"]), L.ptr(d["lb"]), vb.data_ptr() if code_b is not None else None, L.ptr(d["e"]), L.ptr(d["v"]),
           lv.data_ptr() if view is not None else None, H, W, Hc, Wc, _s())
    torch.cuda.synchronize()
    return va.cpu().numpy(), vb.cpu().numpy(), lv.cpu().numpy()


@pytest.mark.parametrize("Hc,Wc", [(37, 53), (32, 48), (64, 96), (16, 24)])
def test_compose(Hc, Wc):
    rng = np.random.default_rng(Hc)
    code_a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    code_b = rng.integers(0, 256, (H, W), dtype=np.uint8)
    lut_a = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    lut_b = live.colormap_lut("viridis")
    edge = (rng.random((H, W)) < 0.2).astype(np.uint8) * 255
    view = rng.integers(0, 256, (Hc, Wc, 3), dtype=np.uint8)
    va, vb, lv = _compose(code_a, lut_a, code_b, lut_b, edge, view, Hc, Wc)
    assert np.abs(va.astype(int) - R.compose(code_a, lut_a, Hc, Wc).astype(int)).max() <= 1
    assert np.abs(vb.astype(int) - R.compose(code_b, lut_b, Hc, Wc).astype(int)).max() <= 1
    if (Hc, Wc) == (H, W):
        assert np.array_equal(va, lut_a[code_a]) and np.array_equal(vb, lut_b[code_b])
    on = R.nearest_mask(edge, Hc, Wc) > 0
    want = np.where(on[..., None], np.array([0, 255, 0], dtype=np.uint8), view)
    assert np.array_equal(lv, want) and on.any() and not on.all()
    # each output alone; a left view without a mask is the view
    va1, _, _ = _compose(code_a, lut_a, None, None, None, None, Hc, Wc)
    assert np.array_equal(va1, va)
    _, _, lv1 = _compose(None, None, None, None, None, view, Hc, Wc)
    assert np.array_equal(lv1, view)


# ---------------------------------------------------------------------- whole path
def _model(state, precision, base=8):
    from stereo_depth_estimation_amd.model import StereoUNet

    m = StereoUNet(base_channels=base, precision=precision)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state.items()})
    return m.to(DEV).eval()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp8"])
def test_step_equals_model_on_the_front_end_output(precision):
    Hc, Wc = 37, 53
    rng = np.random.default_rng(11)
    ml, mr = R.random_maps(rng, Hc, Wc), R.random_maps(rng, Hc, Wc)
    rect = live.Rectification(ml[0], ml[1], mr[0], mr[1], (Wc, Hc), 60.0, 0.1)
    st, st2 = U.make_state(8, seed=0), U.make_state(8, seed=1)
    m_live, m_ref = _model(st, precision), _model(st, precision)
    ld = live.LiveDepth(m_live, (W, H), rectification=rect, center_window=15)
    assert ld.depth_enabled
    fb = float(ld.focal_length_px_model) * 0.1

    def frame_pair(frames=None):
        fl, fr = frames or _frames(rng, Hc, Wc)
        with torch.inference_mode():
            res = ld.step(fl, fr)
            center = res.readout()
            _, b = _front(fl, fr, ml, mr)
            d, lv = m_ref(b, return_uncertainty=True)
        assert torch.equal(res.disparity, d[0, 0]) and torch.equal(res.logvar, lv[0, 0])
        post = _post(d[0, 0].cpu().numpy(), lv[0, 0].cpu().numpy(), fb=fb)
        assert torch.equal(res.confidence, post["conf"])
        assert torch.equal(res.depth_m.view(torch.int32), post["depth"].view(torch.int32))
        for i, t in enumerate((res.disparity, res.depth_m, res.confidence)):
            p = t.cpu().numpy()[9:24, 17:32]
            p = p[np.isfinite(p) & (p > 0.0)]
            assert center[i] == float(np.median(p))
        assert res.depth_vis.shape == (Hc, Wc, 3) and res.confidence_vis.shape == (Hc, Wc, 3)
        view = R.view_u8(fl, ml[0], ml[1])
        on = R.nearest_mask(_contours(res.depth_m), Hc, Wc) > 0
        lvw = res.left_view.cpu().numpy()
        assert np.array_equal(lvw[on], np.broadcast_to(np.array([0, 255, 0], dtype=np.uint8), lvw[on].shape))
        assert np.abs(lvw[~on].astype(int) - view[~on].astype(int)).max() <= 1
        return res.disparity.clone()

    fixed = _frames(rng, Hc, Wc)
    for _ in range(4):  # the first forward of a state, the graph capture, the replays
        frame_pair()
    d_old = frame_pair(fixed)
    for m in (m_live, m_ref):  # the live app reloads checkpoints
        m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st2.items()})
    d_new = frame_pair(fixed)
    assert not torch.equal(d_old, d_new)
    for _ in range(2):
        frame_pair()


def test_step_without_depth_uses_the_auto_range_and_device_frames():
    Hc, Wc = 16, 24
    rng = np.random.default_rng(5)
    m = _model(U.make_state(8, seed=2), "fp32")
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    ld = live.LiveDepth(m, (W, H), uncertainty=False, colormap=lut, ema_alpha=0.5, center_window=5)
    assert not ld.depth_enabled
    fl, fr = (_dev(f) for f in _frames(rng, Hc, Wc))
    with torch.inference_mode():
        res = ld.step(fl, fr)
        d1 = res.disparity.clone()
        _, b = _front(fl.cpu().numpy(), fr.cpu().numpy(), None, None)
        assert torch.equal(d1, m(b)[0, 0])  # the first frame after reset() is copied
        assert res.depth_m is None and res.confidence is None and res.confidence_vis is None and res.left_view is fl
        fl2, fr2 = (_dev(f) for f in _frames(rng, Hc, Wc))
        res = ld.step(fl2, fr2)
        _, b2 = _front(fl2.cpu().numpy(), fr2.cpu().numpy(), None, None)
        want = np.float32(0.5) * m(b2)[0, 0].cpu().numpy() + np.float32(0.5) * d1.cpu().numpy()
        _assert_bit_equal(res.disparity.cpu().numpy(), want)
        c = res.readout()
    assert np.isnan(c[1]) and np.isnan(c[2]) and c[0] > 0
    disp = res.disparity.cpu().numpy()
    got = ld._batch._buf["sel"][0].cpu().numpy()[5:7]
    assert _ulp_diff(got, _percentiles64(disp)) <= 1
    want_vis = R.compose(R.codes(disp, got[0], got[1]), lut, Hc, Wc)
    assert np.abs(res.depth_vis.cpu().numpy().astype(int) - want_vis.astype(int)).max() <= 1
    ld.reset()
    with torch.inference_mode():
        assert torch.equal(ld.step(fl2, fr2).disparity, m(b2)[0, 0])


def test_fp8_range_policy_is_shared_between_the_two_ways_of_feeding():
    """A dark-to-bright frame sequence (as test_gpu_fp8's recalibration test): the static fp8 path's calibration and
    range-recalibration counters, and the outputs, are the same whether the engine is fed by LiveDepth.step or by
    model(x) on the front end's NCHW output."""
    hm, wm = 240, 320
    rng = np.random.default_rng(9)
    st = U.make_state(32, seed=5)
    m_live, m_ref = _model(st, "fp8", 32), _model(st, "fp8", 32)
    ld = live.LiveDepth(m_live, (wm, hm))
    dark = [tuple((f // 5) for f in _frames(rng, hm, wm)) for _ in range(3)]
    bright = [_frames(rng, hm, wm) for _ in range(3)]
    e_live, e_ref = m_live.engine(), m_ref.engine()
    seen = []
    with torch.inference_mode():
        for fl, fr in dark + bright:
            res = ld.step(fl, fr)
            _, b = _front(fl, fr, None, None, h=hm, w=wm)
            d, lv = m_ref(b, return_uncertainty=True)
            torch.cuda.synchronize()
            assert torch.equal(res.disparity, d[0, 0]) and torch.equal(res.logvar, lv[0, 0])
            assert (e_live.fp8_calibrations, e_live.fp8_range_recalibrations) == \
                (e_ref.fp8_calibrations, e_ref.fp8_range_recalibrations)
            seen.append((e_live.fp8_calibrations, e_live.fp8_range_recalibrations))
    # calibrated on the first dark frame; the first bright frame is flagged, the second recalibrates
    assert seen == [(1, 0), (1, 0), (1, 0), (1, 0), (2, 1), (2, 1)], seen
