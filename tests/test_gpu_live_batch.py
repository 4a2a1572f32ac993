"""The multi-stream live frame path on the device (the sd_live_*_n entry points, LiveDepthBatch; needs an MI355X).

Every comparison is bit-equality against code that exists without the batch: stream i of a batched entry point against
the single-stream entry point run on stream i's data (its own, aligned tensors: at odd H * W the batched call's slices
1.. start misaligned and take the scalar kernels while the single-stream call may take the vector ones), and
LiveDepthBatch.step against model(x) on the front end's NCHW output for the batch. The two tolerant agreements (colour
images within 1 code of the NumPy composition, the percentile within 1 ulp) are test_gpu_live's.
"""

import numpy as np
import pytest
import torch

import live_ref as R
import test_gpu_live as T
from oracle import unet_ref as U
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import live

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = T.H, T.W  # 32 x 48
CAPTURES = [(37, 53), (16, 24)]
# 32 x 48: the four-elements-per-thread kernels; 5 x 7: H * W odd, slices 1 and 2 misaligned; 6 x 10: H * W = 60, the
# vector post with the scalar contour kernel
MODEL_SIZES = [(32, 48), (5, 7), (6, 10)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _s():
    return L.stream_handle()


def _eq(a, b):
    """bit equality of two tensors (NaN payloads included)"""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _maps_n(rng, count, Hc, Wc):
    """`count` map sets of one side: (map1 int16 [count, Hc, Wc, 2], map2 uint16 [count, Hc, Wc])"""
    sets = [R.random_maps(rng, Hc, Wc) for _ in range(count)]
    return np.stack([m[0] for m in sets]), np.stack([m[1] for m in sets])


# ---------------------------------------------------------------------- front end and rectified view
def _front_n(left, right, ml, mr, stride, dtype=L.SD_F32, amax=None, slot=0, clear=-1, h=H, w=W):
    n, Hc, Wc = left.shape[:3]
    keep = [T._dev(left), T._dev(right)] + [T._dev(m) for m in (ml or (None, None)) + (mr or (None, None))]
    xin = torch.empty(n * h * w * 8, dtype=torch.bfloat16 if dtype == L.SD_BF16 else torch.float32, device=DEV)
    nchw = torch.empty(n, 6, h, w, dtype=torch.float32, device=DEV)
    L.call("sd_live_frontend_n", n, dtype, keep[0].data_ptr(), keep[1].data_ptr(), Hc, Wc, *[L.ptr(m) for m in keep[2:]],
           stride, h, w, xin.data_ptr(), nchw.data_ptr(), L.ptr(amax), slot, clear, _s())
    torch.cuda.synchronize()
    return xin, nchw


@pytest.mark.parametrize("maps", ["none", "shared", "per_stream"])
@pytest.mark.parametrize("h,w", [(32, 48), (5, 7)])
@pytest.mark.parametrize("Hc,Wc", CAPTURES)
@pytest.mark.parametrize("n", [1, 3])
def test_front_end_and_view_equal_the_single_stream_entries(n, Hc, Wc, h, w, maps):
    rng = np.random.default_rng(1000 * n + Hc + h)
    left = rng.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)
    left[n - 1] //= 3  # the brightest stream is not the last one: the amax is over all
    right[n - 1] //= 3
    count = {"none": 0, "shared": 1, "per_stream": n}[maps]
    ml = _maps_n(rng, count, Hc, Wc) if count else None
    mr = _maps_n(rng, count, Hc, Wc) if count else None
    stride = Hc * Wc if maps == "per_stream" else 0
    for dtype in (L.SD_F32, L.SD_BF16):
        iv = torch.int16 if dtype == L.SD_BF16 else torch.int32
        amax = torch.tensor([0, 123, 456], dtype=torch.int32, device=DEV)
        xin, nchw = _front_n(left, right, ml, mr, stride, dtype, amax=amax, slot=0, clear=1, h=h, w=w)
        xin = xin.view(iv).view(n, -1)
        peak = 0.0
        for i in range(n):
            k = i if maps == "per_stream" else 0
            mli = (ml[0][k], ml[1][k]) if ml else None
            mri = (mr[0][k], mr[1][k]) if mr else None
            a1 = torch.zeros(3, dtype=torch.int32, device=DEV)
            x1, b1 = T._front(left[i], right[i], mli, mri, dtype, amax=a1, h=h, w=w)
            assert torch.equal(xin[i], x1.view(iv)), (dtype, i)
            assert _eq(nchw[i], b1[0]), (dtype, i)
            peak = max(peak, float(a1[:1].view(torch.float32).item()))
        a = amax.cpu().numpy()
        assert a[:1].view(np.float32)[0] == np.float32(peak) and a[1] == 0 and a[2] == 456
        ref = torch.empty_like(xin)  # the engine's batch-n input of the NCHW output
        L.call("sd_pack_input", dtype, nchw.data_ptr(), n, 6, h, w, 8, ref.data_ptr(), _s())
        torch.cuda.synchronize()
        assert torch.equal(xin, ref)
        xin2, _ = _front_n(left, right, ml, mr, stride, dtype, h=h, w=w)  # without amax: nothing but the pack
        assert torch.equal(xin2.view(iv).view(n, -1), xin)
    if ml:
        views = torch.empty(n, Hc, Wc, 3, dtype=torch.uint8, device=DEV)
        d = [T._dev(left), T._dev(ml[0]), T._dev(ml[1])]
        L.call("sd_live_rectify_n", n, d[0].data_ptr(), Hc, Wc, d[1].data_ptr(), d[2].data_ptr(), stride,
               views.data_ptr(), _s())
        for i in range(n):
            k = i if maps == "per_stream" else 0
            v1 = torch.empty(Hc, Wc, 3, dtype=torch.uint8, device=DEV)
            one = [T._dev(left[i]), T._dev(ml[0][k]), T._dev(ml[1][k])]
            L.call("sd_live_rectify", one[0].data_ptr(), Hc, Wc, one[1].data_ptr(), one[2].data_ptr(), v1.data_ptr(), _s())
            assert torch.equal(views[i], v1), i


# ---------------------------------------------------------------------- the stages after the heads
DLO, DSCALE, CLO, CSCALE = 0.0, float(np.float32(10.0)), 0.0, float(np.float32(5.0))
ALPHA = 0.3
WINDOW = 5


class Chain:
    """Buffers of n streams and every stage after the heads: post, contours, the auto-range select (on the EMA state,
    into a code plane of its own), the centre medians and the images, by the batched entry points (batched = True) or
    by the single-stream ones (n = 1)."""

    def __init__(self, n, h, w, Hc, Wc, depth_on, batched, seed=0):
        assert batched or n == 1
        self.n, self.h, self.w, self.Hc, self.Wc, self.on, self.batched = n, h, w, Hc, Wc, depth_on, batched
        g = torch.Generator().manual_seed(seed)  # the initial contents are arbitrary, and identical for both forms

        def f32(*shape):
            return torch.randn(*shape, generator=g).to(DEV)

        def u8(*shape):
            return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(DEV)

        self.b = {"state": f32(n, h, w), "depth": f32(n, h, w), "conf": f32(n, h, w), "dcode": u8(n, h, w),
                  "ccode": u8(n, h, w), "edge": u8(n, h, w), "acode": u8(n, h, w), "sel": f32(n, 8),
                  "center": f32(n, 3), "vis_a": u8(n, Hc, Wc, 3), "vis_b": u8(n, Hc, Wc, 3), "vis_c": u8(n, Hc, Wc, 3),
                  "left_view": u8(n, Hc, Wc, 3)}
        words = L.call("sd_live_select_n_ws_bytes", n) if batched else L.call("sd_live_select_ws_bytes")
        self.ws = torch.zeros(words // 4, dtype=torch.int32, device=DEV)
        self.lut_a = T._dev(live.colormap_lut("turbo"))
        self.lut_b = T._dev(live.colormap_lut("viridis"))

    def run(self, disp, logvar, view, fb, copy_mask=0, hold_mask=0):
        """disp, logvar f32 [n, h, w]; view u8 [n, Hc, Wc, 3]; fb f32 [n] (device tensors)"""
        b, n, h, w, Hc, Wc, on = self.b, self.n, self.h, self.w, self.Hc, self.Wc, self.on
        p = {k: v.data_ptr() for k, v in b.items()}
        a, oma = float(np.float32(ALPHA)), float(np.float32(1.0 - ALPHA))
        if self.batched:
            L.call("sd_live_post_n", n, disp.data_ptr(), logvar.data_ptr(), h, w, p["state"], copy_mask, hold_mask, a, oma,
                   int(on), fb.data_ptr() if on else None, p["depth"] if on else None, p["conf"],
                   p["dcode"] if on else None, DLO, DSCALE, p["ccode"], CLO, CSCALE, _s())
            if on:
                L.call("sd_live_contours_n", n, p["depth"], h, w, 0.0, 10.0, 0.5, p["edge"], hold_mask, _s())
            L.call("sd_live_select_n", n, p["state"], h, w, self.ws.data_ptr(), p["sel"], p["acode"], hold_mask, _s())
            L.call("sd_live_center_n", n, p["state"], p["depth"] if on else None, p["conf"], h, w, WINDOW, p["center"],
                   hold_mask, _s())
            L.call("sd_live_compose_n", n, p["dcode"] if on else p["acode"], self.lut_a.data_ptr(), p["vis_a"], p["ccode"],
                   self.lut_b.data_ptr(), p["vis_b"], p["edge"] if on else None, view.data_ptr() if on else None,
                   p["left_view"] if on else None, h, w, Hc, Wc, hold_mask, _s())
            L.call("sd_live_compose_n", n, p["acode"], self.lut_a.data_ptr(), p["vis_c"], None, None, None, None, None,
                   None, h, w, Hc, Wc, hold_mask, _s())
        elif not hold_mask & 1:
            L.call("sd_live_post", disp.data_ptr(), logvar.data_ptr(), h, w, p["state"], copy_mask & 1, a, oma, int(on),
                   float(fb[0]) if on else 0.0, p["depth"] if on else None, p["conf"], p["dcode"] if on else None, DLO,
                   DSCALE, p["ccode"], CLO, CSCALE, _s())
            if on:
                L.call("sd_live_contours", p["depth"], h, w, 0.0, 10.0, 0.5, p["edge"], _s())
            L.call("sd_live_select", p["state"], h, w, self.ws.data_ptr(), p["sel"], p["acode"], _s())
            L.call("sd_live_center", p["state"], p["depth"] if on else None, p["conf"], h, w, WINDOW, p["center"], _s())
            L.call("sd_live_compose", p["dcode"] if on else p["acode"], self.lut_a.data_ptr(), p["vis_a"], p["ccode"],
                   self.lut_b.data_ptr(), p["vis_b"], p["edge"] if on else None, view.data_ptr() if on else None,
                   p["left_view"] if on else None, h, w, Hc, Wc, _s())
            L.call("sd_live_compose", p["acode"], self.lut_a.data_ptr(), p["vis_c"], None, None, None, None, None, None,
                   h, w, Hc, Wc, _s())
        torch.cuda.synchronize()
        assert not self.ws.any()  # the select leaves its workspace zero, for every stream

    def written(self):
        """the outputs the configuration writes (sel: its 7 words)"""
        skip = () if self.on else ("depth", "dcode", "edge", "left_view")
        return {k: (v[:, :7] if k == "sel" else v) for k, v in self.b.items() if k not in skip}


def _inputs(rng, n, h, w, Hc, Wc):
    """per-stream predictions with the invalid cases in them, views and geometry"""
    disp = rng.uniform(0.5, 40.0, (n, h, w)).astype(np.float32)
    disp[rng.random(disp.shape) < 0.08] = np.nan
    disp[rng.random(disp.shape) < 0.05] = -1.0
    disp[rng.random(disp.shape) < 0.03] = 1e-6  # the depth threshold itself: invalid
    logvar = rng.normal(0.0, 2.0, (n, h, w)).astype(np.float32)
    view = rng.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)
    fb = rng.uniform(5.0, 60.0, n).astype(np.float32)
    return T._dev(disp), T._dev(logvar), T._dev(view), T._dev(fb)


def _check_stream(batch, single, i, what):
    got, want = batch.written(), single.written()
    for k in want:
        assert _eq(got[k][i], want[k][0]), (what, "stream", i, k)


@pytest.mark.parametrize("depth_on", [True, False])
@pytest.mark.parametrize("h,w", MODEL_SIZES)
@pytest.mark.parametrize("n", [1, 3])
def test_stages_equal_the_single_stream_entries(n, h, w, depth_on):
    Hc, Wc = CAPTURES[(h + n) % 2]
    rng = np.random.default_rng(100 * h + n + depth_on)
    batch = Chain(n, h, w, Hc, Wc, depth_on, True, seed=1)
    singles = [Chain(1, h, w, Hc, Wc, depth_on, False, seed=1 + i) for i in range(n)]
    for k, v in batch.b.items():  # the same (arbitrary) previous state
        for i in range(n):
            singles[i].b[k][0].copy_(v[i])
    copy_mask = 0b010 if n == 3 else 0  # n = 1 "with no masks": the EMA branch
    for step in range(2):  # the second call starts from what the first one left
        disp, logvar, view, fb = _inputs(rng, n, h, w, Hc, Wc)
        batch.run(disp, logvar, view, fb, copy_mask=copy_mask)
        for i in range(n):
            singles[i].run(disp[i:i + 1].clone(), logvar[i:i + 1].clone(), view[i:i + 1].clone(), fb[i:i + 1],
                           copy_mask=(copy_mask >> i) & 1)
            _check_stream(batch, singles[i], i, f"step {step}")
    assert batch.b["edge"].any() or not depth_on


@pytest.mark.parametrize("depth_on", [True, False])
@pytest.mark.parametrize("h,w", [(32, 48), (5, 7)])
def test_masks_over_a_three_step_sequence(h, w, depth_on):
    n, (Hc, Wc) = 3, CAPTURES[0]
    rng = np.random.default_rng(7 * h + depth_on)
    batch = Chain(n, h, w, Hc, Wc, depth_on, True, seed=3)
    singles = [Chain(1, h, w, Hc, Wc, depth_on, False, seed=4 + i) for i in range(n)]
    #        copy    hold
    plan = [(0b111, 0b000),   # first frames
            (0b001, 0b010),   # stream 0 reset, stream 1 without a frame
            (0b100, 0b001)]   # stream 2 reset, stream 0 without a frame
    for step, (copy_mask, hold_mask) in enumerate(plan):
        disp, logvar, view, fb = _inputs(rng, n, h, w, Hc, Wc)
        before = {k: v.clone() for k, v in batch.b.items()}
        batch.run(disp, logvar, view, fb, copy_mask=copy_mask, hold_mask=hold_mask)
        for i in range(n):
            if (hold_mask >> i) & 1:  # every buffer of a held stream, written by this configuration or not
                for k, v in batch.b.items():
                    assert _eq(v[i], before[k][i]), ("held", step, i, k)
                continue
            singles[i].run(disp[i:i + 1].clone(), logvar[i:i + 1].clone(), view[i:i + 1].clone(), fb[i:i + 1],
                           copy_mask=(copy_mask >> i) & 1)
            _check_stream(batch, singles[i], i, f"step {step}")
            if (copy_mask >> i) & 1:
                assert _eq(batch.b["state"][i], disp[i])
            else:
                assert not _eq(batch.b["state"][i], disp[i])


def test_select_with_an_empty_stream_next_to_a_large_one():
    """Stream 0 has no finite positive value (NaN, zero codes); stream 1 has 160 x 200 values (31 blocks) of a wide range;
    stream 2 a single valid value."""
    h, w, n = 160, 200, 3
    rng = np.random.default_rng(3)
    m = np.empty((n, h, w), dtype=np.float32)
    m[0] = rng.choice(np.array([np.nan, -1.0, 0.0, -np.inf, np.inf], dtype=np.float32), (h, w))
    m[1] = np.exp(rng.normal(0.0, 3.0, (h, w)))
    m[1][rng.random((h, w)) < 0.05] = np.nan
    m[2] = np.nan
    m[2, 77, 5] = 3.25
    md = T._dev(m)
    work = torch.zeros(L.call("sd_live_select_n_ws_bytes", n) // 4, dtype=torch.int32, device=DEV)
    sel = torch.zeros(n, 8, device=DEV)
    code = torch.full((n, h, w), 9, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        L.call("sd_live_select_n", n, md.data_ptr(), h, w, work.data_ptr(), sel.data_ptr(), code.data_ptr(), 0, _s())
    torch.cuda.synchronize()
    assert not work.any()
    s = sel.cpu().numpy()
    assert s[0, :1].view(np.uint32)[0] == 0 and np.isnan(s[0, 1:7]).all() and not code[0].any()
    assert s[2, :1].view(np.uint32)[0] == 1 and (s[2, 1:7] == np.float32(3.25)).all()
    for i in range(n):
        cnt, stats, lohi, code1 = T._select(m[i])
        assert s[i, :1].view(np.uint32)[0] == cnt
        T._assert_bit_equal(s[i, 1:5], stats)
        T._assert_bit_equal(s[i, 5:7], lohi)
        assert np.array_equal(code[i].cpu().numpy(), code1)
    assert T._ulp_diff(s[1, 5:7], T._percentiles64(m[1])) <= 1
    # a held stream's sel row, codes and workspace words are untouched
    sel.fill_(7.0)
    code.fill_(9)
    L.call("sd_live_select_n", n, md.data_ptr(), h, w, work.data_ptr(), sel.data_ptr(), code.data_ptr(), 0b010, _s())
    torch.cuda.synchronize()
    assert (sel[1] == 7.0).all() and (code[1] == 9).all() and not work.any()
    T._assert_bit_equal(sel[2, 1:7].cpu().numpy(), s[2, 1:7])
    assert np.isnan(sel[0, 1:7].cpu().numpy()).all() and not code[0].any()


# ---------------------------------------------------------------------- whole path
def _rects(rng, n, Hc, Wc):
    out = []
    for i in range(n):
        ml, mr = R.random_maps(rng, Hc, Wc), R.random_maps(rng, Hc, Wc)
        out.append(live.Rectification(ml[0], ml[1], mr[0], mr[1], (Wc, Hc), 60.0 + 10.0 * i, 0.1 + 0.05 * i))
    return out


def _frames_n(rng, n, Hc, Wc):
    return (rng.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8), rng.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8))


def _front_of(ld, rects, fl, fr):
    """the front end's NCHW output for the batch, by the batched entry point"""
    Hc, Wc = fl.shape[1:3]
    if rects is None:
        return _front_n(fl, fr, None, None, 0)[1]
    ml = (np.stack([r.map_l_1 for r in rects]), np.stack([r.map_l_2 for r in rects]))
    mr = (np.stack([r.map_r_1 for r in rects]), np.stack([r.map_r_2 for r in rects]))
    return _front_n(fl, fr, ml, mr, Hc * Wc)[1]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp8"])
def test_step_equals_model_on_the_front_end_output(precision):
    n, (Hc, Wc) = 3, CAPTURES[0]
    rng = np.random.default_rng(11)
    rects = _rects(rng, n, Hc, Wc)
    st, st2 = U.make_state(8, seed=0), U.make_state(8, seed=1)
    m_live, m_ref = T._model(st, precision), T._model(st, precision)
    ld = live.LiveDepthBatch(m_live, n, (W, H), rectification=rects, center_window=15)
    assert ld.depth_enabled and not ld.shared_maps
    fbs = [float(ld.focal_length_px_model[i]) * float(ld.baseline_m[i]) for i in range(n)]
    assert len(set(fbs)) == n

    def step(frames=None):
        fl, fr = frames or _frames_n(rng, n, Hc, Wc)
        with torch.inference_mode():
            res = ld.step(fl, fr)
            center = res.readout()
            b = _front_of(ld, rects, fl, fr)
            d, lv = m_ref(b, return_uncertainty=True)
        assert center.shape == (n, 3) and center.dtype == np.float32
        assert torch.equal(res.disparity, d[:, 0]) and torch.equal(res.logvar, lv[:, 0])
        for i in range(n):
            post = T._post(d[i, 0].cpu().numpy(), lv[i, 0].cpu().numpy(), fb=fbs[i])
            assert torch.equal(res.confidence[i], post["conf"])
            assert torch.equal(res.depth_m[i].view(torch.int32), post["depth"].view(torch.int32))
            for j, t in enumerate((res.disparity, res.depth_m, res.confidence)):
                p = t[i].cpu().numpy()[9:24, 17:32]
                p = p[np.isfinite(p) & (p > 0.0)]
                assert center[i, j] == np.float32(np.median(p))
            view = R.view_u8(fl[i], rects[i].map_l_1, rects[i].map_l_2)
            on = R.nearest_mask(T._contours(res.depth_m[i].clone()), Hc, Wc) > 0
            lvw = res.left_view[i].cpu().numpy()
            assert np.array_equal(lvw[on], np.broadcast_to(np.array([0, 255, 0], dtype=np.uint8), lvw[on].shape))
            assert np.abs(lvw[~on].astype(int) - view[~on].astype(int)).max() <= 1
        assert res.depth_vis.shape == (n, Hc, Wc, 3) and res.confidence_vis.shape == (n, Hc, Wc, 3)
        return res.disparity.clone()

    fixed = _frames_n(rng, n, Hc, Wc)
    for _ in range(4):  # the first forward of a state, the graph capture, the replays
        step()
    d_old = step(fixed)
    assert not torch.equal(d_old[0], d_old[1]) and not torch.equal(d_old[1], d_old[2])
    for m in (m_live, m_ref):  # the live app reloads checkpoints
        m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st2.items()})
    d_new = step(fixed)
    assert not torch.equal(d_old, d_new)
    for _ in range(2):
        step()


def test_step_allocates_nothing_after_the_first_and_launches_the_same_for_any_n(monkeypatch):
    Hc, Wc = CAPTURES[1]
    rng = np.random.default_rng(2)
    # torch creates the default generator's graph-safe seed / offset tensors (2 x 512 B) at the first graph capture
    # of a process, whoever captures: have the engine capture once (the second eval forward of an unchanged state)
    # before memory is compared, so that the comparison below is exact and about the step alone
    warm = T._model(U.make_state(8, seed=3), "fp32")
    with torch.inference_mode():
        for _ in range(3):
            warm(torch.rand(1, 6, H, W, device=DEV))
    names = []
    real = L.call

    def counting(name, *args):
        names.append(name)
        return real(name, *args)

    per_n = {}
    for n in (1, 5):
        m = T._model(U.make_state(8, seed=2), "fp32")  # a model of its own: the same history of forwards for each n
        ld = live.LiveDepthBatch(m, n, (W, H), rectification=_rects(rng, 1, Hc, Wc)[0])  # shared maps
        assert ld.shared_maps and ld.depth_enabled
        steps = []
        with torch.inference_mode():
            for k in range(4):  # first forward, capture, replays
                fl, fr = _frames_n(rng, n, Hc, Wc)
                if k == 1:
                    torch.cuda.synchronize()
                    before = torch.cuda.memory_allocated()
                monkeypatch.setattr(L, "call", counting)
                names.clear()
                res = ld.step(list(fl), list(fr)) if k == 3 else ld.step(fl, fr)  # a sequence of frames too
                monkeypatch.setattr(L, "call", real)
                steps.append([x for x in names if not x.endswith(("_rows", "_splits", "_ok", "_bytes"))])
                if k == 1:
                    torch.cuda.synchronize()
                    assert torch.cuda.memory_allocated() == before
                out = res.readout()
                assert out.shape == (n, 3) and out.dtype == np.float32 and np.isfinite(out[:, 0]).all()
        per_n[n] = steps
        tail = steps[-1][steps[-1].index("sd_live_rectify_n"):]
        assert tail == ["sd_live_rectify_n", "sd_live_post_n", "sd_live_contours_n", "sd_live_center_n", "sd_live_compose_n"]
    assert per_n[1] == per_n[5]
    assert per_n[1][-1].count("sd_live_frontend_n") == 1 and len(per_n[1][-1]) < len(per_n[1][0])  # the graph replays


def test_reset_of_one_stream_hold_and_the_auto_range():
    n, (Hc, Wc) = 3, CAPTURES[1]
    rng = np.random.default_rng(5)
    m = T._model(U.make_state(8, seed=2), "fp32")
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    ld = live.LiveDepthBatch(m, n, (W, H), uncertainty=False, colormap=lut, ema_alpha=0.5, center_window=5)
    assert not ld.depth_enabled
    half = np.float32(0.5)

    def pred(fl, fr):
        return m(_front_of(ld, None, fl.cpu().numpy(), fr.cpu().numpy()))[:, 0].cpu().numpy()

    with torch.inference_mode():
        fl, fr = (T._dev(f) for f in _frames_n(rng, n, Hc, Wc))
        with pytest.raises(ValueError, match="first step must be fresh"):
            ld.step(fl, fr, fresh=[True, False, True])
        res = ld.step(fl, fr)  # device frames; the first frame of every stream is copied
        assert res.depth_m is None and res.confidence is None and res.confidence_vis is None and res.left_view is fl
        s0 = res.disparity.cpu().numpy()
        T._assert_bit_equal(s0, pred(fl, fr))
        fl, fr = (T._dev(f) for f in _frames_n(rng, n, Hc, Wc))
        s1 = ld.step(fl, fr).disparity.cpu().numpy()
        T._assert_bit_equal(s1, half * pred(fl, fr) + half * s0)
        ld.reset(stream=1)  # only stream 1's next frame is a copy
        fl, fr = (T._dev(f) for f in _frames_n(rng, n, Hc, Wc))
        s2 = ld.step(fl, fr).disparity.cpu().numpy()
        p2 = pred(fl, fr)
        T._assert_bit_equal(s2[1], p2[1])
        T._assert_bit_equal(s2[[0, 2]], (half * p2 + half * s1)[[0, 2]])
        # stream 1 held: nothing of it moves, the others go on
        fl, fr = (T._dev(f) for f in _frames_n(rng, n, Hc, Wc))
        keep = {k: ld._buf[k][1].clone() for k in ("state", "dcode", "depth_vis", "sel", "center")}
        res = ld.step(fl, fr, fresh=[True, False, True])
        c = res.readout()
        s3 = res.disparity.cpu().numpy()
        for k, v in keep.items():
            assert _eq(ld._buf[k][1], v), k
        p3 = pred(fl, fr)
        T._assert_bit_equal(s3[[0, 2]], (half * p3 + half * s2)[[0, 2]])
        T._assert_bit_equal(s3[1], s2[1])
        assert not ld._buf["sel_ws"].any()
    assert c.shape == (n, 3) and np.isnan(c[:, 1:]).all() and (c[:, 0] > 0).all()
    for i in range(n):  # each stream's colours in its own 2nd..98th percentile range
        got = ld._buf["sel"][i].cpu().numpy()[5:7]
        assert T._ulp_diff(got, T._percentiles64(s3[i])) <= 1
        want_vis = R.compose(R.codes(s3[i], got[0], got[1]), lut, Hc, Wc)
        assert np.abs(res.depth_vis[i].cpu().numpy().astype(int) - want_vis.astype(int)).max() <= 1
    ld.reset()
    with torch.inference_mode():
        T._assert_bit_equal(ld.step(fl, fr).disparity.cpu().numpy(), p3)
