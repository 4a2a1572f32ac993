"""Several stereo rigs through one semi-global matcher step (csrc/sgm.hip: the stream as a grid dimension of the
single-stream kernels; sd_sgm_compute_n, sd_sgm_speckle_n, sd_sgm_post_n, sd_sgm_center_n; StereoSGM.compute_batch,
ClassicDepthBatch; needs an MI355X).

Every stream of a batch must give the bytes of the single-stream path on that stream's pair: array_equal to the NumPy
restatements (tests/sgm_ref.py, tests/sgm_modes_ref.py) and torch.equal to the single-stream entry points. Every
stream gets a scene of its own (another seed and another shift), so a slice read from the wrong stream shows.
"""

import numpy as np
import pytest
import torch

import live_ref
import sgm_modes_ref as M
import sgm_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import live, sgm

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 3

# (H, W, D, minD, bs)
CASES = [
    (9, 41, 16, 0, 3),       # odd H * W: every stream slice of gray and q is misaligned
    (17, 150, 48, 3, 5),     # D not a multiple of 64, minD > 0
    (33, 200, 128, 0, 7),    # the app's settings
    (12, 300, 256, 0, 7),    # four values per lane
    (10, 17, 16, 0, 3),      # one column right of maxD
    (8, 20, 32, 0, 7),       # W < maxD: everything invalid, nothing written
]
APP_CASE = CASES[2]
MODE_NAMES = ("3way", "hh4", "sgbm", "hh")
_ids = dict(ids=lambda c: "x".join(map(str, c)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _s():
    return L.stream_handle()


def _modes(case):
    return MODE_NAMES if case == APP_CASE else ("3way", "hh")


def _params(case):
    H, W, D, minD, bs = case
    return R.Params(min_disparity=minD, num_disparities=D, block_size=bs,
                    speckle_window_size=100 if case == APP_CASE else 12)


def _scene(case, stream, salt=0):
    H, W, D, minD, bs = case
    rng = np.random.default_rng(1000 * H + W + 100003 * stream + 7919 * salt)
    left, right = R.shifted_bgr_scene(rng, H, W, minD + D // 3 + stream + salt, noise=12)
    return R.gray(left), R.gray(right)


_refs = {}


def _ref(case, stream, salt=0):
    """Stream `stream`'s gray pair of a case and every mode's int16 map of it: computed once, shared, read-only."""
    key = (case, stream, salt)
    if key not in _refs:
        gl, gr = _scene(case, stream, salt)
        ref = {"gray_l": gl, "gray_r": gr, "q": {m: M.compute(gl, gr, _params(case), m) for m in _modes(case)}}
        for a in [gl, gr, *ref["q"].values()]:
            a.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _args(case):
    H, W, D, minD, bs = case
    p = _params(case)
    return (H, W, minD, D, bs, p.P1, p.P2, p.max_diff, p.uniq, p.speckle_window, p.speckle_range, p.cap)


def _compute_n(case, mode, gl, gr, ws=None):
    H, W, D = case[:3]
    n = gl.shape[0]
    if ws is None:  # 0xFF everywhere: nothing may depend on what the workspace held
        ws = torch.full((L.call("sd_sgm_ws_bytes_n", n, H, W, D),), 0xFF, dtype=torch.uint8, device=DEV)
    q = torch.full((n, H, W), 0x5555, dtype=torch.int16, device=DEV)
    L.call("sd_sgm_compute_n", n, gl.data_ptr(), gr.data_ptr(), *_args(case), sgm.MODES[mode][0], ws.data_ptr(),
           q.data_ptr(), _s())
    return q, ws


def _compute_one(case, mode, gl, gr):
    H, W, D = case[:3]
    ws = torch.full((L.call("sd_sgm_ws_bytes", H, W, D),), 0xFF, dtype=torch.uint8, device=DEV)
    q = torch.empty((H, W), dtype=torch.int16, device=DEV)
    if mode == "3way":
        L.call("sd_sgm_compute", gl.data_ptr(), gr.data_ptr(), *_args(case), ws.data_ptr(), q.data_ptr(), _s())
    else:
        L.call("sd_sgm_compute_mode", gl.data_ptr(), gr.data_ptr(), *_args(case), sgm.MODES[mode][0], ws.data_ptr(),
               q.data_ptr(), _s())
    return q


# ---------------------------------------------------------------------- 1: the whole matcher
@pytest.mark.parametrize("case", CASES, **_ids)
def test_every_stream_equals_the_single_stream_matcher(case):
    H, W, D, minD, bs = case
    p = _params(case)
    refs = [_ref(case, i) for i in range(N)]
    gl = _dev(np.stack([r["gray_l"] for r in refs]))
    gr = _dev(np.stack([r["gray_r"] for r in refs]))
    for mode in _modes(case):
        q, _ = _compute_n(case, mode, gl, gr)
        m = sgm.StereoSGM(min_disparity=minD, num_disparities=D, block_size=bs, speckle_window_size=p.speckle_window,
                          mode=mode)
        qb = m.compute_batch(gl, gr)
        assert qb.dtype == torch.int16 and tuple(qb.shape) == (N, H, W)
        for i in range(N):
            assert np.array_equal(_np(q[i]), refs[i]["q"][mode]), (mode, i)
            assert torch.equal(q[i], _compute_one(case, mode, gl[i], gr[i])), (mode, i)
            assert torch.equal(qb[i], q[i]), (mode, i)
        # n = 1 is the single-stream entry point
        q1, _ = _compute_n(case, mode, gl[1:2], gr[1:2])
        assert torch.equal(q1[0], q[1]), mode
        assert torch.equal(m.compute_batch(gl[2:3], gr[2:3])[0], m.compute(gl[2], gr[2])), mode
    if W > p.maxD + 1:  # the streams are told apart, and the scenes are matched
        assert not np.array_equal(refs[0]["q"]["3way"], refs[1]["q"]["3way"])
        assert not np.array_equal(refs[1]["q"]["3way"], refs[2]["q"]["3way"])
        assert all((r["q"]["3way"][:, p.maxD:] != p.invalid).mean() >= 0.99 for r in refs)
    elif W <= p.maxD:
        assert all((r["q"]["3way"] == p.invalid).all() for r in refs)


def test_one_matcher_serves_one_pair_and_batches_from_one_workspace():
    """compute, compute_batch on 3 pairs and compute again on one StereoSGM object: after the first round (which grows
    the workspace to the batch's size) nothing is allocated, and every result is a fresh matcher's, bit for bit."""
    case = CASES[0]
    H, W, D, minD, bs = case
    kw = dict(min_disparity=minD, num_disparities=D, block_size=bs, speckle_window_size=_params(case).speckle_window)
    refs = [_ref(case, i) for i in range(N)]
    gl = _dev(np.stack([r["gray_l"] for r in refs]))
    gr = _dev(np.stack([r["gray_r"] for r in refs]))
    m = sgm.StereoSGM(**kw)
    allocated = []
    for _ in range(3):
        got = [m.compute(gl[0], gr[0]), m.compute_batch(gl, gr), m.compute(gl[2], gr[2])]
        torch.cuda.synchronize()
        allocated.append(torch.cuda.memory_allocated())
        assert m.workspace(gl.device, H, W).numel() == L.call("sd_sgm_ws_bytes_n", N, H, W, D)
        assert torch.equal(got[0], sgm.StereoSGM(**kw).compute(gl[0], gr[0]))
        assert torch.equal(got[1], sgm.StereoSGM(**kw).compute_batch(gl, gr))
        assert torch.equal(got[2], sgm.StereoSGM(**kw).compute(gl[2], gr[2]))
        assert tuple(got[0].shape) == (H, W) and tuple(got[1].shape) == (N, H, W)
        for i in range(N):
            assert np.array_equal(_np(got[1][i]), refs[i]["q"]["3way"]), i
    assert allocated[1] == allocated[0] and allocated[2] == allocated[0]


# ---------------------------------------------------------------------- 2: isolation
@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_a_stream_depends_on_its_own_pair_only(mode):
    case = APP_CASE
    refs = [_ref(case, i) for i in range(N)]
    gl = _dev(np.stack([r["gray_l"] for r in refs]))
    gr = _dev(np.stack([r["gray_r"] for r in refs]))
    q0, ws = _compute_n(case, mode, gl, gr)
    other = _ref(case, 1, salt=1)
    gl[1].copy_(_dev(other["gray_l"]))
    gr[1].copy_(_dev(other["gray_r"]))
    q1, _ = _compute_n(case, mode, gl, gr, ws=ws)  # the same workspace, as it was left
    assert torch.equal(q1[0], q0[0]) and torch.equal(q1[2], q0[2])
    assert np.array_equal(_np(q1[1]), other["q"][mode])
    assert not np.array_equal(other["q"][mode], refs[1]["q"][mode])


# ---------------------------------------------------------------------- 3: the speckle filter at a stream boundary
def test_speckle_components_never_join_across_streams():
    H, W, window, rng_range, invalid = 4, 70, 100, 2, -16
    q = np.full((2, H, W), invalid, dtype=np.int16)
    q[0, 3, :] = 160          # stream 0's last row
    q[1, 0, :] = 168          # stream 1's first row: within 16 * range of it
    q[0, 1, 60:68] = 160      # a run across column 64 (two segments of the init kernel), alone in its row
    want = np.stack([R.speckle(q[i], invalid, window, rng_range) for i in range(2)])
    stacked = R.speckle(q.reshape(2 * H, W), invalid, window, rng_range)
    assert (want != invalid).sum() == 0 and (stacked != invalid).sum() == 140  # what a joined boundary would keep
    t = _dev(q)
    per = L.call("sd_sgm_speckle_ws_bytes", H, W)
    work = torch.full((2 * per,), 0xFF, dtype=torch.uint8, device=DEV)
    L.call("sd_sgm_speckle_n", 2, t.data_ptr(), H, W, invalid, window, rng_range, work.data_ptr(), _s())
    assert np.array_equal(_np(t), want)
    # and each stream alone through the single-stream entry point
    for i in range(2):
        t1 = _dev(q[i])
        L.call("sd_sgm_speckle", t1.data_ptr(), H, W, invalid, window, rng_range, work.data_ptr(), _s())
        assert np.array_equal(_np(t1), want[i])
    # a smaller window keeps the rows (70 > 60) and removes the run (8): the filter did run, per stream
    want60 = np.stack([R.speckle(q[i], invalid, 60, rng_range) for i in range(2)])
    assert (want60 != invalid).sum() == 140
    t = _dev(q)
    L.call("sd_sgm_speckle_n", 2, t.data_ptr(), H, W, invalid, 60, rng_range, work.data_ptr(), _s())
    assert np.array_equal(_np(t), want60)


# ---------------------------------------------------------------------- 4: post stage and centre distance
@pytest.fixture(scope="module")
def calib_Q(golden_dir):
    with np.load(golden_dir / "sgm_calib.npz") as d:
        return np.array(d["Q"], dtype=np.float64)


def _assert_bit_equal(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_post_and_center_per_stream(calib_Q):
    H, W, window = 31, 45, 15
    rng = np.random.default_rng(5)
    q = rng.integers(-40, 2000, (N, H, W)).astype(np.int16)
    q[rng.random(q.shape) < 0.3] = -16
    q[1] = -16                                   # stream 1: nothing valid
    q[2, H // 2 - 7:H // 2 + 8, W // 2 - 7:W // 2 + 8] = -16  # stream 2: an all-NaN centre patch
    Qs = np.stack([calib_Q, 2.0 * calib_Q, 0.5 * calib_Q])
    Qs[1, 3, 0], Qs[1, 3, 1], Qs[1, 2, 0], Qs[1, 3, 3] = 0.013, -0.007, 0.21, 0.5
    Qs[2, 3, 0], Qs[2, 2, 1] = -0.002, 0.4
    qd, Qd = _dev(q), _dev(Qs.reshape(N, 16))
    disp = torch.empty((N, H, W), dtype=torch.float32, device=DEV)
    z = torch.empty((N, H, W), dtype=torch.float32, device=DEV)
    code = torch.full((N, H, W), 77, dtype=torch.uint8, device=DEV)
    mm = torch.full((N, 2), 123, dtype=torch.int32, device=DEV)
    c = torch.zeros(N, dtype=torch.float32, device=DEV)
    L.call("sd_sgm_post_n", N, qd.data_ptr(), H, W, Qd.data_ptr(), disp.data_ptr(), z.data_ptr(), code.data_ptr(),
           mm.data_ptr(), _s())
    L.call("sd_sgm_center_n", N, z.data_ptr(), H, W, window, c.data_ptr(), _s())
    mmv = _np(mm).view(np.float32)
    for i in range(N):
        want_disp, want_z, want_code = R.post(q[i], Qs[i])
        _assert_bit_equal(_np(disp[i]), want_disp)
        _assert_bit_equal(_np(z[i]), want_z)
        assert np.array_equal(_np(code[i]), want_code), i
        _assert_bit_equal([_np(c)[i]], [R.center_distance(want_z, window)])
        d0 = np.nan_to_num(want_disp, nan=0.0)
        assert mmv[i, 0] == d0.min() and mmv[i, 1] == d0.max(), i  # each stream's display range is its own
    assert mmv[1, 0] == mmv[1, 1] == 0.0 and not _np(code[1]).any()
    assert _np(code[0]).max() >= 254 and _np(code[2]).max() >= 254
    assert np.isfinite(_np(c)[0]) and np.isnan(_np(c)[1]) and np.isnan(_np(c)[2])
    # the streams' matrices were told apart
    assert not np.array_equal(R.post(q[0], Qs[0])[1], R.post(q[0], Qs[1])[1], equal_nan=True)


# ---------------------------------------------------------------------- 5: the whole loop body
MATCHER_KW = dict(num_disparities=16, block_size=5, speckle_window_size=10)


@pytest.mark.parametrize("with_maps", [False, True], ids=["no_maps", "per_stream_maps"])
@pytest.mark.parametrize("mode", ["3way", "hh"])
def test_classic_depth_batch_step(calib_Q, mode, with_maps):
    """A stream's bytes do not depend on n: every stream of a 3-rig step equals a ClassicDepth (the same
    implementation with n = 1, pinned to separate entry-point calls by test_gpu_sgm.py::test_classic_depth_step)
    stepped on that rig's pair, and the matcher's maps equal the restatement end to end."""
    H, W = 48, 64
    rng = np.random.default_rng(11 + with_maps)
    Qs = np.stack([calib_Q * s for s in (1.0, 2.0, 0.5)])

    def scenes(base):
        pairs = [R.shifted_bgr_scene(rng, H, W, base + i, noise=6) for i in range(N)]
        return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])

    rects = None
    if with_maps:
        rects = []
        for _ in range(N):
            ml, mr = live_ref.random_maps(rng, H, W, outside=0.0), live_ref.random_maps(rng, H, W, outside=0.0)
            rects.append(live.Rectification(ml[0], ml[1], mr[0], mr[1], (W, H), 500.0, 0.07))
    batch = sgm.ClassicDepthBatch(N, rectification=rects, Q=Qs, center_window=15, mode=mode, **MATCHER_KW)
    singles = [sgm.ClassicDepth(rectification=None if rects is None else rects[i], Q=Qs[i], center_window=15, mode=mode,
                                **MATCHER_KW) for i in range(N)]

    def check(res, fl, fr):
        centers = res.readout()
        assert isinstance(centers, np.ndarray) and centers.dtype == np.float32 and centers.shape == (N,)
        qs = []
        for i in range(N):
            one = singles[i].step(fl[i], fr[i])
            for name in ("disparity_q4", "rect_left", "rect_right", "disp_vis"):
                got = getattr(res, name)
                assert tuple(got.shape[1:]) == tuple(getattr(one, name).shape)
                assert torch.equal(got[i], getattr(one, name)), (name, i)
            _assert_bit_equal(_np(res.disparity[i]), _np(one.disparity))
            _assert_bit_equal(_np(res.depth_m[i]), _np(one.depth_m))
            _assert_bit_equal([centers[i]], [one.readout()])
            qs.append(_np(one.disparity_q4))
        return qs

    fl, fr = scenes(4)
    qs = check(batch.step(fl, fr), fl, fr)  # numpy frames
    if not with_maps:  # the scenes are matched, differ, and equal the restatement end to end
        p = R.Params(**MATCHER_KW)
        for i in range(N):
            assert np.array_equal(qs[i], M.compute(R.gray(fl[i]), R.gray(fr[i]), p, mode))
            assert (qs[i][:, 16:] != -16).mean() > 0.5
        assert not np.array_equal(qs[0], qs[1]) and not np.array_equal(qs[1], qs[2])
    # device frames; a third step at the size allocates nothing
    dl, dr = _dev(fl), _dev(fr)
    check(batch.step(dl, dr), fl, fr)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = batch.step(dl, dr)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    # the step's launches capture into a graph; a replay on new frames gives the eager bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = batch.step(dl, dr)
    fl2, fr2 = scenes(8)
    dl.copy_(_dev(fl2))
    dr.copy_(_dev(fr2))
    g.replay()
    torch.cuda.synchronize()
    qs2 = check(res, fl2, fr2)
    assert not np.array_equal(qs[0], qs2[0])


def test_step_launch_count_does_not_depend_on_n(calib_Q):
    """The entry points a step calls, counted through the call hook: the same list for 1 and for 3 streams, and for
    a ClassicDepth."""
    H, W = 24, 40
    rng = np.random.default_rng(3)
    calls = []
    L.set_call_hook(lambda name, args, phase: calls.append(name) if phase == "pre" else None)
    try:
        seen = []
        for n in (1, N):
            f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
            batch = sgm.ClassicDepthBatch(n, Q=calib_Q, **MATCHER_KW)
            batch.step(_dev(f), _dev(f))
            calls.clear()
            batch.step(_dev(f), _dev(f))
            seen.append(list(calls))
        one = sgm.ClassicDepth(Q=calib_Q, **MATCHER_KW)
        one.step(_dev(f[0]), _dev(f[0]))
        calls.clear()
        one.step(_dev(f[0]), _dev(f[0]))
        seen.append(list(calls))
    finally:
        L.set_call_hook(None)
    torch.cuda.synchronize()
    assert seen[0] == seen[1] == seen[2] == ["sd_sgm_gray", "sd_sgm_gray", "sd_sgm_compute_n", "sd_sgm_post_n",
                                             "sd_sgm_center_n", "sd_live_compose_n"]
