"""The matcher's 4-, 5- and 8-path modes on the device (csrc/sgm.hip: k_sgm_walk, sd_sgm_aggregate_dir,
sd_sgm_compute_mode; needs an MI355X), B = 1 throughout.

array_equal to the NumPy restatement tests/sgm_modes_ref.py everywhere: every single path, accumulation onto a preset
S, the mode's total and the disparities from it, the whole matcher through the C ABI and through StereoSGM, and
ClassicDepth's step. Volumes are allocated zeroed and compared whole: nothing may be written for x < maxD.
"""

import numpy as np
import pytest
import torch

import sgm_modes_ref as M
import sgm_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import sgm

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (H, W, D, minD, bs)
CASES = [
    (9, 40, 16, 0, 3),       # partial wave, H just over the ring depth of 8
    (17, 150, 48, 3, 5),     # D not a multiple of 64, minD > 0, odd tail
    (33, 200, 128, 0, 7),    # the app's settings, two values per lane
    (12, 300, 256, 0, 7),    # four values per lane; hh bound 61544
    (70, 24, 16, 0, 3),      # W - maxD = 8 < H: every diagonal wraps many times
    (10, 17, 16, 0, 3),      # W - maxD = 1: every diagonal step starts a path
    (5, 60, 32, 0, 5),       # H below the ring depth
    (1, 80, 16, 0, 3),       # one row: every vertical-family path is L = C
    (8, 20, 32, 0, 7),       # W < maxD: nothing written, all invalid
]
APP_CASE = CASES[2]
KINDS = ["shift", "noise"]
MODE_NAMES = ("3way", "hh4", "sgbm", "hh")
# the seven directions of sd_sgm_aggregate_dir: the vertical family and left -> right
DIRS = [(dy, dx) for dy in (1, -1) for dx in (-1, 0, 1)] + [(0, 1)]
_ids = dict(ids=lambda c: "x".join(map(str, c)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev(a):
    a = np.array(a, order="C")  # a writable copy (the shared references are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.as_tensor(a).to(DEV)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _s():
    return L.stream_handle()


def _params(case):
    H, W, D, minD, bs = case
    return R.Params(min_disparity=minD, num_disparities=D, block_size=bs,
                    speckle_window_size=100 if case == APP_CASE else 12)


_refs = {}


def _ref(case, kind):
    """Gray planes, the cost volume, every single path and every mode's stages of one case: computed once and shared
    (read-only)."""
    if (case, kind) not in _refs:
        H, W, D, minD, bs = case
        rng = np.random.default_rng(1000 * H + W + (7 if kind == "noise" else 0))
        if kind == "noise":
            left, right = R.shifted_bgr_scene(rng, H, W, W)  # d0 = W: two independent textures
        else:
            left, right = R.shifted_bgr_scene(rng, H, W, minD + D // 3, noise=12)
        p = _params(case)
        gl, gr = R.gray(left), R.gray(right)
        ref = {"gray_l": gl, "gray_r": gr}
        ref["modes"] = {m: M.compute_stages(gl, gr, p, m) for m in MODE_NAMES}
        ref["C"] = ref["modes"]["3way"]["C"]
        ref["paths"] = {d: M.path(ref["C"], p, *d) for d in DIRS}
        for a in [gl, gr, *ref["paths"].values()] + [v for st in ref["modes"].values() for v in st.values()]:
            a.setflags(write=False)
        _refs[(case, kind)] = ref
    return _refs[(case, kind)]


def _dir(C, case, p, dy, dx, accumulate, S):
    H, W, D, minD, bs = case
    L.call("sd_sgm_aggregate_dir", C.data_ptr(), H, W, minD, D, p.P1, p.P2, dy, dx, accumulate, S.data_ptr(), _s())


# ---------------------------------------------------------------------- (a), (b): one path
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, **_ids)
def test_every_direction_alone_and_accumulated(case, kind):
    H, W, D, minD, bs = case
    p, ref = _params(case), _ref(case, kind)
    C = _dev(ref["C"])
    rng = np.random.default_rng(H + W)
    preset = rng.integers(0, 200, (H, W, D)).astype(np.uint16)  # also left of maxD: those columns stay as they are
    want_acc = preset.astype(np.int64)
    for d in DIRS:
        S = torch.zeros((H, W, D), dtype=torch.int16, device=DEV)
        _dir(C, case, p, *d, 0, S)
        assert np.array_equal(_np(S, np.uint16), ref["paths"][d]), d
        S = _dev(preset)
        _dir(C, case, p, *d, 1, S)
        assert np.array_equal(_np(S, np.uint16), want_acc + ref["paths"][d]), d
    if W > p.maxD:  # the paths are not trivially equal: the diagonals differ from the vertical path below row 0
        assert not np.array_equal(ref["paths"][(1, 1)][1:], ref["paths"][(1, 0)][1:]) or H == 1
    else:
        assert not any(v.any() for v in ref["paths"].values())


# ---------------------------------------------------------------------- (c), (d), (e): the modes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, **_ids)
def test_every_mode_equals_the_restatement(case, kind):
    H, W, D, minD, bs = case
    p, ref = _params(case), _ref(case, kind)
    C, gl, gr = _dev(ref["C"]), _dev(ref["gray_l"]), _dev(ref["gray_r"])
    ws_bytes = L.call("sd_sgm_ws_bytes", H, W, D)
    args = (H, W, minD, D, bs, p.P1, p.P2, p.max_diff, p.uniq, p.speckle_window, p.speckle_range, p.cap)
    for mode in MODE_NAMES:
        st = ref["modes"][mode]
        # (c) S from single-path calls, the right -> left path and the winner on top
        if mode != "3way":
            S = torch.zeros((H, W, D), dtype=torch.int16, device=DEV)
            S_total = torch.zeros((H, W, D), dtype=torch.int16, device=DEV)
            q_raw = torch.empty((H, W), dtype=torch.int16, device=DEV)
            q = torch.empty((H, W), dtype=torch.int16, device=DEV)
            for i, d in enumerate(d for d in M.MODES[mode][1] if d != (0, -1)):
                _dir(C, case, p, *d, int(i > 0), S)
            L.call("sd_sgm_winner", C.data_ptr(), S.data_ptr(), H, W, minD, D, p.P1, p.P2, p.uniq, p.max_diff,
                   S_total.data_ptr(), q_raw.data_ptr(), q.data_ptr(), _s())
            assert np.array_equal(_np(S_total, np.uint16), st["S"]), mode
            assert np.array_equal(_np(q_raw), st["q_raw"]), mode
            assert np.array_equal(_np(q), st["q_lr"]), mode
        # (d) the whole matcher: C ABI and Python surface
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        out = torch.empty((H, W), dtype=torch.int16, device=DEV)
        L.call("sd_sgm_compute_mode", gl.data_ptr(), gr.data_ptr(), *args, sgm.MODES[mode][0], ws.data_ptr(),
               out.data_ptr(), _s())
        assert np.array_equal(_np(out), st["q"]), mode
        m = sgm.StereoSGM(min_disparity=minD, num_disparities=D, block_size=bs, speckle_window_size=p.speckle_window,
                          mode=mode)
        assert np.array_equal(_np(m.compute(gl, gr)), st["q"]), mode
        # (e) three paths through the mode entry point: sd_sgm_compute's bytes
        if mode == "3way":
            ws2 = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
            out2 = torch.empty((H, W), dtype=torch.int16, device=DEV)
            L.call("sd_sgm_compute", gl.data_ptr(), gr.data_ptr(), *args, ws2.data_ptr(), out2.data_ptr(), _s())
            assert torch.equal(out, out2)
    if W > p.maxD and kind == "shift" and H > 1:  # the modes are told apart, and the scene is matched
        assert not np.array_equal(ref["modes"]["hh"]["S"], ref["modes"]["3way"]["S"])
        assert (ref["modes"]["hh"]["q_lr"][:, p.maxD:] != p.invalid).mean() > 0.5


def test_eight_paths_give_the_same_bytes_every_time():
    """The paths of a mode add into one S: were two of them ever to run at once, the sums would race. Three runs into
    fresh workspaces give identical, and correct, bytes."""
    H, W, D, minD, bs = APP_CASE
    p, ref = _params(APP_CASE), _ref(APP_CASE, "shift")
    gl, gr = _dev(ref["gray_l"]), _dev(ref["gray_r"])
    outs = []
    for _ in range(3):
        ws = torch.zeros(L.call("sd_sgm_ws_bytes", H, W, D), dtype=torch.uint8, device=DEV)
        out = torch.empty((H, W), dtype=torch.int16, device=DEV)
        L.call("sd_sgm_compute_mode", gl.data_ptr(), gr.data_ptr(), H, W, minD, D, bs, p.P1, p.P2, p.max_diff, p.uniq,
               p.speckle_window, p.speckle_range, p.cap, L.SD_SGM_MODE_HH, ws.data_ptr(), out.data_ptr(), _s())
        outs.append(_np(out))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0], ref["modes"]["hh"]["q"])


# ---------------------------------------------------------------------- the whole loop body
MATCHER_KW = dict(num_disparities=16, block_size=5, speckle_window_size=10)


def test_classic_depth_step_with_eight_paths(golden_dir):
    with np.load(golden_dir / "sgm_calib.npz") as d:
        Q = np.array(d["Q"], dtype=np.float64)
    H, W = 48, 64
    rng = np.random.default_rng(11)
    fl, fr = R.shifted_bgr_scene(rng, H, W, 5, noise=6)
    classic = sgm.ClassicDepth(Q=Q, center_window=15, mode="hh", **MATCHER_KW)
    assert classic.matcher.mode == "hh"
    p = R.Params(**MATCHER_KW)

    def want(a, b):
        q = M.compute(R.gray(a), R.gray(b), p, "hh")
        disp, z, _ = R.post(q, Q)
        return q, disp, z

    def check(res, a, b):
        q, disp, z = want(a, b)
        assert res.disparity_q4.dtype == torch.int16 and np.array_equal(_np(res.disparity_q4), q)
        got_disp, got_z = _np(res.disparity), _np(res.depth_m)
        for got, ref in ((got_disp, disp), (got_z, z)):
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan)
            assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))
        c, wc = np.float32(res.readout()), R.center_distance(z, 15)
        assert (np.isnan(c) and np.isnan(wc)) or c == wc
        return q

    q = check(classic.step(fl, fr), fl, fr)  # numpy frames
    assert (q[:, 16:] != -16).mean() > 0.5
    assert not np.array_equal(q, R.compute(R.gray(fl), R.gray(fr), p))  # not the three-path map
    # device frames; a second step at the size allocates nothing
    dl, dr = _dev(fl), _dev(fr)
    check(classic.step(dl, dr), fl, fr)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = classic.step(dl, dr)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    # the step's launches capture into a graph; a replay on new frames gives the eager bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = classic.step(dl, dr)
    fl2, fr2 = R.shifted_bgr_scene(rng, H, W, 9, noise=6)
    dl.copy_(_dev(fl2))
    dr.copy_(_dev(fr2))
    g.replay()
    torch.cuda.synchronize()
    q2 = check(res, fl2, fr2)
    assert not np.array_equal(q, q2)
