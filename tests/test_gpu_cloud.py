"""Coloured point clouds on the device (csrc/cloud.hip: sd_cloud_build_n; stereo_depth_estimation_amd/cloud.py; the hooks
in sgm.py and predict.py; needs an MI355X).

Everything is compared bit for bit with the NumPy restatement tests/cloud_ref.py: the records as raw bytes, the organised
cloud with equal NaN positions and equal bits elsewhere. The stage is defined in exactly rounded operations, so there is
no tolerance anywhere in this file.

Shapes come from the kernel's own constants (T = TILE_PIXELS pixels per compaction block, S = SCAN_WIDTH tile counts
per scan step): one pixel, less than a wave, a few waves, exactly one tile, one tile and a pixel, and more than S tiles
plus a partial one (so the scan carries across steps).
"""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

import cloud_ref as R
import sgm_ref
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import cloud as C
from stereo_depth_estimation_amd import sgm

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, S = C.TILE_PIXELS, C.SCAN_WIDTH
INF = float("inf")
GOLDEN = Path(__file__).resolve().parent / "golden"

SHAPES = [(1, 1), (3, 5), (37, 61), (T // 64, 64), (25, (T + 1) // 25), ((S + 1) * T // 64 + 5, 64)]
assert SHAPES[3][0] * SHAPES[3][1] == T and SHAPES[4][0] * SHAPES[4][1] == T + 1 and T % 64 == 0
assert SHAPES[5][0] * 64 > (S + 1) * T and (SHAPES[5][0] * 64) % T != 0
PATTERNS = ("all", "none", "first", "last", "checker", "tiles", "rand10", "rand90")
NO_VALUE = np.array([np.nan, 0.0, -3.5, np.inf, -np.inf, -0.0], dtype=np.float32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def calib_Q(golden_dir):
    with np.load(golden_dir / "sgm_calib.npz") as d:
        return np.array(d["Q"], dtype=np.float64)


def stream_Q(Q, i):
    """Another principal point and another baseline per stream, so a matrix read from the wrong stream shows."""
    Q = Q.copy()
    Q[0, 3] -= 7.0 * i
    Q[1, 3] += 3.0 * i
    Q[3, 2] *= 1.0 + 0.25 * i
    return Q


def pattern_disparity(hw, pattern, seed):
    """Valid disparities in [1, 120) where the pattern keeps a pixel, NaN / 0 / negative / inf / -inf / -0 elsewhere."""
    H, W = hw
    rng = np.random.default_rng(seed)
    idx = np.arange(H * W).reshape(H, W)
    yy, xx = np.divmod(idx, W)
    keep = {"all": np.ones((H, W), bool), "none": np.zeros((H, W), bool), "first": idx == 0, "last": idx == H * W - 1,
            "checker": (xx + yy) % 2 == 0, "tiles": (idx // T) % 2 == 0, "rand10": rng.random((H, W)) < 0.1,
            "rand90": rng.random((H, W)) < 0.9}[pattern]
    d = rng.uniform(1, 120, (H, W)).astype(np.float32)
    return np.where(keep, d, NO_VALUE[(idx + seed) % len(NO_VALUE)]).astype(np.float32), keep


def colors(hw, seed):
    return np.random.default_rng(seed + 99).integers(0, 256, (*hw, 3), dtype=np.uint8)


_cases = {}


def case(hw, pattern, stream):
    """One stream's inputs and its reference (unbounded z, stride 1, BGR colours): computed once, shared, read-only."""
    key = (hw, pattern, stream)
    if key not in _cases:
        Q = stream_Q(np.load(GOLDEN / "sgm_calib.npz")["Q"].astype(np.float64), stream)
        seed = hw[0] * 1000 + hw[1] + 17 * stream + PATTERNS.index(pattern)
        d, keep = pattern_disparity(hw, pattern, seed)
        col = colors(hw, seed)
        c = {"Q": Q, "disp": d, "color": col, "keep": keep, "records": R.records(d, Q, col, True),
             "xyz": R.organized(d, Q)}
        for a in c.values():
            a.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def assert_xyz(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def stream_bytes(res, counts, i):
    return res.points[i, :min(int(counts[i]), res.cap)].cpu().numpy().tobytes()


@pytest.mark.parametrize("k", range(len(PATTERNS)))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_records_and_organized_cloud_equal_the_reference(hw, n, k):
    pats = [PATTERNS[(k + i) % len(PATTERNS)] for i in range(n)]
    cs = [case(hw, p, i) for i, p in enumerate(pats)]
    for c, p in zip(cs, pats):  # with this Q every value reprojects to finite numbers: the pattern is what is kept
        assert len(c["records"]) == c["keep"].sum(), p
    builder = C.PointCloudBuilder(n)
    res = builder.build(dev(np.stack([c["disp"] for c in cs])), np.stack([c["Q"] for c in cs]),
                        color=dev(np.stack([c["color"] for c in cs])), bgr=True, organized=True)
    counts = res.counts()
    assert counts.dtype == np.uint32 and res.points.shape == (n, hw[0] * hw[1], 16) and res.cap == hw[0] * hw[1]
    xyz = res.xyz.cpu().numpy()
    for i, c in enumerate(cs):
        assert counts[i] == len(c["records"]), (pats[i], counts[i])
        assert stream_bytes(res, counts, i) == c["records"].tobytes(), pats[i]
        assert np.array_equal(res.numpy(i), c["records"]) and res.numpy(i).dtype == C.RECORD
        assert_xyz(xyz[i], c["xyz"])


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("hw", [SHAPES[2], SHAPES[4]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stride_and_depth_range(hw, stride, calib_Q):
    """The prototype input (uniform [-4, 140), 10 % NaN, one inf) with z_range (0.3, 10): every predicate has both
    outcomes. Sizes that are no multiples of the stride; the organised cloud ignores the stride."""
    assert hw[0] % 2 and hw[1] % 2 and (hw[0] % 3 or hw[1] % 3)
    n = 2
    disp = np.stack([R.prototype_disparity(*hw, seed=i) for i in range(n)])
    Qs = np.stack([stream_Q(calib_Q, i) for i in range(n)])
    col = np.stack([colors(hw, i) for i in range(n)])
    res = C.PointCloudBuilder(n).build(dev(disp), Qs, color=dev(col), z_range=(0.3, 10), stride=stride, organized=True)
    counts = res.counts()
    assert res.cap == -(-hw[0] // stride) * -(-hw[1] // stride)
    for i in range(n):
        want = R.records(disp[i], Qs[i], col[i], True, (0.3, 10), stride)
        xyz, has = R.reproject(disp[i], Qs[i])
        kept = R.kept_mask(xyz, has, (0.3, 10))
        assert 0 < len(want) < kept.sum() or stride == 1
        assert 0 < kept.sum() < has.sum() < disp[i].size
        assert counts[i] == len(want) and stream_bytes(res, counts, i) == want.tobytes()
        assert_xyz(res.xyz[i].cpu().numpy(), R.organized(disp[i], Qs[i], (0.3, 10)))


def test_points_exactly_on_the_bounds_are_kept(calib_Q):
    hw = SHAPES[2]
    d = R.prototype_disparity(*hw, seed=3)
    z = np.sort(R.records(d, calib_Q)["z"])
    lo, hi = float(z[len(z) // 4]), float(z[3 * len(z) // 4])
    assert lo < hi
    want = R.records(d, calib_Q, None, True, (lo, hi))
    assert (want["z"] == np.float32(lo)).any() and (want["z"] == np.float32(hi)).any() and 0 < len(want) < len(z)
    res = C.PointCloudBuilder(1).build(dev(d[None]), calib_Q, z_range=(lo, hi))
    counts = res.counts()
    assert counts[0] == len(want) and stream_bytes(res, counts, 0) == want.tobytes()
    got = res.numpy(0)
    assert (got["z"] == np.float32(lo)).any() and (got["z"] == np.float32(hi)).any()
    assert (got["red"] == 255).all() and (got["green"] == 255).all() and (got["blue"] == 255).all()  # no colour: white
    # half-open and one-point ranges
    for zr in ((-INF, hi), (lo, INF), (lo, lo)):
        w = R.records(d, calib_Q, None, True, zr)
        r = C.PointCloudBuilder(1).build(dev(d[None]), calib_Q, z_range=zr)
        c = r.counts()
        assert c[0] == len(w) > 0 and stream_bytes(r, c, 0) == w.tobytes()


def test_zero_denominator_pixels_are_dropped(calib_Q):
    """A last row that gives R_3 = x - 2: column 2 divides by zero (inf or NaN as float32) and is dropped."""
    hw = SHAPES[2]
    d, _ = pattern_disparity(hw, "all", 5)
    Q = calib_Q.copy()
    Q[3] = [1.0, 0.0, 0.0, -2.0]
    want = R.records(d, Q)
    assert len(want) == hw[0] * (hw[1] - 1)
    res = C.PointCloudBuilder(1).build(dev(d[None]), Q, organized=True)
    counts = res.counts()
    assert counts[0] == len(want) and stream_bytes(res, counts, 0) == want.tobytes()
    xyz = res.xyz[0].cpu().numpy()
    assert np.isnan(xyz[:, 2]).all() and not np.isnan(xyz[:, 3]).any()
    assert_xyz(xyz, R.organized(d, Q))


def test_colour_orders(calib_Q):
    hw = SHAPES[2]
    d, _ = pattern_disparity(hw, "rand90", 8)
    col = colors(hw, 8)
    b = C.PointCloudBuilder(1)
    for kw, ref_col, ref_bgr in ((dict(color=dev(col[None]), bgr=True), col, True),
                                 (dict(color=dev(col[None]), bgr=False), col, False), (dict(), None, True)):
        res = b.build(dev(d[None]), calib_Q, **kw)
        want = R.records(d, calib_Q, ref_col, ref_bgr)
        c = res.counts()
        assert c[0] == len(want) and stream_bytes(res, c, 0) == want.tobytes()
        assert (res.numpy(0)["alpha"] == 255).all()
    rgb = b.build(dev(d[None]), calib_Q, color=dev(col[None]), bgr=False).numpy(0)
    bgr = b.build(dev(d[None]), calib_Q, color=dev(col[None]), bgr=True).numpy(0)
    assert np.array_equal(rgb["red"], bgr["blue"]) and not np.array_equal(rgb["red"], bgr["red"])


# ---------------------------------------------------------------------- the entry point on raw buffers
FILL = 0xEE
GUARD = 4096


def raw_build(disp, Qs, color=None, bgr=True, z_range=(-INF, INF), stride=1, cap=None, work=None, xyz=False):
    """sd_cloud_build_n on buffers of this test's own: points pre-filled with 0xEE and followed by a guard region, a
    workspace of 0xFF bytes unless one is handed in. Returns (points bytes [n, cap, 16], guard, counts, work, xyz)."""
    n, H, W = disp.shape
    cap = C.lattice_size(H, W, stride) if cap is None else cap
    pts = torch.full((n * cap * 16 + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    cnt = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ws = L.call("sd_cloud_ws_bytes", n, H, W, stride)
    if work is None:
        work = torch.full((ws + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((n, H, W, 3), 7.0, device=DEV) if xyz else None
    d_d, q_d = dev(disp), dev(np.ascontiguousarray(Qs, dtype=np.float64).reshape(n, 16))
    c_d = dev(color) if color is not None else None
    L.call("sd_cloud_build_n", n, d_d.data_ptr(), L.ptr(c_d), int(bgr), H, W, q_d.data_ptr(), float(z_range[0]),
           float(z_range[1]), stride, L.ptr(out), pts.data_ptr(), cap, cnt.data_ptr(), work.data_ptr(),
           L.stream_handle())
    torch.cuda.synchronize()
    h = pts.cpu().numpy()
    c = cnt.cpu().numpy()
    assert (c[n:] == 0x5A5A5A5A).all() and (work[ws:].cpu().numpy() == 0xFF).all()  # nothing past count and work
    return (h[:n * cap * 16].reshape(n, cap, 16), h[n * cap * 16:], c[:n].view(np.uint32), work,
            out.cpu().numpy() if xyz else None)


def three_streams(hw, pats=("rand90", "checker", "rand10")):
    cs = [case(hw, p, i) for i, p in enumerate(pats)]
    return (np.stack([c["disp"] for c in cs]), np.stack([c["Q"] for c in cs]), np.stack([c["color"] for c in cs]),
            [c["records"] for c in cs])


@pytest.mark.parametrize("hw", [SHAPES[2], SHAPES[4]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cap_below_count_writes_the_first_records_and_nothing_else(hw):
    disp, Qs, col, want = three_streams(hw, ("rand90", "checker", "first"))
    cap = 100
    assert len(want[0]) > cap and len(want[1]) > cap and len(want[2]) == 1  # two clipped streams and one that fits
    pts, guard, counts, _, _ = raw_build(disp, Qs, col, cap=cap)
    assert (guard == FILL).all()
    for i in range(3):
        assert counts[i] == len(want[i])  # the full number, whether or not it fits
        k = min(len(want[i]), cap)
        assert pts[i, :k].tobytes() == want[i][:k].tobytes()
        assert (pts[i, k:] == FILL).all()  # from there to cap: untouched
    # cap = 1, and a cap far above the lattice
    pts, guard, counts, _, _ = raw_build(disp, Qs, col, cap=1)
    assert (guard == FILL).all() and [int(c) for c in counts] == [len(w) for w in want]
    for i in range(3):
        assert pts[i, 0].tobytes() == want[i][:1].tobytes()
    pts, guard, counts, _, _ = raw_build(disp, Qs, col, cap=hw[0] * hw[1] + 13)
    assert (guard == FILL).all()
    for i in range(3):
        assert pts[i, :len(want[i])].tobytes() == want[i].tobytes() and (pts[i, len(want[i]):] == FILL).all()


@pytest.mark.parametrize("hw", [SHAPES[2], SHAPES[5]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stream_independence_and_determinism(hw):
    disp, Qs, col, want = three_streams(hw)
    pts, guard, counts, work, xyz = raw_build(disp, Qs, col, xyz=True)
    assert (guard == FILL).all()
    for i in range(3):
        assert counts[i] == len(want[i]) and pts[i, :len(want[i])].tobytes() == want[i].tobytes()
        one, _, c1, _, x1 = raw_build(disp[i:i + 1], Qs[i:i + 1], col[i:i + 1], xyz=True)  # the stream alone
        assert c1[0] == counts[i] and np.array_equal(one[0], pts[i])
        assert np.array_equal(x1[0].view(np.uint32), xyz[i].view(np.uint32))
    again = raw_build(disp, Qs, col, xyz=True)
    assert np.array_equal(again[0], pts) and np.array_equal(again[2], counts)
    assert np.array_equal(again[4].view(np.uint32), xyz.view(np.uint32))
    # a workspace left dirty by a call on other inputs (the streams in another order, another stride)
    raw_build(disp[::-1], Qs[::-1], col[::-1], stride=2, work=work)
    dirty = raw_build(disp, Qs, col, work=work)
    assert np.array_equal(dirty[0], pts) and np.array_equal(dirty[2], counts)
    # xyz alone: one launch, the same organised cloud; points alone: the same records
    out = torch.full((3, *hw, 3), 7.0, device=DEV)
    L.call("sd_cloud_build_n", 3, dev(disp).data_ptr(), None, 1, hw[0], hw[1], dev(Qs.reshape(3, 16)).data_ptr(), -INF,
           INF, 1, out.data_ptr(), None, 0, None, None, L.stream_handle())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), xyz.view(np.uint32))


def test_builder_reuses_its_buffers(calib_Q):
    hw = SHAPES[2]
    d = dev(np.stack([case(hw, "rand90", i)["disp"] for i in range(2)]))
    b = C.PointCloudBuilder(2)
    r1 = b.build(d, calib_Q, organized=True)
    r1.counts()
    before = torch.cuda.memory_allocated()
    ptrs = (r1.points.data_ptr(), r1.xyz.data_ptr())
    r2 = b.build(d, calib_Q, organized=True, stride=2)  # a smaller cap: the same allocations
    r3 = b.build(d[:1], calib_Q, organized=True)  # fewer streams than the builder's
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert (r2.points.data_ptr(), r2.xyz.data_ptr()) == ptrs and r3.points.shape[0] == 1
    with pytest.raises(ValueError, match="streams"):
        b.build(torch.zeros(3, *hw, device=DEV), calib_Q)
    with pytest.raises(ValueError, match="float32"):
        b.build(torch.zeros(2, *hw, device=DEV, dtype=torch.float64), calib_Q)
    with pytest.raises(ValueError, match="color"):
        b.build(d, calib_Q, color=torch.zeros(2, *hw, 3, device=DEV))
    with pytest.raises(ValueError, match="NaN"):
        b.build(d, calib_Q, z_range=(float("nan"), 1.0))
    with pytest.raises(ValueError, match="min <= max"):
        b.build(d, calib_Q, z_range=(2.0, 1.0))
    with pytest.raises(ValueError, match="stride"):
        b.build(d, calib_Q, stride=65)
    with pytest.raises(ValueError, match="cap"):
        b.build(d, calib_Q, cap=0)
    with pytest.raises(ValueError, match="Q must be"):
        b.build(d, np.zeros((3, 4, 4)))


def test_save_ply_round_trip(tmp_path, calib_Q):
    hw = SHAPES[2]
    cs = [case(hw, p, i) for i, p in enumerate(("rand90", "none", "first"))]
    res = C.PointCloudBuilder(3).build(dev(np.stack([c["disp"] for c in cs])), np.stack([c["Q"] for c in cs]),
                                       color=dev(np.stack([c["color"] for c in cs])))
    paths = [tmp_path / f"{i}.ply" for i in range(3)]
    counts = res.save_ply(paths)
    assert [int(c) for c in counts] == [len(c["records"]) for c in cs] and counts[1] == 0 and counts[2] == 1
    for p, c in zip(paths, cs):
        got = C.read_ply(p)
        assert np.array_equal(got, c["records"])
        assert p.read_bytes() == C.ply_header(len(got)) + c["records"].tobytes()


# ---------------------------------------------------------------------- against the matcher's own reprojection
MATCHER_KW = dict(num_disparities=16, block_size=5, speckle_window_size=10)


def test_z_equals_sgm_post_z_bit_for_bit(calib_Q):
    H, W, n = 48, 64, 2
    rng = np.random.default_rng(21)
    pairs = [sgm_ref.shifted_bgr_scene(rng, H, W, 4 + i, noise=6) for i in range(n)]
    gl = dev(np.stack([sgm_ref.gray(a) for a, _ in pairs]))
    gr = dev(np.stack([sgm_ref.gray(b) for _, b in pairs]))
    q = sgm.StereoSGM(**MATCHER_KW).compute_batch(gl, gr)
    Qs = np.stack([stream_Q(calib_Q, i) for i in range(n)])
    Qd = dev(Qs.reshape(n, 16))
    disp, z = torch.empty(n, H, W, device=DEV), torch.empty(n, H, W, device=DEV)
    code = torch.empty(n, H, W, dtype=torch.uint8, device=DEV)
    mm = torch.zeros(n, 2, dtype=torch.int32, device=DEV)
    L.call("sd_sgm_post_n", n, q.data_ptr(), H, W, Qd.data_ptr(), disp.data_ptr(), z.data_ptr(), code.data_ptr(),
           mm.data_ptr(), L.stream_handle())
    res = C.PointCloudBuilder(n).build(disp, Qd, organized=True)  # the device matrices, as ClassicDepthBatch holds them
    torch.cuda.synchronize()
    z_h, xyz = z.cpu().numpy(), res.xyz.cpu().numpy()
    valid = ~np.isnan(z_h)
    assert valid.mean() > 0.3 and not valid.all()
    assert np.array_equal(np.isnan(xyz[..., 2]), ~valid)
    assert np.array_equal(xyz[..., 2][valid].view(np.uint32), z_h[valid].view(np.uint32))
    for i in range(n):
        assert_xyz(xyz[i], R.organized(disp[i].cpu().numpy(), Qs[i]))


def test_classic_depth_batch_cloud(calib_Q):
    H, W, n = 48, 64, 2
    rng = np.random.default_rng(12)
    pairs = [sgm_ref.shifted_bgr_scene(rng, H, W, 5 + i, noise=6) for i in range(n)]
    fl, fr = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    Qs = np.stack([stream_Q(calib_Q, i) for i in range(n)])
    rigs = sgm.ClassicDepthBatch(n, Q=Qs, **MATCHER_KW)
    with pytest.raises(RuntimeError, match="before the first step"):
        rigs.cloud()
    res = rigs.step(fl, fr)
    cloud = rigs.cloud(z_range=(0.3, 10.0), stride=2, organized=True)
    counts = cloud.counts()
    disp, left = res.disparity.cpu().numpy(), res.rect_left.cpu().numpy()
    assert np.array_equal(left, fl)  # no rectification: the frames themselves, BGR
    for i in range(n):
        want = R.records(disp[i], Qs[i], left[i], True, (0.3, 10.0), 2)
        assert 0 < len(want) < cloud.cap
        assert counts[i] == len(want) and stream_bytes(cloud, counts, i) == want.tobytes()
        assert_xyz(cloud.xyz[i].cpu().numpy(), R.organized(disp[i], Qs[i], (0.3, 10.0)))
    # step() is untouched by it: the same bytes as a rig that never built a cloud
    other = sgm.ClassicDepthBatch(n, Q=Qs, **MATCHER_KW).step(fl, fr)
    assert torch.equal(other.disparity_q4, res.disparity_q4) and torch.equal(other.disp_vis, res.disp_vis)
    # one rig
    one = sgm.ClassicDepth(Q=Qs[1], **MATCHER_KW)
    with pytest.raises(RuntimeError, match="before the first step"):
        one.cloud()
    one.step(fl[1], fr[1])
    c1 = one.cloud(z_range=(0.3, 10.0), stride=2)
    assert np.array_equal(c1.numpy(0), R.records(disp[1], Qs[1], left[1], True, (0.3, 10.0), 2))


# ---------------------------------------------------------------------- predict --write-ply
MODEL_HW = (32, 48)


def tiny_model():
    from oracle import unet_ref as U
    from stereo_depth_estimation_amd.model import StereoUNet

    st = U.make_state(8, seed=0, signed_gamma=True)
    m = StereoUNet(base_channels=8, precision="fp32")
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV).eval()


def expected_disp_up(model, items, batch_size):
    """Per item (sd_disp_export's disp_up, the left frame): the model on the sd_stereo_preprocess input in the tool's
    batches, its disparity through sd_resize_bilinear (the entry point disp_up equals bit for bit, test_gpu_predict)."""
    from stereo_depth_estimation_amd import dataset as D
    from stereo_depth_estimation_amd import predict as P

    H, W = MODEL_HW
    out = {}
    for hw, its in P.plan_batches(items, batch_size):
        n = len(its)
        frames = [np.stack([D.read_rgb_uint8(getattr(it, a)) for it in its])
                  for a in ("left_rgb_path", "right_rgb_path", "disparity_path")]
        l_d, r_d, g_d = (torch.from_numpy(f).to(DEV) for f in frames)
        inp = torch.empty(n, 6, H, W, device=DEV)
        tgt = torch.empty(n, 1, H, W, device=DEV)
        val = torch.empty(n, 1, H, W, device=DEV, dtype=torch.bool)
        L.call("sd_stereo_preprocess", l_d.data_ptr(), r_d.data_ptr(), g_d.data_ptr(), n, hw[0], hw[1], H, W,
               inp.data_ptr(), tgt.data_ptr(), val.data_ptr(), L.stream_handle())
        with torch.inference_mode():
            d, _ = model(inp, return_uncertainty=True)
        up = torch.empty(n, *hw, device=DEV)
        mul = float(np.float32(hw[1] / float(W)))
        L.call("sd_resize_bilinear", d[:, 0].contiguous().data_ptr(), n, H, W, up.data_ptr(), hw[0], hw[1], mul,
               L.stream_handle())
        torch.cuda.synchronize()
        for k, it in enumerate(its):
            out[it.relpath] = (up[k].cpu().numpy(), frames[0][k])
    return out


def files_under(root, suffix=None):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file() and (not suffix or p.suffix == suffix))


def test_predictor_cloud_in_batches_above_64_streams():
    """Predictor.run with 70 samples: two sd_cloud_build_n calls (64 + 6 streams) into one block of records."""
    from stereo_depth_estimation_amd import predict as P

    n, hw = 70, (20, 24)
    rng = np.random.default_rng(3)
    left = rng.integers(0, 256, (n, *hw, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (n, *hw, 3), dtype=np.uint8)
    opts = P.CloudOptions(focal_px=30.0, baseline_m=0.1, stride=3)
    res = P.Predictor(tiny_model(), (MODEL_HW[1], MODEL_HW[0])).run(dev(left), dev(right), cloud=opts)
    torch.cuda.synchronize()
    up, pts = res["disp_up"].cpu().numpy(), res["points"].cpu().numpy()
    counts = res["counts"].cpu().numpy().view(np.uint32)
    Q = C.pinhole_Q(30.0, 0.1, (hw[1] - 1) / 2, (hw[0] - 1) / 2)
    assert pts.shape == (n, C.lattice_size(*hw, 3), 16) and res["disp_rgb"].shape == (n, *hw, 3)
    for k in range(n):
        want = R.records(up[k], Q, left[k], False, stride=3)
        assert counts[k] == len(want) == pts.shape[1], k  # softplus disparities: every lattice pixel has a value
        assert pts[k].tobytes() == want.tobytes(), k


def test_predict_write_ply(tmp_path, calib_Q):
    from conftest import write_stereo_tree
    from stereo_depth_estimation_amd import predict as P

    H, W = MODEL_HW
    root = tmp_path / "data"
    write_stereo_tree(root, scenes=2, frames=3, hw=(45, 61), seed=5)
    model = tiny_model()
    items = P.dataset_items(root)
    assert len(items) == 6
    want_up = expected_disp_up(model, items, 4)
    common = dict(model=model, height=H, width=W, batch_size=4)

    # an ideal rig in pixels of the frames, the principal point at the frame centre. The random-weight model's
    # disparities lie close to 0.87 px on these frames (softplus of a small head; the CPU oracle gives 0.867 ... 0.875
    # with the median at 0.8712), so Z = f B / d is near 6.6 / 0.8712 = 7.5758 m: a bound there splits the pixels
    f, B, ZMAX = 55.0, 0.12, 7.5755
    out = tmp_path / "out"
    meta = P.predict_dataset(None, root, out, write_ply=True, focal_px=f, baseline_m=B, ply_stride=2,
                             ply_max_depth=ZMAX, **common)
    Q = C.pinhole_Q(f, B, (61 - 1) / 2, (45 - 1) / 2)
    plys = [P.ply_relpath(it.relpath).as_posix() for it in items]
    assert files_under(out, ".ply") == sorted(plys) and len(files_under(out, ".png")) == 6
    total, per_sample = 0, []
    for it in items:
        up, left = want_up[it.relpath]
        want = R.records(up, Q, left, False, (-INF, ZMAX), 2)  # the left frame is RGB
        got = C.read_ply(out / P.ply_relpath(it.relpath))
        assert 0 < len(want) < C.lattice_size(45, 61, 2)  # the depth bound drops some
        assert got.tobytes() == want.tobytes(), it.relpath
        total += len(want)
        per_sample.append(len(want))
    assert meta["points"] == total and json.loads((out / "predict_meta.json").read_text()) == meta
    assert (meta["write_ply"], meta["focal_px"], meta["baseline_m"], meta["ply_stride"], meta["ply_min_depth"],
            meta["ply_max_depth"], meta["cx"], meta["ply_calibration_Q"]) == (True, f, B, 2, None, float(np.float32(ZMAX)), None, None)
    rows = [json.loads(s) for s in (out / "metrics.jsonl").read_text().splitlines()]
    assert [r["points"] for r in rows] == per_sample and [r["sample"] for r in rows] == [it.relpath.as_posix() for it in items]

    # a calibration file for another image size: Q rescaled to the frames
    calib = tmp_path / "calib.npz"
    np.savez(calib, Q=calib_Q, image_size=np.array([640, 480]))
    out2 = tmp_path / "out_calib"
    meta2 = P.predict_dataset(None, root, out2, write_ply=True, calibration=calib, **common)
    Qs = C.rescale_Q(calib_Q, 61 / 640, 45 / 480)
    total2 = 0
    for it in items:
        up, left = want_up[it.relpath]
        want = R.records(up, Qs, left, False)
        assert C.read_ply(out2 / P.ply_relpath(it.relpath)).tobytes() == want.tobytes(), it.relpath
        total2 += len(want)
    assert meta2["points"] == total2 > 0 and meta2["ply_calibration_image_size"] == [640, 480]

    # without the flag: no .ply, none of the new keys, and the same disparity bytes as with it
    out3 = tmp_path / "out_plain"
    meta3 = P.predict_dataset(None, root, out3, **common)
    assert files_under(out3, ".ply") == []
    assert not ({"points", "write_ply", "ply_stride", "focal_px", "baseline_m", "ply_calibration_Q"} & set(meta3))
    assert all("points" not in json.loads(s) for s in (out3 / "metrics.jsonl").read_text().splitlines())
    for it in items:
        assert (out3 / it.relpath).read_bytes() == (out / it.relpath).read_bytes()
    assert (out3 / "metrics.jsonl").read_text() == "".join(
        json.dumps({k: v for k, v in r.items() if k != "points"}) + "\n" for r in rows)

    # directory pairs and the command line
    data0 = root / "scene00" / "dataset" / "data"
    out4 = tmp_path / "out_pairs"
    ck = tmp_path / "best.pt"
    torch.save({"epoch": 1, "model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()},
                "args": {"height": H, "width": W}, "metrics": {}}, ck)
    meta4 = P.main(["--checkpoint", str(ck), "--left-dir", str(data0 / "left" / "rgb"), "--right-dir",
                    str(data0 / "right" / "rgb"), "--output-root", str(out4), "--base-channels", "8", "--batch-size", "4",
                    "--write-ply", "--focal-px", str(f), "--baseline-m", str(B), "--ply-stride", "2", "--ply-max-depth",
                    str(ZMAX)])
    assert files_under(out4, ".ply") == [f"{k:06d}.ply" for k in range(3)]
    assert meta4["points"] == sum(len(C.read_ply(out4 / f"{k:06d}.ply")) for k in range(3)) > 0

    # argument errors
    with pytest.raises(ValueError, match="--write-ply needs --output-root"):
        P.predict_dataset(None, root, None, write_ply=True, focal_px=f, baseline_m=B, **common)
    with pytest.raises(ValueError, match="needs a geometry"):
        P.predict_dataset(None, root, tmp_path / "never", write_ply=True, **common)
    with pytest.raises(ValueError, match="needs a geometry"):
        P.predict_dataset(None, root, tmp_path / "never", write_ply=True, focal_px=f, **common)
    with pytest.raises(ValueError, match="only with --write-ply"):
        P.predict_dataset(None, root, tmp_path / "never", focal_px=f, baseline_m=B, **common)
    with pytest.raises(ValueError, match="not both"):
        P.predict_dataset(None, root, tmp_path / "never", write_ply=True, calibration=calib, focal_px=f, baseline_m=B,
                          **common)
    with pytest.raises(ValueError, match="--ply-stride"):
        P.predict_dataset(None, root, tmp_path / "never", write_ply=True, focal_px=f, baseline_m=B, ply_stride=0,
                          **common)
    assert not (tmp_path / "never").exists()
