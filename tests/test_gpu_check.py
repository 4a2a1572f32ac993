"""The label-free check on the device (csrc/check.hip: sd_stereo_check; stereo_depth_estimation_amd/check.py; the hooks
in sgm.py and predict.py; needs an MI355X).

cls, disp_vis, resid and vis_rgb are compared bit for bit with the NumPy restatement tests/check_ref.py (equal NaN
positions, equal bits elsewhere): the stage is defined in exactly rounded float32 operations and the minimum is exact
in any order. The counts of rows are equal; its two sums are fp64 additions of at most rows[3] terms in another order
than NumPy's, so they are held to rows[3] * 2^-53 * value, the bound tests/test_gpu_predict.py:assert_rows uses for the
same kind of sum.

Shapes come from the kernel's own constant P = SCAN_PIXELS, the pixels of one step of the right-to-left row walk (four
per thread, 64 lanes, four waves): one pixel, less than a thread's four, around a wave-quarter (63, 64, 65), around one
step (P - 1, P, P + 1) and two steps and a partial third (2P + 5), with one row and with several rows per block.
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import check_ref as R
import cloud_ref
import sgm_ref
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import check as C
from stereo_depth_estimation_amd import sgm

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = C.SCAN_PIXELS
INF = float("inf")
WIDTHS = [1, 3, 63, 64, 65, P - 1, P, P + 1, 2 * P + 5]
THR = 250.0
OUTPUTS = ("cls", "resid", "disp_vis", "vis_rgb")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


_inputs, _refs = {}, {}


def inputs(n, H, W):
    """The generator's inputs of one shape: made once, shared, read-only."""
    key = (n, H, W)
    if key not in _inputs:
        arrs = R.random_case(n, H, W, seed=1000 * W + 10 * H + n)
        for a in arrs:
            a.setflags(write=False)
        _inputs[key] = arrs
    return _inputs[key]


def reference(n, H, W, tol, frames=True):
    """check_ref on every sample of ``inputs(n, H, W)``: computed once per (shape, tolerance), shared, read-only."""
    key = (n, H, W, tol, frames)
    if key not in _refs:
        disp, left, right = inputs(n, H, W)
        per = [R.check(disp[i], left[i], right[i], tol, THR) if frames else R.check(disp[i], occ_tol=tol)
               for i in range(n)]
        ref = {k: np.stack([p[k] for p in per]) for k in ("cls", "disp_vis", "row") + (("resid", "vis_rgb") if frames else ())}
        for a in ref.values():
            a.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def assert_f32(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def assert_rows(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    for k in (0, 1, 2, 3, 6, 7):
        assert np.array_equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    for k in (4, 5):
        tol = want[:, 3] * 2.0 ** -53 * want[:, k]
        assert (np.abs(got[:, k] - want[:, k]) <= tol).all(), (k, got[:, k], want[:, k])


def assert_outputs(got: dict, ref: dict):
    """got: numpy arrays by output name (those that were made)."""
    for k, a in got.items():
        if k in ("resid", "disp_vis"):
            assert_f32(a, ref[k])
        elif k == "rows":
            assert_rows(a, ref["row"])
        else:
            assert a.dtype == np.uint8 and np.array_equal(a, ref[k]), k


def host(res, names=C.OUTPUTS):
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in names if getattr(res, k) is not None}


@pytest.mark.parametrize("tol", [0.0, 0.5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("W", WIDTHS)
def test_outputs_equal_the_reference(W, H, n, tol):
    disp, left, right = inputs(n, H, W)
    ref = reference(n, H, W, tol)
    if W >= 64:  # the condition on the inputs, on the reference: every class is there
        share = np.bincount(ref["cls"].reshape(-1), minlength=5) / ref["cls"].size
        assert (share >= 0.005).all(), share
    chk = C.StereoCheck(n)
    d, l, r = dev(disp), dev(left), dev(right)
    first = host(chk.run(d, l, r, occ_tol=tol, photo_thr=THR))
    assert sorted(first) == sorted(C.OUTPUTS)
    assert_outputs(first, ref)
    # a second run: the same 64 bits
    again = host(chk.run(d, l, r, occ_tol=tol, photo_thr=THR))
    for k in C.OUTPUTS:
        assert first[k].tobytes() == again[k].tobytes(), k
    # each output alone: the same bytes
    for k in C.OUTPUTS:
        res = chk.run(d, l, r, occ_tol=tol, photo_thr=THR, want=(k,))
        assert [o for o in C.OUTPUTS if getattr(res, o) is not None] == [k]
        assert host(res)[k].tobytes() == first[k].tobytes(), k


def raw_check(disp, left, right, tol, thr, shift_out=0, shift_in=0, rows=True):
    """sd_stereo_check itself on buffers whose first element lies `shift` elements into an allocation (so 1 moves a
    float tensor off its 16-byte and a byte tensor off its 4-byte alignment), the workspace filled with 0xFF."""
    n, H, W = disp.shape

    def shifted(a, k):
        src = torch.from_numpy(np.array(a, order="C")).reshape(-1)
        t = torch.empty(src.numel() + k, dtype=src.dtype, device=DEV)
        t[k:].copy_(src)
        return t[k:]

    def out(shape, dtype, k):
        return torch.full((int(np.prod(shape)) + k,), 0x5A if dtype == torch.uint8 else 7.0, dtype=dtype, device=DEV)[k:]

    d, l, r = shifted(disp, shift_in), shifted(left, shift_in), shifted(right, shift_in)
    o = {"cls": out((n, H, W), torch.uint8, shift_out), "resid": out((n, H, W), torch.float32, shift_out),
         "disp_vis": out((n, H, W), torch.float32, shift_out), "vis_rgb": out((n, H, W, 3), torch.uint8, shift_out)}
    rw = torch.full((n, 8), 7.0, dtype=torch.float64, device=DEV) if rows else None
    work = torch.full((L.call("sd_stereo_check_ws_bytes", n, H, W),), 0xFF, dtype=torch.uint8, device=DEV)
    L.call("sd_stereo_check", n, d.data_ptr(), l.data_ptr(), r.data_ptr(), H, W, tol, thr, o["cls"].data_ptr(),
           o["resid"].data_ptr(), o["disp_vis"].data_ptr(), o["vis_rgb"].data_ptr(), L.ptr(rw), work.data_ptr(),
           L.stream_handle())
    torch.cuda.synchronize()
    got = {"cls": o["cls"].view(n, H, W), "resid": o["resid"].view(n, H, W), "disp_vis": o["disp_vis"].view(n, H, W),
           "vis_rgb": o["vis_rgb"].view(n, H, W, 3)}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    if rows:
        got["rows"] = rw.cpu().numpy()
    return got


@pytest.mark.parametrize("W", [64, P])
def test_misaligned_pointers_give_the_same_bytes(W):
    """W % 4 == 0: aligned buffers take the four-pixel path with word stores, misaligned ones the scalar path."""
    n, H = 3, 5
    disp, left, right = inputs(n, H, W)
    ref = reference(n, H, W, 0.5)
    aligned = raw_check(disp, left, right, 0.5, THR)
    assert_outputs(aligned, ref)
    for so, si in ((1, 0), (0, 1), (3, 2)):
        got = raw_check(disp, left, right, 0.5, THR, shift_out=so, shift_in=si)
        for k in aligned:
            assert got[k].tobytes() == aligned[k].tobytes(), (k, so, si)


def test_without_frames():
    n, H, W = 3, 5, P + 1
    disp, _, _ = inputs(n, H, W)
    ref = reference(n, H, W, 0.5, frames=False)
    res = C.StereoCheck(n).run(dev(disp))
    assert res.resid is None and res.vis_rgb is None
    got = host(res)
    assert_outputs(got, ref)
    assert set(np.unique(got["cls"])) == {0, 1, 2, 3}
    assert (got["rows"][:, 3:7] == 0).all() and (got["rows"][:, :3] > 0).all()
    s = res.summary()
    for i in range(n):
        assert s[i] == C.summary_from_row(ref["row"][i]) and s[i]["photo_l1"] is None
        assert s[i]["visible"] == int((ref["cls"][i] == 0).sum())
    chk = C.StereoCheck(n)
    with pytest.raises(ValueError, match="need the frames"):
        chk.run(dev(disp), want=("resid",))
    with pytest.raises(ValueError, match="both or neither"):
        chk.run(dev(disp), left=dev(inputs(n, H, W)[1]))
    with pytest.raises(ValueError, match="1..3 samples"):
        chk.run(dev(np.zeros((4, H, W), np.float32)))


@pytest.mark.parametrize("hw", [(5, 65), (5, 2 * P + 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sample_independence(hw):
    n, (H, W) = 3, hw
    disp, left, right = inputs(n, H, W)
    full = raw_check(disp, left, right, 0.5, THR)
    for i in range(n):
        one = raw_check(disp[i:i + 1], left[i:i + 1], right[i:i + 1], 0.5, THR)
        for k in full:
            assert one[k][0].tobytes() == full[k][i].tobytes(), (k, i)
    # the summary of the Python layer, and its buffers reused by a smaller and a larger run
    chk = C.StereoCheck(n)
    res = chk.run(dev(disp), dev(left), dev(right), photo_thr=THR)
    ptrs = [getattr(res, k).data_ptr() for k in C.OUTPUTS]
    s = res.summary()
    for i in range(n):
        want = C.summary_from_row(full["rows"][i])
        assert s[i] == want and s[i]["visible"] == int((full["cls"][i] == 0).sum())
        assert s[i]["mismatch"] == int((full["cls"][i] == 4).sum()) > 0
    res1 = chk.run(dev(disp[:1]), dev(left[:1]), dev(right[:1]), photo_thr=THR)
    assert [getattr(res1, k).data_ptr() for k in C.OUTPUTS] == ptrs
    assert host(res1)["cls"].tobytes() == full["cls"][:1].tobytes()


def test_special_rows():
    W = 2 * P + 5
    rng = np.random.default_rng(5)
    left = rng.integers(0, 256, (4, 1, W, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (4, 1, W, 3), dtype=np.uint8)
    disp = np.empty((4, 1, W), dtype=np.float32)
    disp[0] = np.resize(np.array([np.nan, 0.0, -3.5, np.inf, -np.inf, -0.0], dtype=np.float32), W)  # no value anywhere
    disp[1] = 2.0  # a plain row: nothing occluded
    # the far occluder: in the last scan step (the first the walk takes), its victims down to the first step
    disp[2] = 2.0
    disp[2, 0, W - 1] = W - 1 - 10  # xr = 10: hides x = 12 .. W - 2
    # the same with the occluder itself out of view
    disp[3] = 2.0
    disp[3, 0, W - 1] = W + 10
    got = raw_check(disp, left, right, 0.0, INF)
    ref = [R.check(disp[i], left[i], right[i], 0.0, INF) for i in range(4)]
    for i in range(4):
        assert_outputs({k: got[k][i:i + 1] for k in got},
                       {**{k: ref[i][k][None] for k in OUTPUTS}, "row": ref[i]["row"][None]})
    assert (got["cls"][0] == 1).all() and (got["rows"][0] == 0).all() and np.isnan(got["resid"][0]).all()
    assert got["cls"][1, 0].tolist() == [2, 2] + [0] * (W - 2)
    assert got["cls"][2, 0].tolist() == [2, 2] + [0] * 10 + [3] * (W - 13) + [0]
    assert got["cls"][3, 0].tolist() == [2, 2] + [3] * (W - 3) + [2]
    assert 12 < P and W - 1 >= 2 * P  # victims in the first step, the occluder in the third
    # one pixel
    for d, c in ((3.0, 2), (np.nan, 1), (0.0, 1)):
        one = raw_check(np.full((1, 1, 1), d, np.float32), left[:1, :, :1], right[:1, :, :1], 0.0, INF)
        assert one["cls"].tolist() == [[[c]]] and one["rows"][0].tolist() == [float(c == 2), float(c == 2), 0, 0, 0, 0, 0, 0]


def test_step_edge_worked_case():
    """The worked case of tests/test_check_cpu.py on the device: the classes by hand, every visible residual 0."""
    disp, left, right = R.step_edge_case()
    res = C.StereoCheck(1).run(dev(disp[None]), dev(left[None]), dev(right[None]), occ_tol=0.0)
    got = host(res)
    want = np.array([2] * 6 + [0] * 25 + [3] * 9 + [0] * 40, dtype=np.uint8)
    for y in range(4):
        assert np.array_equal(got["cls"][0, y], want), y
    vis = got["cls"][0] == 0
    assert (got["resid"][0][vis] == 0).all() and np.isnan(got["resid"][0][~vis]).all()
    assert got["rows"][0].tolist() == [320, 24, 36, 260, 0, 0, 0, 0]
    assert res.summary()[0] == {"valued": 320, "out_of_view": 24, "occluded": 36, "visible": 260, "mismatch": 0,
                                "photo_l1": 0.0, "photo_rms": 0.0}


def test_graph_capture():
    """No allocation and no synchronisation: the stage is captured into a graph and replayed on new inputs."""
    n, H, W = 3, 5, 65
    disp, left, right = inputs(n, H, W)
    ref = reference(n, H, W, 0.5)
    chk = C.StereoCheck(n)
    d, l, r = torch.zeros(n, H, W, device=DEV), dev(left), dev(right)
    chk.run(d, l, r, photo_thr=THR)  # buffers made
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = chk.run(d, l, r, photo_thr=THR)
    d.copy_(dev(disp))
    g.replay()
    assert_outputs(host(res), ref)


# ---------------------------------------------------------------------- the hooks
MATCHER_KW = dict(num_disparities=16, block_size=5, speckle_window_size=10)


def test_classic_depth_batch_check(golden_dir):
    H, W, n = 24, 40, 2  # the smallest rigs of tests/test_gpu_sgm_batch.py
    rng = np.random.default_rng(12)
    pairs = [sgm_ref.shifted_bgr_scene(rng, H, W, 4 + i, noise=6) for i in range(n)]
    fl, fr = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    Q = np.load(golden_dir / "sgm_calib.npz")["Q"].astype(np.float64)
    rigs = sgm.ClassicDepthBatch(n, Q=Q, **MATCHER_KW)
    with pytest.raises(RuntimeError, match="before the first step"):
        rigs.check()
    res = rigs.step(fl, fr)
    got = host(rigs.check(occ_tol=0.5, photo_thr=40.0))
    disp, left, right = (t.cpu().numpy() for t in (res.disparity, res.rect_left, res.rect_right))
    assert np.isnan(disp).any() and (disp > 0).any()
    for i in range(n):
        ref = R.check(disp[i], left[i], right[i], 0.5, 40.0)
        assert_outputs({k: got[k][i:i + 1] for k in got},
                       {**{k: ref[k][None] for k in OUTPUTS}, "row": ref["row"][None]})
        assert np.array_equal(got["cls"][i] == 1, ~(np.isfinite(disp[i]) & (disp[i] > 0)))  # the NaN holes: class 1
    # step() is untouched by it: the same bytes as a rig that never ran a check
    other = sgm.ClassicDepthBatch(n, Q=Q, **MATCHER_KW).step(fl, fr)
    assert torch.equal(other.disparity_q4, res.disparity_q4) and torch.equal(other.disp_vis, res.disp_vis)
    # one rig
    one = sgm.ClassicDepth(Q=Q, **MATCHER_KW)
    with pytest.raises(RuntimeError, match="before the first step"):
        one.check()
    one.step(fl[1], fr[1])
    c1 = host(one.check(occ_tol=0.5, photo_thr=40.0))
    for k in got:
        assert c1[k][0].tobytes() == got[k][1].tobytes(), k


MODEL_HW = (32, 48)
FRAME_HW = (48, 64)


def tiny_model():
    from oracle import unet_ref as U
    from stereo_depth_estimation_amd.model import StereoUNet

    st = U.make_state(8, seed=0, signed_gamma=True)
    m = StereoUNet(base_channels=8, precision="fp32")
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV).eval()


def test_predictor_check_and_visible_only_cloud():
    from stereo_depth_estimation_amd import cloud as CL
    from stereo_depth_estimation_amd import predict as PR

    n, hw = 2, FRAME_HW
    rng = np.random.default_rng(3)
    left = rng.integers(0, 256, (n, *hw, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (n, *hw, 3), dtype=np.uint8)
    pred = PR.Predictor(tiny_model(), (MODEL_HW[1], MODEL_HW[0]))
    opts = C.CheckOptions(0.5, THR, write_check=True, ply_visible_only=True)
    cl = PR.CloudOptions(focal_px=30.0, baseline_m=0.1)
    res = pred.run(dev(left), dev(right), cloud=cl, check=opts)
    torch.cuda.synchronize()
    up = res["disp_up"].cpu().numpy()
    counts = res["counts"].cpu().numpy().view(np.uint32)
    Q = CL.pinhole_Q(30.0, 0.1, (hw[1] - 1) / 2, (hw[0] - 1) / 2)
    for k in range(n):
        ref = R.check(up[k], left[k], right[k], 0.5, THR)
        assert_outputs({"disp_vis": res["disp_vis"][k].cpu().numpy()[None], "vis_rgb": res["check_rgb"][k].cpu().numpy()[None],
                        "rows": res["check_rows"][k].cpu().numpy()[None]},
                       {"disp_vis": ref["disp_vis"][None], "vis_rgb": ref["vis_rgb"][None], "row": ref["row"][None]})
        assert 0 < (ref["cls"] == 0).sum() < ref["cls"].size
        # the records come from the visible pixels alone
        want = cloud_ref.records(ref["disp_vis"], Q, left[k], False)
        assert counts[k] == len(want) == (ref["cls"] == 0).sum()
        assert res["points"][k, :len(want)].cpu().numpy().tobytes() == want.tobytes()
    # the check alone (no cloud, no images): it holds the upsampled disparity itself, the same bytes
    alone = pred.run(dev(left), dev(right), images=False, check=C.CheckOptions(0.5, THR))
    torch.cuda.synchronize()
    assert alone["disp_up"].cpu().numpy().tobytes() == up.tobytes() and alone["check_rgb"] is None
    assert alone["check_rows"].cpu().numpy().tobytes() == res["check_rows"].cpu().numpy().tobytes()
    # without a check the result has none of its keys
    plain = pred.run(dev(left), dev(right))
    assert not ({"check_rows", "check_rgb", "disp_vis", "disp_up"} & set(plain))


def files_under(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


def test_predict_pairs_self_check(tmp_path):
    from PIL import Image

    from stereo_depth_estimation_amd import dataset as D
    from stereo_depth_estimation_amd import predict as PR

    H, W = MODEL_HW
    rng = np.random.default_rng(8)
    stems = [f"f{k}" for k in range(4)]
    frames = {}
    for side in ("left", "right"):
        (tmp_path / side).mkdir()
        for s in stems:
            frames[side, s] = rng.integers(0, 256, (*FRAME_HW, 3), dtype=np.uint8)
            Image.fromarray(frames[side, s]).save(tmp_path / side / f"{s}.png")
    model = tiny_model()
    common = dict(model=model, height=H, width=W, batch_size=3)
    out = tmp_path / "out"
    meta = PR.predict_pairs(None, tmp_path / "left", tmp_path / "right", out, self_check=True, write_check=True,
                            check_photo_thr=THR, **common)
    assert files_under(out) == sorted([f"{s}.png" for s in stems] + [f"{s}.check.png" for s in stems]
                                      + ["metrics.jsonl", "predict_meta.json"])
    assert json.loads((out / "predict_meta.json").read_text()) == meta
    assert (meta["self_check"], meta["check_occ_tol"], meta["check_photo_thr"], meta["write_check"],
            meta["ply_visible_only"]) == (True, 0.5, THR, True, False)
    recs = [json.loads(s) for s in (out / "metrics.jsonl").read_text().splitlines()]
    assert [r["sample"] for r in recs] == [f"{s}.png" for s in stems]
    assert all(set(r) == {"sample", *C.SUMMARY_KEYS} for r in recs)
    # the rows behind the figures, and the pictures: Predictor.run on the same batches
    pred = PR.Predictor(model, (W, H))
    rows = []
    for b in (stems[:3], stems[3:]):
        l, r = (dev(np.stack([frames[side, s] for s in b])) for side in ("left", "right"))
        res = pred.run(l, r, check=C.CheckOptions(0.5, THR, write_check=True))
        torch.cuda.synchronize()
        rows.append(res["check_rows"].cpu().numpy())
        for k, s in enumerate(b):
            assert np.array_equal(D.read_rgb_uint8(out / f"{s}.check.png"), res["check_rgb"][k].cpu().numpy()), s
            assert D.read_rgb_uint8(out / f"{s}.png").tobytes() == res["disp_rgb"][k].cpu().numpy().tobytes()
    rows = np.concatenate(rows)
    assert [{k: r[k] for k in C.SUMMARY_KEYS} for r in recs] == [C.summary_from_row(r) for r in rows]
    assert meta["check"] == C.aggregate_rows(rows) and meta["check"]["photo_l1"] > 0
    assert meta["check"]["valued"] == 4 * FRAME_HW[0] * FRAME_HW[1]  # softplus disparities: every pixel has a value

    # without the flags: the files of before and nothing else, the same bytes, none of the new keys
    plain = tmp_path / "plain"
    meta0 = PR.predict_pairs(None, tmp_path / "left", tmp_path / "right", plain, **common)
    assert files_under(plain) == sorted([f"{s}.png" for s in stems] + ["predict_meta.json"])
    for s in stems:
        assert (plain / f"{s}.png").read_bytes() == (out / f"{s}.png").read_bytes()
    assert not ({"check", "self_check", "check_occ_tol", "check_photo_thr", "write_check", "ply_visible_only"} & set(meta0))
    volatile = {"output_root", "elapsed_seconds", "created_at_unix", "check", *C.CheckOptions().describe()}
    assert {k: v for k, v in meta.items() if k not in volatile} == {k: v for k, v in meta0.items() if k not in volatile}

    # the command line, with a visible-only cloud
    ck = tmp_path / "best.pt"
    torch.save({"epoch": 1, "model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()},
                "args": {"height": H, "width": W}, "metrics": {}}, ck)
    out2 = tmp_path / "out_cli"
    base = ["--checkpoint", str(ck), "--left-dir", str(tmp_path / "left"), "--right-dir", str(tmp_path / "right"),
            "--output-root", str(out2), "--base-channels", "8", "--batch-size", "3", "--write-ply", "--focal-px", "30",
            "--baseline-m", "0.1"]
    meta2 = PR.main(base + ["--self-check", "--check-photo-thr", str(THR), "--ply-visible-only"])
    assert meta2["check"] == meta["check"] and meta2["ply_visible_only"] is True
    assert meta2["points"] == meta["check"]["visible"]  # one point per visible pixel
    with pytest.raises(ValueError, match="only with --self-check"):
        PR.main(base + ["--ply-visible-only"])
    with pytest.raises(ValueError, match="--ply-visible-only needs --write-ply"):
        PR.predict_pairs(None, tmp_path / "left", tmp_path / "right", tmp_path / "never", self_check=True,
                         ply_visible_only=True, **common)
    assert not (tmp_path / "never").exists()
