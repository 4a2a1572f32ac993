"""The label-free adaptation loss on the device (csrc/selfsup.hip: sd_selfsup_loss; stereo_depth_estimation_amd/selfsup.py
and adapt.py; needs an MI355X).

The reference is always the float64 evaluation of the NumPy restatement tests/selfsup_ref.py. The counts (``count``,
rows[0], rows[4]) are equal. The bound of everything else is derived from the restatement's own float32 evaluation,
which rounds every operation as the kernel does: the device differs from it only in ``exp`` (the project documents 4
ulp) and in the order of its sums, so a per-pixel gradient gets 4 x max |ref32 - ref64| over the case, with a floor of
16 float32 ulps of the case's largest gradient term; a sum of k terms gets k times the per-term bound of the same form
plus k * 2^-53 * value for its fp64 additions in another order than NumPy's. Division and square root are correctly
rounded in this build (the kernel asks for the round-to-nearest forms by name), and on an MI355X the worst ratio of an
error to that bound over every case of this file was 0.25 for the gradients and 0.13 for the sums, so
the tests hold the device to half of it: BOUND_FACTOR = 2, BOUND_FLOOR_ULPS = 8. The kernels have one fixed order and
no atomics, so the errors are the same on every run.

Shapes come from the kernel's own constant P = STEP_PIXELS, the pixels of one step of the row walk (four per thread, 64
lanes, four waves): one pixel, less than a thread's four, around a wave-quarter (63, 64, 65), around one step (P - 1, P,
P + 1) and two steps and a partial third (2P + 5), with one row, two rows and several rows per block, one and three
samples. Every shape runs with and without logvar, with both weights, with w_photo = 0 and with w_smooth = 0, and with
buffers that start 0, 1 and 3 elements into their allocation (so the scalar path runs where W % 4 == 0 too).
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import selfsup_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import selfsup as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = S.STEP_PIXELS
WIDTHS = [1, 2, 3, 63, 64, 65, P - 1, P, P + 1, 2 * P + 5]
WEIGHTS = ((1.0, 0.1), (0.0, 0.1), (1.0, 0.0))  # (w_photo, w_smooth)
OFFSETS = (0, 1, 3)
ULP32 = 2.0 ** -23
GUARD = 16  # elements of 0xFF bytes on both sides of every output
LEARN_LR = 3e-2
BOUND_FACTOR, BOUND_FLOOR_ULPS = 2.0, 8.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


_inputs, _refs = {}, {}


def inputs(n, H, W):
    """The generator's inputs of one shape and the geometry-only classes of the restatement: made once, read-only."""
    key = (n, H, W)
    if key not in _inputs:
        disp, logvar, x = R.random_case(n, H, W, seed=1000 * W + 10 * H + n)
        cls, crows = R.classes(disp)
        arrs = (disp, logvar, x, cls, crows)
        for a in arrs:
            a.setflags(write=False)
        _inputs[key] = arrs
    return _inputs[key]


def reference(n, H, W, with_lv, weights):
    """(float64, float32) evaluations of the restatement: computed once per case, shared, read-only."""
    key = (n, H, W, with_lv, weights)
    if key not in _refs:
        disp, logvar, x, cls, crows = inputs(n, H, W)
        kw = dict(w_photo=weights[0], w_smooth=weights[1])
        _refs[key] = tuple(R.loss(disp, logvar if with_lv else None, x, cls, crows, dtype=t, **kw)
                           for t in (np.float64, np.float32))
    return _refs[key]


def placed(a: np.ndarray, off: int, fill=0xFF):
    """``a`` on the device, ``off`` elements into an allocation of 0xFF bytes (guards on both sides). Returns (the
    allocation as bytes, the view)."""
    t = torch.as_tensor(np.array(a, order="C"))
    es = t.element_size()
    raw = torch.full(((t.numel() + off + 2 * GUARD) * es + 64,), fill, dtype=torch.uint8, device=DEV)
    start = (GUARD + off) * es
    view = raw[start:start + t.numel() * es].view(t.dtype).view(t.shape)
    view.copy_(t)
    return raw, view


def guards_untouched(raw, view):
    es = view.element_size()
    start = view.data_ptr() - raw.data_ptr()
    end = start + view.numel() * es
    return bool((raw[:start] == 0xFF).all()) and bool((raw[end:] == 0xFF).all())


def run_device(n, H, W, disp, logvar, x, weights, off=0, check_rows=None, occ_tol=0.5):
    """sd_stereo_check (geometry only) and sd_selfsup_loss on buffers ``off`` elements into their allocations. Returns
    numpy outputs and whether every guard survived."""
    s = L.stream_handle(torch.device(DEV))
    bufs = {"disp": placed(disp, off), "x": placed(x, off), "cls": placed(np.zeros((n, H, W), np.uint8), off),
            "gdisp": placed(np.zeros((n, H, W), np.float32), off)}
    if logvar is not None:
        bufs["logvar"] = placed(logvar, off)
        bufs["glogvar"] = placed(np.zeros((n, H, W), np.float32), off)
    crows = torch.zeros(n, 8, dtype=torch.float64, device=DEV)
    rows = torch.full((n, 8), -1.0, dtype=torch.float64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    cwork = torch.empty(L.call("sd_stereo_check_ws_bytes", n, H, W) // 8, dtype=torch.float64, device=DEV)
    work = torch.full((L.call("sd_selfsup_ws_bytes", n, H, W) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    ptr = lambda k: bufs[k][1].data_ptr() if k in bufs else None  # noqa: E731
    L.call("sd_stereo_check", n, ptr("disp"), None, None, H, W, occ_tol, float("inf"), ptr("cls"), None, None, None,
           crows.data_ptr(), cwork.data_ptr(), s)
    if check_rows is not None:
        crows.copy_(torch.as_tensor(check_rows))
    L.call("sd_selfsup_loss", n, ptr("disp"), ptr("logvar"), ptr("x"), ptr("cls"), crows.data_ptr(), H, W,
           weights[0], weights[1], 0.01, 0.01, 10.0, ptr("gdisp"), ptr("glogvar"), rows.data_ptr(), count.data_ptr(),
           work.data_ptr(), s)
    torch.cuda.synchronize()
    out = {k: bufs[k][1].cpu().numpy() for k in ("cls", "gdisp", "glogvar") if k in bufs}
    out.update(rows=rows.cpu().numpy(), count=int(count.item()), check_rows=crows.cpu().numpy(),
               guards=all(guards_untouched(*bufs[k]) for k in bufs))
    return out


def term_bound(a32, a64):
    """The per-term bound of the module docstring for one quantity of a case."""
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    if a64.size == 0:
        return 0.0
    return max(BOUND_FACTOR * float(np.abs(a32 - a64).max()), BOUND_FLOOR_ULPS * ULP32 * float(np.abs(a64).max()))


worst = {"grad": 0.0, "sum": 0.0}


def assert_case(got, r64, r32, with_lv, disp):
    """The counts equal, the gradients and the sums within the derived bound of the float64 restatement."""
    assert got["guards"]
    assert got["count"] == r64["count"]
    assert np.array_equal(got["rows"][:, [0, 4]], r64["rows"][:, [0, 4]])
    assert (got["rows"][:, 6:] == 0).all()
    gb = max(BOUND_FACTOR * float(np.abs(r32["gdisp"].astype(np.float64) - r64["gdisp"]).max()),
             BOUND_FLOOR_ULPS * ULP32 * r64["gterm"])
    pairs = [("gdisp", gb)]
    if with_lv:
        pairs.append(("glogvar", max(BOUND_FACTOR * float(np.abs(r32["glogvar"].astype(np.float64) - r64["glogvar"]).max()),
                                     BOUND_FLOOR_ULPS * ULP32 * r64["gterm"])))
    else:
        assert "glogvar" not in got
    for k, b in pairs:
        assert np.isfinite(got[k]).all()
        err = float(np.abs(got[k].astype(np.float64) - r64[k]).max())
        print(f"{k}: err {err:.3e} bound {b:.3e}")
        if b > 0:
            worst["grad"] = max(worst["grad"], err / b)
        assert err <= b, (k, err, b)
    assert (got["gdisp"][~np.isfinite(disp)] == 0).all()
    n = got["rows"].shape[0]
    for col, per32, per64 in ((1, r32["l"], r64["l"]), (2, r32["e"], r64["e"]), (3, r32["terms"], r64["terms"]),
                              (5, np.abs(r32["gdisp"]).reshape(n, -1), np.abs(r64["gdisp"]).reshape(n, -1))):
        k = per64.shape[1]
        per = gb if col == 5 else term_bound(per32, per64)
        for i in range(n):
            b = k * per + k * 2.0 ** -53 * float(np.abs(per64[i]).sum())
            err = abs(got["rows"][i, col] - r64["rows"][i, col])
            print(f"rows[{i}][{col}]: err {err:.3e} bound {b:.3e}")
            if b > 0:
                worst["sum"] = max(worst["sum"], err / b)
            assert err <= b, (col, i, err, b)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 5])
@pytest.mark.parametrize("W", WIDTHS)
def test_outputs_within_the_derived_bound(W, H, n):
    disp, logvar, x, cls, crows = inputs(n, H, W)
    for li, with_lv in enumerate((True, False)):
        for wi, weights in enumerate(WEIGHTS):
            off = OFFSETS[(wi + li) % 3]
            r64, r32 = reference(n, H, W, with_lv, weights)
            got = run_device(n, H, W, disp, logvar if with_lv else None, x, weights, off)
            assert np.array_equal(got["cls"], cls) and np.array_equal(got["check_rows"], crows)
            assert_case(got, r64, r32, with_lv, disp)
    print("worst ratio so far:", worst)


@pytest.mark.parametrize("W", [64, P + 1])
def test_two_runs_and_both_paths_give_equal_bytes(W):
    """Two runs give equal bytes, and the vector path (offset 0, W % 4 == 0) the scalar path's (offset 1)."""
    n, H = 3, 5
    disp, logvar, x, _, _ = inputs(n, H, W)
    a = run_device(n, H, W, disp, logvar, x, WEIGHTS[0], 0)
    for off in (0, 1):
        b = run_device(n, H, W, disp, logvar, x, WEIGHTS[0], off)
        for k in ("gdisp", "glogvar", "rows"):
            assert a[k].tobytes() == b[k].tobytes(), (k, off)
        assert a["count"] == b["count"] and b["guards"]


@pytest.mark.parametrize("W", [65, P])
def test_a_stream_does_not_depend_on_its_neighbours(W):
    """Sample i alone (n = 1), with the batch's normaliser handed over in check_rows, gives the bytes it has in the batch
    of three."""
    n, H = 3, 5
    disp, logvar, x, _, crows = inputs(n, H, W)
    full = run_device(n, H, W, disp, logvar, x, WEIGHTS[0], 0)
    total = np.zeros((1, 8))
    total[0, 0] = R.normaliser(crows)[0]
    assert total[0, 0] > 0
    for i in range(n):
        one = run_device(1, H, W, disp[i:i + 1], logvar[i:i + 1], x[i:i + 1], WEIGHTS[0], 0, check_rows=total)
        assert one["count"] == full["count"]
        # w_smooth / float32(M): M is the batch's pixel count, so the smoothness share differs by that known factor;
        # the photometric bytes are compared with the smoothness weight 0 below
        assert one["rows"][0, [0, 1, 2, 3, 4]].tobytes() == full["rows"][i, [0, 1, 2, 3, 4]].tobytes()
        assert one["glogvar"].tobytes() == full["glogvar"][i:i + 1].tobytes()
    full = run_device(n, H, W, disp, logvar, x, WEIGHTS[2], 0)
    for i in range(n):
        one = run_device(1, H, W, disp[i:i + 1], logvar[i:i + 1], x[i:i + 1], WEIGHTS[2], 0, check_rows=total)
        for k in ("gdisp", "glogvar"):
            assert one[k].tobytes() == full[k][i:i + 1].tobytes(), (k, i)
        assert one["rows"].tobytes() == full["rows"][i:i + 1].tobytes()


def test_nothing_counted_and_the_class_api():
    """A batch without a counted pixel: count 0, normaliser 1, zero photometric gradient. And SelfSupLoss.run: the same
    numbers through the class, its summary from the rows, its totals."""
    n, H, W = 2, 5, 65
    disp, logvar, x, cls, crows = inputs(3, H, W)
    disp, logvar, x, cls, crows = disp[:n], logvar[:n], x[:n], cls[:n], crows[:n]
    none = run_device(n, H, W, np.full_like(disp, -1.0), logvar, x, WEIGHTS[2], 0)
    assert none["count"] == 0 and (none["gdisp"] == 0).all() and (none["glogvar"] == 0).all()
    assert (none["rows"][:, [0, 1, 2, 5]] == 0).all() and (none["rows"][:, 3:5] > 0).all()  # flat: the terms are w eps_s
    loss = S.SelfSupLoss(3)
    d, lv, xs = (torch.as_tensor(np.array(a)).to(DEV) for a in (disp, logvar, x))
    res = loss.run(d, lv, xs)
    res2_rows = res.rows.clone()
    r64 = R.loss(disp, logvar, x, cls, crows)
    r32 = R.loss(disp, logvar, x, cls, crows, dtype=np.float32)
    torch.cuda.synchronize()
    got = {"gdisp": res.gdisp.cpu().numpy(), "glogvar": res.glogvar.cpu().numpy(), "rows": res.rows.cpu().numpy(),
           "count": int(res.count.item()), "guards": True}
    assert np.array_equal(res.cls.cpu().numpy(), cls)
    assert_case(got, r64, r32, True, disp)
    s = res.summary()
    want = S.summary_from_rows(r64["rows"], n * H * W, loss.w_photo, loss.w_smooth)
    assert set(s) == set(S.SUMMARY_KEYS)
    for k in S.SUMMARY_KEYS:
        assert s[k] == pytest.approx(want[k], rel=1e-5), k
    assert s["loss"] == pytest.approx(r64["total"], rel=1e-5)
    loss.run(d[:, None], lv[:, None], xs)  # [n, 1, H, W] as the heads write it; the totals now hold two runs
    m = loss.means()
    assert m["steps"] == 2 and m["photo"] == pytest.approx(want["photo"], rel=1e-5)
    assert m["visible_fraction"] == pytest.approx(r64["count"] / (n * H * W), rel=1e-12)
    assert torch.equal(res.rows, res2_rows)  # the second run wrote the same rows into the same buffer
    plain = S.SelfSupLoss(3, uncertainty=False).run(d, None, xs)
    assert plain.glogvar is None and int(plain.count.item()) == r64["count"]
    with pytest.raises(ValueError, match="needs the logvar"):
        loss.run(d, None, xs)
    with pytest.raises(ValueError, match="inputs must be"):
        loss.run(d, lv, xs[:, :5])


def small_model(precision="fp32", seed=0):
    from stereo_depth_estimation_amd.model import StereoUNet

    torch.manual_seed(seed)
    return StereoUNet(base_channels=8, precision=precision).to(DEV).train()


def ramp_scene(n=2, H=32, W=64, seed=0, passes=6, d0=2.0, d1=6.0):
    """Low-pass-filtered noise; the left view is the right one warped by a known disparity ramp (2 px at the left edge
    to 6 px at the right). Returns inputs float32 [n, 6, H, W] in [0, 1]."""
    rng = np.random.default_rng(seed)
    noise = rng.random((n, 3, H, W + 16))
    k = np.array([1, 4, 6, 4, 1], dtype=np.float64) / 16
    for _ in range(passes):
        noise = sum(k[j] * np.roll(noise, j - 2, axis=3) for j in range(5))
        noise = sum(k[j] * np.roll(noise, j - 2, axis=2) for j in range(5))
    right = (noise - noise.min()) / (noise.max() - noise.min())
    d = np.linspace(d0, d1, W)[None, None, None, :]
    xr = np.arange(W)[None, None, None, :] - d + 8  # the right view's columns start 8 into the noise
    x0 = np.floor(xr).astype(np.int64)
    f = xr - x0
    x0 = np.broadcast_to(x0, (n, 3, H, W))
    left = np.take_along_axis(right, x0, 3) * (1 - f) + np.take_along_axis(right, x0 + 1, 3) * f
    return np.concatenate([left, right[..., 8:8 + W]], axis=1).astype(np.float32)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_adapt_step_gradients_equal_the_autograd_bridge(precision):
    """adapt_step's flat gradient buffer against the gradients through the existing autograd bridge fed with
    SelfSupLoss.run's maps on the same outputs: both routes run the same kernels, so they are equal bit for bit."""
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x = torch.as_tensor(ramp_scene(seed=3)).to(DEV)
    m = small_model(precision, seed=1)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    loss = S.SelfSupLoss(2)
    disp, logvar = m(x, return_uncertainty=True)
    res = loss.run(disp.detach(), logvar.detach(), x)
    gd, gl = res.gdisp.clone()[:, None], res.glogvar.clone()[:, None]
    torch.autograd.backward((disp, logvar), (gd, gl))
    want = m.flat_buffers()[1].clone()
    assert float(want.abs().sum()) > 0

    m2 = small_model(precision, seed=1)
    m2.load_state_dict(state)
    m2 = m2.to(DEV).train()
    opt = FusedAdamW(m2.parameters(), lr=0.0, weight_decay=0.0)
    res2 = S.adapt_step(m2, opt, x, S.SelfSupLoss(2))
    assert torch.equal(res2.gdisp, gd[:, 0]) and torch.equal(res2.glogvar, gl[:, 0])
    assert int(res2.count.item()) == int(res.count.item()) > 0
    assert torch.equal(m2.flat_buffers()[1], want)


def test_a_batch_that_counts_nothing_leaves_the_weights():
    """The AdamW gate: with classes that count nothing (a disparity past the row everywhere: occ_tol is irrelevant, every
    pixel is out of view) the parameters are unchanged bit for bit after the step; with the scene's own classes they
    move."""
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x = torch.as_tensor(ramp_scene(seed=4)).to(DEV)
    m = small_model(seed=2)
    opt = FusedAdamW(m.parameters(), lr=1e-2, weight_decay=1e-2)
    with torch.no_grad():
        m.disparity_head.bias.fill_(200.0)  # softplus(~200) > W = 64: every pixel looks left of the right image
    m.engine(DEV)
    before = m.flat_buffers()[0].clone()
    res = S.adapt_step(m, opt, x, S.SelfSupLoss(2))
    assert int(res.count.item()) == 0 and bool((res.cls == 2).all())
    assert float(res.gdisp.abs().sum()) > 0  # the smoothness gradient is there; only the update is gated
    assert torch.equal(m.flat_buffers()[0], before)
    with torch.no_grad():
        m.disparity_head.bias.fill_(0.0)
    before = m.flat_buffers()[0].clone()
    res = S.adapt_step(m, opt, x, S.SelfSupLoss(2))
    assert int(res.count.item()) > 0 and not torch.equal(m.flat_buffers()[0], before)


def test_it_learns():
    """20 adapt_steps on the ramp scene with a fixed seed: the mean photometric loss of the last 5 steps is below that
    of the first 5. The learning rate was chosen on an MI355X among 1e-3, 3e-3, 1e-2 and 3e-2: at 3e-2 the
    means were 0.0854 and 0.0700 with this seed and 0.0852 and 0.0510 with the next, at 1e-3 the difference was within
    the noise of 20 steps."""
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x = torch.as_tensor(ramp_scene(seed=0)).to(DEV)
    m = small_model(seed=0)
    opt = FusedAdamW(m.parameters(), lr=LEARN_LR, weight_decay=0.0)
    loss = S.SelfSupLoss(2)
    photo = []
    for _ in range(20):
        photo.append(S.adapt_step(m, opt, x, loss).summary()["photo"])
    first, last = float(np.mean(photo[:5])), float(np.mean(photo[-5:]))
    print(f"lr {LEARN_LR}: photo first 5 {first:.5f}, last 5 {last:.5f}")
    assert all(p is not None for p in photo)
    assert last < first, (first, last)
    assert loss.means()["steps"] == 20


def test_adapt_tool(tmp_path):
    """The tool on 4 synthetic PNG pairs, 1 epoch at 32 x 64: adapted.pt loads through cli.load_checkpoint, and
    adapt_meta.json holds the stated keys."""
    from PIL import Image

    from stereo_depth_estimation_amd import adapt as A
    from stereo_depth_estimation_amd import cli
    from stereo_depth_estimation_amd.model import StereoUNet
    from stereo_depth_estimation_amd.optim import FusedAdamW

    frames = (ramp_scene(4, 32, 64, seed=9) * 255).round().astype(np.uint8)
    for side, sl in (("left", slice(0, 3)), ("right", slice(3, 6))):
        (tmp_path / side).mkdir()
        for i in range(4):
            Image.fromarray(np.ascontiguousarray(frames[i, sl].transpose(1, 2, 0))).save(tmp_path / side / f"{i:03d}.png")
    src = small_model(seed=5)
    cfg = cli.parse_args(["--height", "32", "--width", "64", "--output-dir", str(tmp_path)])
    cli.save_checkpoint(tmp_path / "src.pt", 3, src, FusedAdamW(src.parameters()), cfg, {"val_mae": 1.0})
    meta = A.main(["--checkpoint", str(tmp_path / "src.pt"), "--left-dir", str(tmp_path / "left"), "--right-dir",
                   str(tmp_path / "right"), "--output-dir", str(tmp_path / "out"), "--base-channels", "8",
                   "--batch-size", "2", "--lr", "1e-4"])
    on_disk = json.loads((tmp_path / "out" / "adapt_meta.json").read_text())
    assert on_disk == json.loads(json.dumps(meta))
    for k in ("checkpoint", "left_dir", "right_dir", "output_dir", "height", "width", "epochs", "batch_size", "lr",
              "weight_decay", "precision", "w_smooth", "edge_gamma", "occ_tol", "uncertainty", "max_samples", "seed",
              "epochs_run", "photo_first", "photo_last", "epe_before", "epe_after", "num_samples", "rectified"):
        assert k in meta, k
    assert (meta["height"], meta["width"], meta["num_samples"], meta["num_batches"]) == (32, 64, 4, 2)
    assert len(meta["epochs_run"]) == 1 and set(meta["epochs_run"][0]) == {"loss", "photo", "smooth", "visible_fraction"}
    assert meta["photo_first"] == meta["photo_last"] == meta["epochs_run"][0]["photo"] > 0
    assert meta["epe_before"] is None and 0 < meta["epochs_run"][0]["visible_fraction"] <= 1
    back = StereoUNet(base_channels=8)
    ck = cli.load_checkpoint(tmp_path / "out" / "adapted.pt", back, None, DEV)
    assert ck["epoch"] == 3 and ck["args"]["height"] == 32 and ck["args"]["lr"] == 1e-4
    moved = [k for k, v in src.state_dict().items() if not torch.equal(v.cpu(), back.state_dict()[k].cpu())]
    assert any(k.endswith("weight") for k in moved)


def test_adapt_tool_with_labels_measures_epe(tmp_path):
    """--dataset-root: the labels are not trained on, they measure. EPE before and after come from sd_disp_export's rows
    over all samples (before: what predict_dataset reports for the same model), and the model handed in is the one
    adapted (no checkpoint is read)."""
    from conftest import write_stereo_tree

    from stereo_depth_estimation_amd import adapt as A
    from stereo_depth_estimation_amd import predict as Pr

    write_stereo_tree(tmp_path / "data", scenes=2, frames=2, hw=(45, 61), seed=3)
    m = small_model(seed=6)
    want = Pr.predict_dataset(None, tmp_path / "data", model=m, height=32, width=64)["epe"]
    start = m.flat_buffers()[0].clone()
    meta = A.adapt(None, model=m, dataset_root=tmp_path / "data", output_dir=tmp_path / "out", height=32, width=64,
                   batch_size=3, epochs=2, lr=1e-3)
    assert meta["epe_before"] == want and meta["epe_after"] is not None and meta["epe_after"] != meta["epe_before"]
    assert (meta["num_samples"], meta["num_batches"], len(meta["epochs_run"])) == (4, 2, 2)
    assert meta["photo_first"] == meta["epochs_run"][0]["photo"] and meta["photo_last"] == meta["epochs_run"][1]["photo"]
    assert not torch.equal(m.flat_buffers()[0], start) and not m.training
    assert (tmp_path / "out" / "adapted.pt").exists() and (tmp_path / "out" / "adapt_meta.json").exists()
