"""Epoch previews on the GPU: sd_quantile_select_n and sd_preview_compose_n against the NumPy restatement
(tests/preview_ref.py) and the reference's own montages (tests/golden/preview.npz), batches against single calls, graph
capture, argument validation, log_epoch_previews end to end, and cli.main with previews on and off (the training
trajectory must not move).

Tolerances. The order statistics and n are exact. lo / hi: the device evaluates v[k] + (v[k+1] - v[k]) * g in fp64 and
rounds to float32 once; a contraction of the fp64 expression into an fma would move it by one fp64 ulp, so at most one
float32 step is allowed (sd_live_select's margin). The montage is byte-equal to the restatement evaluated with the
device's own lo / hi; against the reference's montages the colour panels are byte-equal and the map panels within one
code (a one-step change of vmin or scale moves x * 255 by far less than 1)."""

from __future__ import annotations

import sys
import types

import numpy as np
import pytest
import torch

import preview_ref
from conftest import GOLDEN, write_stereo_tree

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Q = (preview_ref.Q_LO, preview_ref.Q_HI)


@pytest.fixture(scope="module")
def L():
    from stereo_depth_estimation_amd import _lib

    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "preview.npz")


def _select(L, maps, q=Q):
    """maps: m arrays of one size -> (sel f32 [m][8] as numpy, the work buffer after the call)."""
    v = torch.as_tensor(np.stack([np.asarray(m, dtype=np.float32).reshape(-1) for m in maps])).to(DEV)
    m, count = v.shape
    work = torch.zeros(L.call("sd_quantile_select_ws_bytes", m) // 4, dtype=torch.int32, device=DEV)
    sel = torch.full((m, 8), 7.0, dtype=torch.float32, device=DEV)
    L.call("sd_quantile_select_n", m, v.data_ptr(), count, q[0], q[1], work.data_ptr(), sel.data_ptr(),
           L.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    return sel.cpu().numpy(), work


def _within_one_step(got, want) -> bool:
    got, want = np.float32(got), np.float32(want)
    return bool(got == want or got == np.nextafter(want, np.float32(np.inf)) or got == np.nextafter(want, np.float32(-np.inf)))


def _check_sel(row, values, q=Q):
    want = preview_ref.quantile_select(values, *q)
    assert int(row[:1].view(np.uint32)[0]) == want["n"]
    if want["n"] == 0:
        assert np.isnan(row[1:7]).all()
        return
    assert np.array_equal(row[1:5], want["stats"]), (row[1:5], want["stats"])  # as numbers: -0 == +0
    nz = want["stats"] != 0
    assert np.array_equal(row[1:5][nz].view(np.uint32), want["stats"][nz].view(np.uint32))
    assert _within_one_step(row[5], want["lo"]) and _within_one_step(row[6], want["hi"]), (row[5:7], want["lo"], want["hi"])


def _holes(rng, shape, frac=0.1):
    m = rng.normal(5.0, 30.0, shape).astype(np.float32)
    flat = m.reshape(-1)
    idx = rng.choice(flat.size, int(frac * flat.size), replace=False)
    flat[idx] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)[rng.integers(0, 5, idx.size)]
    return m


def _select_cases():
    rng = np.random.default_rng(77)
    nan = np.full((6, 9), np.nan, dtype=np.float32)
    nan[1, ::2] = np.inf
    nan[2, 1::2] = -np.inf
    one = nan.copy()
    one[3, 4] = -7.25
    two = one.copy()
    two[5, 0] = 2.5
    zeros = np.array([0.0, -0.0] * 40 + [1.0, -1.0], dtype=np.float32)
    rng.shuffle(zeros)
    # duplicates around both percentiles: 1000 values, ranks 49.95 and 949.05 inside runs of equal values and at their ends
    dup = np.concatenate([np.full(50, -3.0), np.full(1, -2.0), np.full(898, 1.5), np.full(1, 4.0), np.full(50, 9.0)])
    dup = dup.astype(np.float32)
    rng.shuffle(dup)
    dup2 = np.repeat(np.arange(25, dtype=np.float32) / 4 - 2, 40)
    rng.shuffle(dup2)
    return {
        "5x7": rng.normal(0.0, 3.0, (5, 7)).astype(np.float32),
        "33x50": rng.uniform(-2.0, 90.0, (33, 50)).astype(np.float32),
        "48x64_holes": _holes(rng, (48, 64)),
        "one_value": one,
        "two_values": two,
        "all_nan": nan,
        "negatives_only": -rng.uniform(1e-3, 50.0, (17, 13)).astype(np.float32),
        "mixed_zeros": zeros,
        "duplicates": dup,
        "duplicates_runs": dup2,
        "constant_240x320": np.full((240, 320), 3.5, dtype=np.float32),
        "target_like": np.where(rng.random((48, 64)) < 0.4, 0.0, rng.uniform(0.5, 90.0, (48, 64))).astype(np.float32),
        "denormals_and_huge": np.array([1e-45, -1e-45, 3e38, -3e38, 1e-40, 0.0, 1.0, -1.0, 2.0] * 5, dtype=np.float32),
    }


SELECT_CASES = _select_cases()


@pytest.mark.parametrize("name", list(SELECT_CASES))
def test_select_matches_restatement(L, name):
    values = SELECT_CASES[name]
    sel, work = _select(L, [values])
    _check_sel(sel[0], values)
    assert not work.any()


def test_select_other_quantiles(L):
    values = SELECT_CASES["48x64_holes"]
    for q in ((0.0, 1.0), (0.5, 0.5), (0.02, 0.98), (0.0, 0.0), (1.0, 1.0)):
        sel, work = _select(L, [values], q)
        _check_sel(sel[0], values, q)
        assert not work.any()


@pytest.mark.parametrize("m", [1, 3, 8])
def test_select_batch_equals_single_calls(L, m):
    rng = np.random.default_rng(m)
    maps = [_holes(rng, (48, 64), frac=0.05 * i) for i in range(m)]
    if m >= 3:
        maps[1] = np.full((48, 64), np.nan, dtype=np.float32)  # a map without a finite value between two others
    sel, work = _select(L, maps)
    assert not work.any()
    for i, values in enumerate(maps):
        _check_sel(sel[i], values)
        single, _ = _select(L, [values])
        assert np.array_equal(sel[i, :7].view(np.uint32), single[0, :7].view(np.uint32))
    # a second call on the same (zero again) workspace gives the same rows
    v = torch.as_tensor(np.stack([x.reshape(-1) for x in maps])).to(DEV)
    sel2 = torch.zeros((m, 8), dtype=torch.float32, device=DEV)
    for _ in range(2):
        L.call("sd_quantile_select_n", m, v.data_ptr(), v.shape[1], Q[0], Q[1], work.data_ptr(), sel2.data_ptr(),
               L.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert np.array_equal(sel2.cpu().numpy()[:, :7].view(np.uint32), sel[:, :7].view(np.uint32)) and not work.any()


def _two_rules_cases():
    rng = np.random.default_rng(5)
    return {
        "37x53_wide": np.exp(rng.normal(0.0, 3.0, (37, 53))).astype(np.float32),  # a ragged last block
        "160x200_narrow": (5.0 + 1e-4 * rng.random((160, 200))).astype(np.float32),  # four ranks in one level-1 bin
        "1x1": np.array([[2.75]], dtype=np.float32),  # n = 1, 2: every rank clamped
        "1x2": np.array([[9.5, 0.125]], dtype=np.float32),
        "8x8_repeated": np.full((8, 8), 3.5, dtype=np.float32),
    }


TWO_RULES_CASES = _two_rules_cases()


@pytest.mark.parametrize("name", list(TWO_RULES_CASES))
def test_live_and_preview_rules_share_one_select(L, name):
    """The two rule sets of the shared radix select on a map whose members are the same under both (finite, > 0):
    sd_live_select_n and sd_quantile_select_n with q = 0.02, 0.98 agree on n and on the four order statistics bit for
    bit. lo / hi follow each rule's own restatement (numpy's _lerp there, a + d g here; one float32 step, as the
    tests of each stage allow), not each other. Each runs twice on its work buffer, which is zero again afterwards."""
    m = TWO_RULES_CASES[name]
    assert np.isfinite(m).all() and (m > 0).all()
    h, w = m.shape
    q = (0.02, 0.98)
    dev = torch.device(DEV)
    v = torch.as_tensor(m).to(dev)
    s = L.stream_handle(dev)
    work_l = torch.zeros(L.call("sd_live_select_n_ws_bytes", 1) // 4, dtype=torch.int32, device=dev)
    work_p = torch.zeros(L.call("sd_quantile_select_ws_bytes", 1) // 4, dtype=torch.int32, device=dev)
    sel_l, sel_p = torch.full((1, 8), 7.0, device=dev), torch.full((1, 8), 7.0, device=dev)
    for _ in range(2):
        L.call("sd_live_select_n", 1, v.data_ptr(), h, w, work_l.data_ptr(), sel_l.data_ptr(), None, 0, s)
        L.call("sd_quantile_select_n", 1, v.data_ptr(), h * w, q[0], q[1], work_p.data_ptr(), sel_p.data_ptr(), s)
    torch.cuda.synchronize()
    assert not work_l.any() and not work_p.any()
    live, prev = sel_l.cpu().numpy()[0], sel_p.cpu().numpy()[0]
    assert int(live[:1].view(np.uint32)[0]) == int(prev[:1].view(np.uint32)[0]) == m.size
    assert np.array_equal(live[1:5].view(np.uint32), prev[1:5].view(np.uint32)), (live[1:5], prev[1:5])
    _check_sel(prev, m, q)
    srt = np.sort(m.reshape(-1)).astype(np.float64)  # sd_live_select's lo, hi: tests/test_gpu_live.py _percentiles64
    for got, qq in zip(live[5:7], q):
        vi = (srt.size - 1) * qq
        k = int(np.floor(vi))
        a, b = srt[k], srt[min(k + 1, srt.size - 1)]
        assert _within_one_step(got, np.float32(a + (b - a) * (vi - k))), (got, a, b, vi)


# ---------------------------------------------------------------------------------------------------- montage
def _device_montage(L, inp, tgt, pred):
    """The three ABI calls on a batch (numpy [n][6][H][W], [n][H][W] x 2) -> (montage u8, sel_t, sel_p) as numpy."""
    n, _, H, W = inp.shape
    dev = torch.device(DEV)
    x, t, p = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (inp, tgt, pred))
    work = torch.zeros(L.call("sd_quantile_select_ws_bytes", n) // 4, dtype=torch.int32, device=dev)
    sel_t, sel_p = torch.zeros((n, 8), device=dev), torch.zeros((n, 8), device=dev)
    out = torch.full((n, H, 4 * W, 3), 99, dtype=torch.uint8, device=dev)
    s = L.stream_handle(dev)
    L.call("sd_quantile_select_n", n, t.data_ptr(), H * W, Q[0], Q[1], work.data_ptr(), sel_t.data_ptr(), s)
    L.call("sd_quantile_select_n", n, p.data_ptr(), H * W, Q[0], Q[1], work.data_ptr(), sel_p.data_ptr(), s)
    L.call("sd_preview_compose_n", n, x.data_ptr(), t.data_ptr(), p.data_ptr(), H, W, sel_t.data_ptr(), sel_p.data_ptr(),
           out.data_ptr(), s)
    torch.cuda.synchronize()
    assert not work.any()
    return out.cpu().numpy(), sel_t.cpu().numpy(), sel_p.cpu().numpy()


def _restated(inp, tgt, pred, sel_t, sel_p):
    return preview_ref.montage(inp, tgt, pred, (sel_t[5], sel_t[6]), (sel_p[5], sel_p[6]))


def _extra_samples():
    """Samples beyond the fixture: special values in the colour planes, an all-NaN map, a one-value map, W % 4 != 0."""
    rng = np.random.default_rng(31)
    out = []
    for h, w in ((6, 9), (8, 12)):
        inp = rng.uniform(-0.2, 1.2, (6, h, w)).astype(np.float32)
        inp.reshape(-1)[:6] = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, 255.5 / 255.0], dtype=np.float32)
        tgt = np.full((h, w), np.nan, dtype=np.float32)
        pred = _holes(rng, (h, w), 0.2)
        out.append((inp, tgt, pred))
        one = tgt.copy()
        one[1, 2] = 4.0
        out.append((inp, one, np.full((h, w), -1.25, dtype=np.float32)))
    return out


def test_montage_matches_restatement_and_golden(L, gold):
    samples = [(gold[f"{n}/input"], gold[f"{n}/target"], gold[f"{n}/pred"], gold[f"{n}/montage"]) for n in gold["names"]]
    samples += [(*s, None) for s in _extra_samples()]
    for inp, tgt, pred, ref in samples:
        W = inp.shape[2]
        got, sel_t, sel_p = _device_montage(L, inp[None], tgt[None], pred[None])
        _check_sel(sel_t[0], tgt)
        _check_sel(sel_p[0], pred)
        assert np.array_equal(got[0], _restated(inp, tgt, pred, sel_t[0], sel_p[0]))
        if ref is not None:
            assert np.array_equal(got[0][:, : 2 * W], ref[:, : 2 * W])
            diff = np.abs(got[0][:, 2 * W:].astype(np.int16) - ref[:, 2 * W:].astype(np.int16))
            assert diff.max() <= 1, int(diff.max())


def test_montage_batch_of_three_equals_single_calls(L, gold):
    names = ["a", "b", "c"]  # the three 24x40 samples
    inp, tgt, pred = (np.stack([gold[f"{n}/{k}"] for n in names]) for k in ("input", "target", "pred"))
    got, sel_t, sel_p = _device_montage(L, inp, tgt, pred)
    for i in range(3):
        one, st, sp = _device_montage(L, inp[i:i + 1], tgt[i:i + 1], pred[i:i + 1])
        assert np.array_equal(got[i], one[0])
        assert np.array_equal(sel_t[i, :7].view(np.uint32), st[0, :7].view(np.uint32))
        assert np.array_equal(sel_p[i, :7].view(np.uint32), sp[0, :7].view(np.uint32))
    # an odd width (no 16-B path) in a batch
    inp, tgt, pred = (np.stack([gold[f"e/{k}"], gold[f"e/{k}"][..., ::-1, :]]) for k in ("input", "target", "pred"))
    got, sel_t, sel_p = _device_montage(L, inp, tgt, pred)
    for i in range(2):
        assert np.array_equal(got[i], _restated(inp[i], tgt[i], pred[i], sel_t[i], sel_p[i]))


def test_montages_module_function(L, gold):
    from stereo_depth_estimation_amd import preview

    names = ["a", "b", "c"]
    inp, tgt, pred = (np.stack([gold[f"{n}/{k}"] for n in names]) for k in ("input", "target", "pred"))
    want, _, _ = _device_montage(L, inp, tgt, pred)
    x, t, p = (torch.as_tensor(a).to(DEV) for a in (inp, tgt[:, None], pred[:, None]))
    got = preview.montages(x, t, p)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 24, 160, 3) and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), want)
    out = torch.zeros_like(got)
    assert preview.montages(x, t, p, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="out must be"):
        preview.montages(x, t, p, out=out[:2])
    # more than 64 samples go in chunks; the buffers are kept, not reallocated
    rng = np.random.default_rng(3)
    B = 67
    xb = torch.as_tensor(rng.uniform(0, 1, (B, 6, 5, 7)).astype(np.float32)).to(DEV)
    tb = torch.as_tensor(rng.uniform(0, 90, (B, 1, 5, 7)).astype(np.float32)).to(DEV)
    pb = torch.as_tensor(rng.normal(0, 9, (B, 1, 5, 7)).astype(np.float32)).to(DEV)
    big = preview.montages(xb, tb, pb)
    kept = dict(preview._buffers)
    again = preview.montages(xb, tb, pb)
    assert torch.equal(big, again) and all(preview._buffers[k] is v for k, v in kept.items())
    for i in (0, 63, 64, 66):
        assert torch.equal(big[i], preview.montages(xb[i:i + 1], tb[i:i + 1], pb[i:i + 1])[0]), i
    torch.cuda.synchronize()
    assert not any(bufs[0].any() for bufs in preview._buffers.values())


def test_graph_capture_replays_eager_bytes(L, gold):
    from stereo_depth_estimation_amd import preview

    names = ["a", "b", "c"]
    inp, tgt, pred = (np.stack([gold[f"{n}/{k}"] for n in names]) for k in ("input", "target", "pred"))
    x, t, p = (torch.as_tensor(a).to(DEV) for a in (inp, tgt, pred))
    eager = preview.montages(x, t, p).clone()  # also allocates the kept buffers ahead of the capture
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preview.montages(x, t, p, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # new maps in the captured buffers: the replay gives their eager bytes
    t.copy_(p.flip(0).nan_to_num(0.0, 0.0, 0.0))
    p.copy_(torch.as_tensor(pred[::-1].copy()).to(DEV) * 2 - 1)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert not torch.equal(replayed, eager)
    assert torch.equal(replayed, preview.montages(x, t, p))


def test_validation_errors_without_launch(L):
    dev = torch.device(DEV)
    v = torch.zeros(64, device=dev)
    work = torch.zeros(L.call("sd_quantile_select_ws_bytes", 1) // 4, dtype=torch.int32, device=dev)
    sel = torch.full((1, 8), 3.0, device=dev)
    s = L.stream_handle(dev)
    assert L.call("sd_quantile_select_ws_bytes", 0) == -1 and L.call("sd_quantile_select_ws_bytes", 65) == -1
    assert L.call("sd_quantile_select_ws_bytes", 64) == 64 * L.call("sd_quantile_select_ws_bytes", 1)
    for m in (0, 65):
        with pytest.raises(L.StereoHipError, match=r"1\.\.64"):
            L.call("sd_quantile_select_n", m, v.data_ptr(), 64, 0.05, 0.95, work.data_ptr(), sel.data_ptr(), s)
    with pytest.raises(L.StereoHipError, match="q_lo <= q_hi"):
        L.call("sd_quantile_select_n", 1, v.data_ptr(), 64, 0.95, 0.05, work.data_ptr(), sel.data_ptr(), s)
    for q in ((-0.1, 0.5), (0.5, 1.5), (float("nan"), 0.5)):
        with pytest.raises(L.StereoHipError, match="quantiles"):
            L.call("sd_quantile_select_n", 1, v.data_ptr(), 64, q[0], q[1], work.data_ptr(), sel.data_ptr(), s)
    with pytest.raises(L.StereoHipError, match="count"):
        L.call("sd_quantile_select_n", 1, v.data_ptr(), 0, 0.05, 0.95, work.data_ptr(), sel.data_ptr(), s)
    for args in ((None, work.data_ptr(), sel.data_ptr()), (v.data_ptr(), None, sel.data_ptr()),
                 (v.data_ptr(), work.data_ptr(), None)):
        with pytest.raises(L.StereoHipError, match="null pointer"):
            L.call("sd_quantile_select_n", 1, args[0], 64, 0.05, 0.95, args[1], args[2], s)
    x = torch.zeros(6 * 64, device=dev)
    out = torch.full((8 * 32 * 3,), 5, dtype=torch.uint8, device=dev)
    good = [x.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 8, sel.data_ptr(), sel.data_ptr(), out.data_ptr()]
    for n in (0, 65):
        with pytest.raises(L.StereoHipError, match=r"1\.\.64"):
            L.call("sd_preview_compose_n", n, *good, s)
    for k in (0, 1, 2, 5, 6, 7):
        bad = list(good)
        bad[k] = None
        with pytest.raises(L.StereoHipError, match="null pointer"):
            L.call("sd_preview_compose_n", 1, *bad, s)
    for hw in ((0, 8), (8, -1)):
        bad = list(good)
        bad[3], bad[4] = hw
        with pytest.raises(L.StereoHipError, match="bad sizes"):
            L.call("sd_preview_compose_n", 1, *bad, s)
    torch.cuda.synchronize()
    assert bool((sel == 3.0).all()) and bool((out == 5).all()) and not work.any()  # nothing ran


# ---------------------------------------------------------------------------------------------------- end to end
def _rng_equal(a, b) -> bool:
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_rng_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_rng_equal(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def _read_png(path, hw):
    from stereo_depth_estimation_amd.dataset import read_png_batch

    out = torch.empty((1, *hw, 3), dtype=torch.uint8)
    assert read_png_batch([path], hw, out, threads=1)
    return out[0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_log_epoch_previews_end_to_end(tmp_path, precision):
    from stereo_depth_estimation_amd import cli, preview
    from stereo_depth_estimation_amd.dataset import DeviceLoader, FoundationStereoDataset, discover_samples
    from stereo_depth_estimation_amd.model import StereoUNet

    dev = torch.device(DEV)
    write_stereo_tree(tmp_path / "data", scenes=1, frames=3, hw=(40, 52), seed=4)
    ds = FoundationStereoDataset(discover_samples(tmp_path / "data"), image_size=(32, 48))
    loader = DeviceLoader(ds, 2, shuffle=False, num_workers=0, device=dev, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(11)
    model = StereoUNet(in_channels=6, out_channels=1, precision=precision).to(dev)
    model.train()
    buffers = {k: v.detach().clone() for k, v in model.state_dict().items()}
    before = cli.rng_state()
    written = preview.log_epoch_previews(model, loader, dev, 3, tmp_path / "previews")
    after = cli.rng_state()
    assert written == 3 and model.training
    assert _rng_equal(before, after)
    for k, v in model.state_dict().items():
        assert torch.equal(v, buffers[k]), k
    files = sorted(p.name for p in (tmp_path / "previews" / "epoch_0003").iterdir())
    assert files == ["sample_000_00.png", "sample_000_01.png", "sample_001_00.png"]
    assert [p.name for p in (tmp_path / "previews").iterdir()] == ["epoch_0003"]
    model.eval()
    with torch.inference_mode():
        for bi, batch in enumerate(loader):
            pred = model(batch["input"])
            want = preview.montages(batch["input"], batch["target"], pred).cpu()
            # and the device path agrees with the restatement on real network outputs
            sel = [preview_ref.quantile_select(m) for m in (batch["target"][0].cpu().numpy(), pred[0].cpu().numpy())]
            ref = preview_ref.montage(batch["input"][0].cpu().numpy(), batch["target"][0].cpu().numpy(),
                                      pred[0].cpu().numpy())
            assert sel[0]["n"] == 32 * 48 and np.abs(want[0].numpy().astype(np.int16) - ref.astype(np.int16)).max() <= 1
            for ii in range(want.shape[0]):
                png = _read_png(preview.preview_path(tmp_path / "previews", 3, bi, ii), (32, 192))
                assert torch.equal(png, want[ii]), (bi, ii)
    # an eval-mode model stays in eval mode
    assert preview.log_epoch_previews(model, loader, dev, 4, tmp_path / "previews") == 3 and not model.training


class _FakeMlflow(types.ModuleType):
    """The calls cli.main makes, recorded."""

    def __init__(self):
        super().__init__("mlflow")
        self.artifacts, self.metrics, self._run = [], [], None

    def set_tracking_uri(self, uri):
        pass

    def set_experiment(self, name):
        pass

    def start_run(self, run_name=None):
        self._run = types.SimpleNamespace(info=types.SimpleNamespace(run_id=run_name))
        return self._run

    def active_run(self):
        return self._run

    def log_metrics(self, metrics, step=None):
        self.metrics.append(step)

    def log_artifacts(self, local_dir, artifact_path=None):
        self.artifacts.append((local_dir, artifact_path))

    def set_tag(self, key, value):
        pass

    def end_run(self):
        self._run = None


def test_cli_writes_previews_and_leaves_training_untouched(tmp_path, monkeypatch, capsys):
    from stereo_depth_estimation_amd import cli

    write_stereo_tree(tmp_path / "data", scenes=2, frames=4, hw=(40, 52), seed=9)

    def run(name, extra):
        fake = _FakeMlflow()
        monkeypatch.setitem(sys.modules, "mlflow", fake)
        cli.main(["--dataset-root", str(tmp_path / "data"), "--height", "32", "--width", "48", "--epochs", "2",
                  "--batch-size", "2", "--num-workers", "0", "--val-fraction", "0.25", "--output-dir",
                  str(tmp_path / "out"), "--run-name", name, "--augment", "--brightness-jitter", "0.2",
                  "--noise-std-max", "0.02", *extra])
        return fake, tmp_path / "out" / name

    fake, with_dir = run("with", [])
    assert "MLflow previews: logging 2 fixed val samples each epoch." in capsys.readouterr().out
    for epoch in (1, 2):
        files = sorted((with_dir / "mlflow_previews" / f"epoch_{epoch:04d}").iterdir())
        assert [f.name for f in files] == ["sample_000_00.png", "sample_000_01.png"]  # min(8, |val| = 2)
        for f in files:
            img = _read_png(f, (32, 192))
            assert tuple(img.shape) == (32, 192, 3) and img.float().std() > 1
    assert sorted(p.name for p in (with_dir / "mlflow_previews").iterdir()) == ["epoch_0001", "epoch_0002"]
    assert fake.artifacts == [(str(with_dir / "mlflow_previews" / f"epoch_{e:04d}"), f"previews/epoch_{e:04d}")
                              for e in (1, 2)]

    fake0, without_dir = run("without", ["--preview-samples", "0"])
    assert "MLflow previews" not in capsys.readouterr().out
    assert not (without_dir / "mlflow_previews").exists() and fake0.artifacts == []
    a = torch.load(with_dir / "checkpoints" / "last.pt", map_location="cpu", weights_only=True)
    b = torch.load(without_dir / "checkpoints" / "last.pt", map_location="cpu", weights_only=True)
    assert a["epoch"] == b["epoch"] == 2 and a["args"]["preview_samples"] == 8 and b["args"]["preview_samples"] == 0
    for k, v in a["model_state_dict"].items():
        assert torch.equal(v, b["model_state_dict"][k]), k
    assert a["optimizer_state_dict"]["state"].keys() == b["optimizer_state_dict"]["state"].keys()
    for pid, st in a["optimizer_state_dict"]["state"].items():
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["optimizer_state_dict"]["state"][pid][k])), (pid, k)
    assert _rng_equal(a["rng_state"], b["rng_state"])
    assert a["metrics"]["train_mae"] == b["metrics"]["train_mae"] and a["metrics"]["val_mae"] == b["metrics"]["val_mae"]
