"""Uncertainty evaluation on the device: sd_uncert_eval (csrc/uncert.hip), uncert.py, and the flag in predict / adapt.

"Reference chain" below: sd_resize_bilinear on both maps (the values the kernel must see bit for bit), then
tests/uncert_ref.py (NumPy, Python integers, float64) on its output.

* bit-equal to the reference chain: n, sum q, the two saturation counts, both curves, AUSE and AURG (integer
  histograms and a stated fp64 order leave nothing to round differently), at odd sizes, the identity, a downscale,
  through misaligned buffers and for 1, 7, 20 and 256 cuts, with the memory around rows and work untouched;
* each coverage count lies in [lo, hi] of the reference, which leaves undecided the pixels within 8 float32 ulps of the
  threshold z * exp(lv) (twice the 4-ulp bound INTEGRATION.md states for the device exp, the allowance
  test_gpu_predict.py gives sigma); hi - lo <= n / 1000 is asserted on the reference, so the allowance cannot hide a
  failure;
* sum nll: see ``nll_bound``;
* a sample larger than one sweep of the grid and many blocks per sample, twice: the same 64 bits;
* a sample's row does not depend on its neighbours in the batch; special samples; a poisoned work buffer; bad arguments;
* predict_dataset(eval_uncertainty=True) and adapt(eval_uncertainty=True) end to end on a small tree.
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import predict_ref as R
import uncert_ref as U
from test_gpu_predict import CANARY, DEV, PAD, L, resize, tiny_model

pytestmark = pytest.mark.gpu


def evaluate(lib, disp, logvar, gt_rgb, out_hw, steps=20, off=0, poison=True):
    """sd_uncert_eval with every buffer placed `off` elements of its type into a canaried allocation (bytes for the
    ground truth, floats for the maps, doubles for rows and work); work itself is filled with the canary byte (the entry
    point must not need it cleared); asserts the canaries on both sides of rows and work. Returns rows [B, 16 + 2 steps]."""
    B, H, W = disp.shape
    Hs, Ws = out_hw

    def dev_in(a, item):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = torch.zeros(off * item + raw.size, dtype=torch.uint8, device=DEV)
        buf[off * item:] = torch.from_numpy(raw).to(DEV)
        return buf, buf.data_ptr() + off * item

    keep_d, p_disp = dev_in(disp.astype(np.float32), 4)
    keep_l, p_lv = dev_in(logvar.astype(np.float32), 4)
    keep_g, p_gt = dev_in(gt_rgb, 1)
    ws = lib.call("sd_uncert_eval_ws_bytes", B, Hs, Ws, steps)
    assert ws > 0 and ws % 8 == 0
    nrow = B * (U.HEAD + 2 * steps) * 8
    lead = PAD + off * 8
    rows = torch.full((lead + nrow + PAD,), CANARY, dtype=torch.uint8, device=DEV)
    work = torch.full((lead + ws + PAD,), CANARY if poison else 0, dtype=torch.uint8, device=DEV)
    lib.call("sd_uncert_eval", p_disp, p_lv, B, H, W, p_gt, Hs, Ws, steps, rows.data_ptr() + lead,
             work.data_ptr() + lead, lib.stream_handle())
    torch.cuda.synchronize()
    if poison:
        wh = work.cpu().numpy()
        assert (wh[:lead] == CANARY).all() and (wh[lead + ws:] == CANARY).all(), "wrote outside work"
    rh = rows.cpu().numpy()
    assert (rh[:lead] == CANARY).all() and (rh[lead + nrow:] == CANARY).all(), "wrote outside rows"
    return rh[lead:lead + nrow].copy().view(np.float64).reshape(B, U.HEAD + 2 * steps)


def make_case(lib, B, hw, out_hw, seed, ranked=True):
    """test_gpu_predict.make_case's maps; the ground truth is the upsampled prediction plus Laplace noise of scale
    exp(lv_up) * mul (``ranked``: the head is calibrated, the curves fall) or of one scale everywhere, independent of
    lv (they do not); 10 % of it zero. Returns disp, logvar, gt_rgb, d_up, lv_up, mul."""
    rng = np.random.default_rng(seed)
    mul = R.width_scale(out_hw[1], hw[1])
    disp = (rng.uniform(0, 200, (B, *hw)) / float(mul)).astype(np.float32)
    logvar = rng.uniform(-4, 1, (B, *hw)).astype(np.float32)
    d_up = resize(lib, disp, out_hw, mul)
    lv_up = resize(lib, logvar, out_hw, 1.0)
    scale = np.exp(lv_up.astype(np.float64)) * float(mul) if ranked else 0.3 * float(mul)
    gt = (d_up + rng.laplace(0.0, 1.0, d_up.shape) * scale).astype(np.float32)
    gt[rng.random(gt.shape) < 0.1] = 0
    return disp, logvar, R.encode(gt), d_up, lv_up, mul


def nll_bound(ref: dict) -> float:
    """|got - want| allowed for row [2], the fp64 sum of the float32 nll_px = e_m * expf(-lv) + lv, want = NumPy's fp64
    sum of the reference's float32 terms. Per pixel: the device expf is within 4 ulp of the true value and np.exp within
    1, so the two exps differ by at most 5 * 2^-23 relative (bounded with 8, the allowance used for sigma, plus the
    reference's own), which the product t = e_m * exp(-lv) inherits: 8 * 2^-23 t; the product's own rounding on either
    side adds 2^-24 t each: together under 10 * 2^-23 t. The float32 sum t + lv rounds once on either side, and the two
    roundings differ by at most one ulp of the result: 2^-23 |nll|. Over the sample these add; the fp64 accumulation in
    any order adds n * 2^-53 * sum |nll| (assert_rows' order term)."""
    t, nll = ref["t"], ref["nll"]
    return float((10 * 2.0 ** -23 * t + 2.0 ** -23 * np.abs(nll)).sum() + nll.size * 2.0 ** -53 * np.abs(nll).sum())


EXACT = (0, 1, 7, 8, 9, 10)  # n, sum q, AUSE, AURG, the saturation counts


def assert_rows(got, refs, steps):
    assert got.shape == (len(refs), U.HEAD + 2 * steps) and got.dtype == np.float64
    for b, ref in enumerate(refs):
        want = ref["row"]
        for k in EXACT:
            assert got[b, k] == want[k], (b, k, got[b, k], want[k])
        assert not got[b, 11:U.HEAD].any()
        assert np.array_equal(got[b, U.HEAD:].view(np.uint64), want[U.HEAD:].view(np.uint64)), (b, "curves")
        n = want[0]
        for i in range(4):
            lo, hi = ref["cov_lo"][i], ref["cov_hi"][i]
            assert hi - lo <= n / 1000, (b, i, lo, hi, n)  # on the reference: the allowance is narrow
            assert lo <= got[b, 3 + i] <= hi, (b, i, lo, got[b, 3 + i], hi)
        print(f"sample {b}: nll got {got[b, 2]!r} want {want[2]!r} bound {nll_bound(ref):.3e}")
        assert abs(got[b, 2] - want[2]) <= nll_bound(ref), (b, got[b, 2], want[2], nll_bound(ref))


CASES = {
    "odd": ((16, 16), (17, 23), 0),
    "odd_larger": ((32, 48), (45, 61), 0),
    "identity": ((24, 32), (24, 32), 0),
    "downscale": ((48, 64), (20, 32), 0),
    "upscale": ((32, 48), (45, 64), 0),
    "upscale_misaligned": ((32, 48), (45, 64), 1),
}


@pytest.mark.parametrize("ranked", [True, False], ids=["ranked", "unranked"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_reference_chain(name, ranked):
    lib = L()
    hw, out_hw, off = CASES[name]
    steps = 20
    disp, logvar, gt_rgb, d_up, lv_up, mul = make_case(lib, 3, hw, out_hw, seed=out_hw[1] + hw[0], ranked=ranked)
    refs = U.sample_rows(d_up, lv_up, gt_rgb, mul, steps)
    for ref in refs:
        row = ref["row"]
        unc, orc = row[U.HEAD:U.HEAD + steps], row[U.HEAD + steps:]
        assert row[0] > 0.8 * out_hw[0] * out_hw[1] and (np.diff(orc) < 0).all()
        if ranked:  # the head ranks the errors: the curve falls, most of the way to the oracle's
            assert unc[-1] < 0.5 * unc[0] and row[8] > 0.2 and 0 < row[7] < row[8]
            for i, p in enumerate(U.NOMINAL):  # and has the right size: the Laplace shares, to four binomial sigmas
                assert abs(row[3 + i] / row[0] - p) < 4 * np.sqrt(p * (1 - p) / row[0]) + 0.01, (i, row[3 + i] / row[0], p)
        else:  # it does not: flat
            assert abs(row[8]) < 0.1 and row[7] > 0.3
    got = evaluate(lib, disp, logvar, gt_rgb, out_hw, steps, off=off)
    assert_rows(got, refs, steps)
    again = evaluate(lib, disp, logvar, gt_rgb, out_hw, steps, off=off)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))  # one fixed summation order


@pytest.mark.parametrize("steps", [1, 7, 256])
def test_other_step_counts(steps):
    lib = L()
    hw, out_hw, _ = CASES["odd_larger"]
    disp, logvar, gt_rgb, d_up, lv_up, mul = make_case(lib, 3, hw, out_hw, seed=steps)
    assert_rows(evaluate(lib, disp, logvar, gt_rgb, out_hw, steps), U.sample_rows(d_up, lv_up, gt_rgb, mul, steps), steps)


def test_many_blocks_and_sweeps_give_the_same_bits_twice():
    """(64, 96) -> (270, 480), B = 2: the grid is ceil(Hs * Ws / 8192) blocks per sample, 64 at most and 1024 / B at
    most, so 129600 pixels take 16 blocks of 1024 threads (every cut of the four small cases fits one): each block
    flushes its LDS histograms into the sample's global ones, 16 partial rows are added, and a thread walks 7 or 8
    pixels of the grid-stride loop."""
    lib = L()
    hw, out_hw = (64, 96), (270, 480)
    disp, logvar, gt_rgb, d_up, lv_up, mul = make_case(lib, 2, hw, out_hw, seed=5)
    nblk = -(-out_hw[0] * out_hw[1] // 8192)
    assert nblk == 16
    assert lib.call("sd_uncert_eval_ws_bytes", 2, *out_hw, 20) == 2 * 2 * 4096 * 12 + 2 * nblk * 64
    got = evaluate(lib, disp, logvar, gt_rgb, out_hw)
    assert_rows(got, U.sample_rows(d_up, lv_up, gt_rgb, mul, 20), 20)
    again = evaluate(lib, disp, logvar, gt_rgb, out_hw)
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


def test_a_row_does_not_depend_on_the_batch():
    lib = L()
    hw, out_hw, _ = CASES["odd_larger"]
    disp, logvar, gt_rgb, *_ = make_case(lib, 3, hw, out_hw, seed=21)
    batch = evaluate(lib, disp, logvar, gt_rgb, out_hw)
    alone = evaluate(lib, disp[1:2], logvar[1:2], gt_rgb[1:2], out_hw)
    assert np.array_equal(alone[0].view(np.uint64), batch[1].view(np.uint64))


def test_special_samples():
    lib = L()
    hw = out_hw = (16, 24)
    steps = 20
    rng = np.random.default_rng(11)
    B = 6
    disp = rng.uniform(1, 100, (B, *hw)).astype(np.float32)
    logvar = rng.uniform(-4, 1, (B, *hw)).astype(np.float32)
    gt = (disp + rng.laplace(0, 1, disp.shape) * np.exp(logvar)).astype(np.float32)
    gt = np.maximum(gt, 0.01).astype(np.float32)
    gt_rgb = R.encode(gt)
    gt_rgb[0] = 0  # no ground truth
    disp[1, 3, 5], disp[1, 8, 9], disp[1, 2, 2] = np.nan, np.inf, -np.inf  # left out
    logvar[1, 4, 4], logvar[1, 9, 1], logvar[1, 7, 7] = np.nan, np.inf, -np.inf
    gt_rgb[2] = 0
    gt_rgb[2, 5, 7] = R.encode(np.array([33.25], dtype=np.float32))[0]  # one counted pixel
    logvar[3] = -0.75  # constant
    logvar[4, :8], logvar[4, 8:] = -40.0, 40.0  # saturates both ends
    got = evaluate(lib, disp, logvar, gt_rgb, out_hw, steps)
    # the identity resize returns finite input as it is, but a non-finite value also takes the neighbours it has weight
    # 0 in (0 * inf): the reference chain sees what the kernel sees
    d_up, lv_up = resize(lib, disp, out_hw, 1.0), resize(lib, logvar, out_hw, 1.0)
    assert np.array_equal(d_up[0], disp[0]) and np.array_equal(lv_up[3:], logvar[3:])
    refs = U.sample_rows(d_up, lv_up, gt_rgb, 1.0, steps)
    assert_rows(got, refs, steps)
    px = hw[0] * hw[1]
    assert not got[0].any()
    left_out = (~np.isfinite(d_up[1]) | ~np.isfinite(lv_up[1])).sum()
    assert 6 <= left_out < 40 and got[1, 0] == px - left_out
    assert got[2, 0] == 1 and (got[2, U.HEAD:] == got[2, U.HEAD]).all() and got[2, 7] == 0 and got[2, 8] == 0
    unc = got[3, U.HEAD:U.HEAD + steps]
    assert got[3, 0] == px and (np.abs(unc - unc[0]) <= 2 * np.spacing(unc[0])).all() and abs(got[3, 8]) <= 1e-15
    assert got[4, 0] == px and got[4, 9] == px and got[5, 9] == 0


def test_work_needs_no_clearing():
    """Two consecutive calls with different inputs, the work buffer filled with 0xA5 before each (``evaluate`` does):
    both right; and the same rows from a zeroed work buffer."""
    lib = L()
    hw, out_hw, _ = CASES["upscale"]
    for seed in (1, 2):
        disp, logvar, gt_rgb, d_up, lv_up, mul = make_case(lib, 3, hw, out_hw, seed=seed)
        got = evaluate(lib, disp, logvar, gt_rgb, out_hw, poison=True)
        assert_rows(got, U.sample_rows(d_up, lv_up, gt_rgb, mul, 20), 20)
        clean = evaluate(lib, disp, logvar, gt_rgb, out_hw, poison=False)
        assert np.array_equal(clean.view(np.uint64), got.view(np.uint64))


def test_rejects_bad_arguments_without_launch():
    lib = L()
    p = 256  # a non-null, aligned address that is never dereferenced
    ok = dict(disp=p, logvar=p, B=1, H=4, W=4, gt=p, Hs=4, Ws=4, steps=20, rows=p, work=p)

    def call(**kw):
        a = {**ok, **kw}
        lib.call("sd_uncert_eval", a["disp"], a["logvar"], a["B"], a["H"], a["W"], a["gt"], a["Hs"], a["Ws"], a["steps"],
                 a["rows"], a["work"], None)

    for kw, msg in ((dict(disp=None), "null disp"), (dict(logvar=None), "null disp or logvar"),
                    (dict(gt=None), "null gt_rgb"), (dict(steps=0), "steps"), (dict(steps=257), "steps"),
                    (dict(rows=None), "rows"), (dict(rows=p + 4), "rows"), (dict(work=None), "work buffer"),
                    (dict(work=p + 4), "work buffer"), (dict(B=0), "bad batch"), (dict(B=65536), "bad batch"),
                    (dict(H=0), "bad model size"), (dict(W=-1), "bad model size"), (dict(Hs=0), "output size"),
                    (dict(Ws=0), "output size"), (dict(Hs=65536, Ws=65536), "output size")):
        with pytest.raises(lib.StereoHipError, match=msg):
            call(**kw)
    for args in ((0, 4, 4, 20), (65536, 4, 4, 20), (1, 0, 4, 20), (1, 65536, 65536, 20), (1, 4, 4, 0), (1, 4, 4, 257)):
        assert lib.call("sd_uncert_eval_ws_bytes", *args) == -1, args
    # 32 samples of 540 x 960: 64 blocks of pixels, 1024 / 32 = 32 blocks per sample
    assert lib.call("sd_uncert_eval_ws_bytes", 32, 540, 960, 20) == 32 * 2 * 4096 * 12 + 32 * 32 * 64


def test_uncertainty_eval_class():
    from stereo_depth_estimation_amd.uncert import UncertaintyEval

    lib = L()
    hw, out_hw, _ = CASES["odd_larger"]
    disp, logvar, gt_rgb, d_up, lv_up, mul = make_case(lib, 3, hw, out_hw, seed=8)
    ev = UncertaintyEval(steps=7)
    t = [torch.from_numpy(a).to(DEV) for a in (disp[:, None], logvar[:, None], gt_rgb)]
    rows = ev.run(*t, out_hw)
    assert rows.shape == (3, U.HEAD + 14) and rows.dtype == torch.float64 and rows.device.type == "cuda"
    torch.cuda.synchronize()
    assert_rows(rows.cpu().numpy(), U.sample_rows(d_up, lv_up, gt_rgb, mul, 7), 7)
    assert ev.run(*t).data_ptr() == rows.data_ptr()  # the buffers are kept per (n, Hs, Ws)
    with pytest.raises(ValueError):
        ev.run(t[0], t[1], t[2][:2])
    with pytest.raises(ValueError):
        UncertaintyEval(steps=0)


# ---------------------------------------------------------------------------------------------- end to end
MODEL_HW = (32, 48)


def write_tree(root):
    """Four PNG samples at 45 x 61 in one scene; smooth-free frames, the ground truth 5...40 px with zeros."""
    from PIL import Image

    rng = np.random.default_rng(2)
    hw = (45, 61)
    data = root / "sceneA" / "dataset" / "data"
    for d in ("left/rgb", "right/rgb", "left/disparity"):
        (data / d).mkdir(parents=True, exist_ok=True)
    for f in range(4):
        left = rng.integers(0, 256, (*hw, 3), dtype=np.uint8)
        gt = rng.uniform(5, 40, hw).astype(np.float32)
        gt[rng.random(hw) < 0.1] = 0
        Image.fromarray(left).save(data / "left/rgb" / f"{f:06d}.png")
        Image.fromarray(np.roll(left, 3, axis=1)).save(data / "right/rgb" / f"{f:06d}.png")
        Image.fromarray(R.encode(gt)).save(data / "left/disparity" / f"{f:06d}.png")


def reference_rows(lib, model, items, batch_size, steps):
    """The reference chain's rows per item, in order: the model on the sd_stereo_preprocess input in the tool's batches,
    sd_resize_bilinear on both heads, uncert_ref."""
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
        lib.call("sd_stereo_preprocess", l_d.data_ptr(), r_d.data_ptr(), g_d.data_ptr(), n, hw[0], hw[1], H, W,
                 inp.data_ptr(), tgt.data_ptr(), val.data_ptr(), lib.stream_handle())
        with torch.inference_mode():
            d, lv = model(inp, return_uncertainty=True)
        torch.cuda.synchronize()
        mul = R.width_scale(hw[1], W)
        d_up = resize(lib, d[:, 0].cpu().numpy(), hw, mul)
        lv_up = resize(lib, lv[:, 0].cpu().numpy(), hw, 1.0)
        for it, ref in zip(its, U.sample_rows(d_up, lv_up, frames[2], mul, steps)):
            out[it.relpath] = ref
    return [out[it.relpath] for it in items]


def close_summary(got: dict, want: dict, ref: dict):
    """A per-sample ``uncertainty`` object against summary_from_row of the reference's row: everything equal but the
    NLL (within nll_bound / n) and the coverage shares (inside [lo, hi] / n)."""
    n = ref["row"][0]
    assert set(got) == set(want)
    for k in set(got) - {"nll", "coverage"}:
        assert got[k] == want[k], k
    assert abs(got["nll"] - want["nll"]) <= nll_bound(ref) / n + 2.0 ** -52 * abs(want["nll"])
    for i, z in enumerate(("0.5", "1.0", "2.0", "3.0")):
        assert ref["cov_lo"][i] / n <= got["coverage"][z] <= ref["cov_hi"][i] / n, z


def test_predict_end_to_end(tmp_path):
    from stereo_depth_estimation_amd import predict as P
    from stereo_depth_estimation_amd import uncert as M

    lib = L()
    H, W = MODEL_HW
    steps = 7
    root = tmp_path / "data"
    write_tree(root)
    model = tiny_model("fp32")
    items = P.dataset_items(root)
    assert len(items) == 4
    refs = reference_rows(lib, model, items, 3, steps)
    assert all(r["row"][0] > 2000 for r in refs)

    plain = P.predict_dataset(None, root, tmp_path / "plain", model=model, height=H, width=W, batch_size=3)
    meta = P.predict_dataset(None, root, tmp_path / "out", model=model, height=H, width=W, batch_size=3,
                             eval_uncertainty=True, sparsification_steps=steps)
    # without the flag: the keys and files of before; with it: three more keys, the same files with the same bytes
    assert not {"uncertainty", "eval_uncertainty", "sparsification_steps"} & set(plain)
    assert set(meta) - set(plain) == {"uncertainty", "eval_uncertainty", "sparsification_steps"}
    assert meta["eval_uncertainty"] is True and meta["sparsification_steps"] == steps
    assert json.loads((tmp_path / "out" / "predict_meta.json").read_text()) == meta
    names = sorted(str(p.relative_to(tmp_path / "out")) for p in (tmp_path / "out").rglob("*") if p.is_file())
    assert names == sorted(str(p.relative_to(tmp_path / "plain")) for p in (tmp_path / "plain").rglob("*") if p.is_file())
    for it in items:
        assert (tmp_path / "out" / it.relpath).read_bytes() == (tmp_path / "plain" / it.relpath).read_bytes()
    for k in ("epe", "rmse", "bad1", "bad2", "bad3", "d1", "valid_pixels"):
        assert meta[k] == plain[k], k
    lines = [json.loads(s) for s in (tmp_path / "out" / "metrics.jsonl").read_text().splitlines()]
    plain_lines = [json.loads(s) for s in (tmp_path / "plain" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 4
    for rec, old, ref in zip(lines, plain_lines, refs):
        assert "uncertainty" not in old and {k: v for k, v in rec.items() if k != "uncertainty"} == old
        close_summary(rec["uncertainty"], M.summary_from_row(ref["row"], steps), ref)
    want = M.aggregate_rows(np.stack([r["row"] for r in refs]), steps)
    got = meta["uncertainty"]
    assert set(got) == set(want)
    for k in set(got) - {"nll", "coverage"}:
        assert got[k] == want[k], k
    n_all = sum(r["row"][0] for r in refs)
    assert abs(got["nll"] - want["nll"]) <= sum(nll_bound(r) for r in refs) / n_all + 2.0 ** -50 * abs(want["nll"])
    for i, z in enumerate(("0.5", "1.0", "2.0", "3.0")):
        assert sum(r["cov_lo"][i] for r in refs) / n_all <= got["coverage"][z] <= sum(r["cov_hi"][i] for r in refs) / n_all
    with pytest.raises(ValueError, match="--sparsification-steps"):
        P.predict_dataset(None, root, None, model=model, height=H, width=W, eval_uncertainty=True,
                          sparsification_steps=300)


def test_adapt_end_to_end(tmp_path):
    from stereo_depth_estimation_amd import adapt as A
    from stereo_depth_estimation_amd.model import StereoUNet

    def fresh_model():
        torch.manual_seed(6)
        return StereoUNet(base_channels=8, precision="fp32").to(DEV).train()

    root = tmp_path / "data"
    write_tree(root)
    common = dict(dataset_root=str(root), height=32, width=64, epochs=1, batch_size=2, lr=1e-3)  # 4 samples: 2 steps
    meta = A.adapt(None, model=fresh_model(), output_dir=str(tmp_path / "on"), eval_uncertainty=True, **common)
    assert meta["eval_uncertainty"] is True and meta["num_batches"] == 2
    for k in ("uncertainty_before", "uncertainty_after"):
        u = meta[k]
        assert u["samples"] == 4 and u["steps"] == 20 and len(u["sparsification"]) == 20
        assert np.isfinite(u["nll"]) and np.isfinite(u["ause"]) and u["sparsification"][0] == 1.0
        assert all(0.0 <= u["coverage"][z] <= 1.0 for z in ("0.5", "1.0", "2.0", "3.0"))
    assert meta["uncertainty_before"]["valid_pixels"] == meta["uncertainty_after"]["valid_pixels"]
    assert json.loads((tmp_path / "on" / "adapt_meta.json").read_text()) == meta
    off = A.adapt(None, model=fresh_model(), output_dir=str(tmp_path / "off"), **common)
    assert set(meta) - set(off) == {"eval_uncertainty", "uncertainty_before", "uncertainty_after"}
    assert off["epe_before"] == meta["epe_before"]
