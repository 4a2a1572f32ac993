"""The predict tool on the device: sd_disp_export (csrc/predict.hip) and stereo_depth_estimation_amd/predict.py.

"Reference chain" below: sd_resize_bilinear on the same maps (the entry point the kernel must equal bit for bit),
then tests/predict_ref.py (NumPy) on its output.

* disp_rgb, disp_up and the counts of the metric rows are bit-equal to the reference chain in the per-pixel and the
  four-pixel store path, at odd sizes, the identity, a source smaller than the model and through misaligned buffers,
  with the memory around every output untouched; the two fp64 sums are within n * 2^-53 relative of NumPy's (the terms
  are non-negative and exact in fp64, so any summation order stays inside that); two runs give the same 64 bits;
* special samples and values: an all-zero ground truth gives a row of zeros; NaN, +inf and negative disparities give
  code 0, values above the range the largest code; non-finite pixels are left out of the metrics;
* sigma codes equal the reference (np.exp in float32) wherever the reference's value * 1000 lies farther from a
  half-integer than 8 float32 ulps (twice the 4-ulp bound INTEGRATION.md states for the device exp), else within 1;
* bad arguments are rejected before any launch;
* predict_dataset / predict_pairs / the CLI end to end on a small tree: file layout, the files' bytes, the metadata.
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch
from PIL import Image

import predict_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CANARY = 0xA5
PAD = 64  # canary bytes on either side of an output


def L():
    from stereo_depth_estimation_amd import _lib

    _lib.load()
    return _lib


def resize(lib, maps: np.ndarray, out_hw, mul) -> np.ndarray:
    """sd_resize_bilinear on [B,H,W] float32 -> [B,Hs,Ws]."""
    B, H, W = maps.shape
    src = torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float32)).to(DEV)
    out = torch.empty(B, *out_hw, device=DEV)
    lib.call("sd_resize_bilinear", src.data_ptr(), B, H, W, out.data_ptr(), out_hw[0], out_hw[1], float(mul),
             lib.stream_handle())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def export(lib, disp, logvar, gt_rgb, out_hw, off=0, want=("rgb", "sigma", "up", "rows")):
    """sd_disp_export with every buffer placed `off` elements of its type (bytes for the images and the ground truth,
    floats for the maps, doubles for the rows and the workspace) into a canaried allocation (torch allocations are
    256-B aligned, so `off` sets the alignment); asserts the canaries on both sides of each output."""
    B, H, W = disp.shape
    Hs, Ws = out_hw
    px = B * Hs * Ws

    def dev_in(a, item):
        if a is None:
            return None, 0
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = torch.zeros(off * item + raw.size, dtype=torch.uint8, device=DEV)
        buf[off * item:] = torch.from_numpy(raw).to(DEV)
        return buf, buf.data_ptr() + off * item

    keep_d, p_disp = dev_in(disp.astype(np.float32), 4)
    keep_l, p_lv = dev_in(None if logvar is None else logvar.astype(np.float32), 4)
    keep_g, p_gt = dev_in(gt_rgb, 1)
    sizes = {"rgb": (px * 3, 1), "sigma": (px * 3, 1), "up": (px * 4, 4), "rows": (B * 64, 8)}
    outs = {k: torch.full((PAD + off * sizes[k][1] + sizes[k][0] + PAD,), CANARY, dtype=torch.uint8, device=DEV)
            for k in want}
    ptr = {k: o.data_ptr() + PAD + off * sizes[k][1] for k, o in outs.items()}
    ws = lib.call("sd_disp_export_ws_bytes", B, Hs, Ws)
    assert ws > 0 and ws % 8 == 0
    work = torch.full((PAD + off * 8 + ws + PAD,), CANARY, dtype=torch.uint8, device=DEV)
    lib.call("sd_disp_export", p_disp, p_lv or None, B, H, W, p_gt or None, Hs, Ws, ptr.get("rgb"), ptr.get("sigma"),
             ptr.get("up"), ptr.get("rows"), work.data_ptr() + PAD + off * 8, lib.stream_handle())
    torch.cuda.synchronize()
    wh = work.cpu().numpy()
    assert (wh[:PAD + off * 8] == CANARY).all() and (wh[PAD + off * 8 + ws:] == CANARY).all(), "wrote outside work"
    res = {}
    for k, o in outs.items():
        n, item = sizes[k]
        lead = PAD + off * item
        h = o.cpu().numpy()
        assert (h[:lead] == CANARY).all() and (h[lead + n:] == CANARY).all(), f"wrote outside {k}"
        res[k] = h[lead:lead + n].copy()
    shaped = {"rgb": lambda a: a.reshape(B, Hs, Ws, 3), "sigma": lambda a: a.reshape(B, Hs, Ws, 3),
              "up": lambda a: a.view(np.float32).reshape(B, Hs, Ws), "rows": lambda a: a.view(np.float64).reshape(B, 8)}
    return {k: shaped[k](v) for k, v in res.items()}


def make_case(lib, B, hw, out_hw, seed):
    """Seeded maps; disparities 0...200 px after the upsample's width scaling; ground truth = the upsampled
    prediction plus N(0, 2.5 px) noise through the encoder (so the 1 / 2 / 3 px and the 5 % thresholds split the
    pixels), 10 % of it zero (no value)."""
    rng = np.random.default_rng(seed)
    mul = R.width_scale(out_hw[1], hw[1])
    disp = (rng.uniform(0, 200, (B, *hw)) / float(mul)).astype(np.float32)
    logvar = rng.uniform(-4, 1, (B, *hw)).astype(np.float32)
    d_up = resize(lib, disp, out_hw, mul)
    gt = (d_up + rng.normal(0, 2.5, d_up.shape)).astype(np.float32)
    gt[rng.random(gt.shape) < 0.1] = 0
    return disp, logvar, R.encode(gt), d_up, mul


def assert_rows(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    for k in (0, 3, 4, 5, 6, 7):
        assert np.array_equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    for k in (1, 2):
        tol = want[:, 0] * 2.0 ** -53 * want[:, k]
        assert (np.abs(got[:, k] - want[:, k]) <= tol).all(), (k, got[:, k], want[:, k])


CASES = {
    "per_pixel_odd": ((16, 16), (17, 23), 0),
    "per_pixel": ((32, 48), (45, 61), 0),
    "identity": ((24, 32), (24, 32), 0),
    "downscale_vector": ((48, 64), (20, 32), 0),
    "vector": ((32, 48), (45, 64), 0),
    "vector_shape_misaligned": ((32, 48), (45, 64), 1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_reference_chain(name):
    lib = L()
    hw, out_hw, off = CASES[name]
    B = 3
    disp, logvar, gt_rgb, d_up, mul = make_case(lib, B, hw, out_hw, seed=out_hw[1] + hw[0])
    if name == "identity":
        assert float(mul) == 1.0 and np.array_equal(d_up, disp)
    want_rows = R.metric_rows(d_up, gt_rgb)
    n = want_rows[:, 0]
    assert (n > 0.8 * out_hw[0] * out_hw[1]).all()
    for k in (3, 4, 5, 6):  # every threshold splits the counted pixels
        assert ((want_rows[:, k] > 0.02 * n) & (want_rows[:, k] < 0.98 * n)).all(), (k, want_rows)
    assert (want_rows[:, 6] < want_rows[:, 5]).all()  # D1's relative clause excludes some of the > 3 px errors
    got = export(lib, disp, logvar, gt_rgb, out_hw, off=off)
    assert np.array_equal(got["up"].view(np.uint32), d_up.view(np.uint32))
    assert np.array_equal(got["rgb"], R.encode(d_up))
    assert_rows(got["rows"], want_rows)
    again = export(lib, disp, logvar, gt_rgb, out_hw, off=off)
    assert np.array_equal(again["rows"].view(np.uint64), got["rows"].view(np.uint64))  # one fixed summation order
    if off:  # the same bytes as the four-pixel path on this shape, rows included
        vec = export(lib, disp, logvar, gt_rgb, out_hw, off=0)
        for k in ("rgb", "sigma", "up"):
            assert np.array_equal(vec[k], got[k]), k
        assert np.array_equal(vec["rows"].view(np.uint64), got["rows"].view(np.uint64))
    # each output alone gives the same bytes
    assert np.array_equal(export(lib, disp, None, None, out_hw, off=off, want=("rgb",))["rgb"], got["rgb"])
    only_rows = export(lib, disp, None, gt_rgb, out_hw, off=off, want=("rows",))["rows"]
    assert np.array_equal(only_rows.view(np.uint64), got["rows"].view(np.uint64))


def test_more_partial_rows_than_one_block_sums():
    """(240, 320) -> (270, 480): 127 blocks per sample, so the second launch adds many partial rows."""
    lib = L()
    hw, out_hw = (240, 320), (270, 480)
    disp, logvar, gt_rgb, d_up, _ = make_case(lib, 2, hw, out_hw, seed=5)
    assert lib.call("sd_disp_export_ws_bytes", 2, *out_hw) == 2 * 127 * 64
    got = export(lib, disp, None, gt_rgb, out_hw, want=("rgb", "rows"))
    assert np.array_equal(got["rgb"], R.encode(d_up))
    assert_rows(got["rows"], R.metric_rows(d_up, gt_rgb))


def test_special_samples_and_values():
    lib = L()
    hw = out_hw = (16, 24)
    rng = np.random.default_rng(11)
    disp = rng.uniform(1, 100, (3, *hw)).astype(np.float32)
    disp[0, 3, 5], disp[0, 8, 9], disp[0, 12, 20], disp[0, 5, 15] = np.nan, np.inf, -3.0, 2e4
    disp[2, 1, 1] = -np.inf
    d_up = resize(lib, disp, out_hw, 1.0)
    gt = rng.uniform(1, 100, (3, *hw)).astype(np.float32)
    gt_rgb = R.encode(gt)
    gt_rgb[1] = 0  # a sample without ground truth
    got = export(lib, disp, None, gt_rgb, out_hw, want=("rgb", "up", "rows"))
    assert np.array_equal(got["up"].view(np.uint32), d_up.view(np.uint32))
    code = R.rgb_to_code(got["rgb"])
    nonfinite = ~np.isfinite(d_up)
    assert nonfinite[0, 3, 5] and nonfinite[0, 8, 9] and nonfinite[2, 1, 1] and d_up[0, 12, 20] == -3.0
    assert (code[nonfinite] == 0).all() and code[0, 12, 20] == 0
    assert d_up[0, 5, 15] == 2e4 and code[0, 5, 15] == R.MAX_CODE and got["rgb"][0, 5, 15].tolist() == [255, 255, 255]
    assert np.array_equal(got["rgb"], R.encode(d_up))
    want_rows = R.metric_rows(d_up, gt_rgb)
    assert_rows(got["rows"], want_rows)
    assert not got["rows"][1].any()  # all-zero ground truth: a row of zeros
    assert got["rows"][0, 0] == hw[0] * hw[1] - nonfinite[0].sum() < hw[0] * hw[1]  # non-finite pixels not counted
    assert got["rows"][2, 0] == hw[0] * hw[1] - nonfinite[2].sum()


@pytest.mark.parametrize("name", ["per_pixel", "vector"])
def test_sigma_codes(name):
    lib = L()
    hw, out_hw, _ = CASES[name]
    disp, logvar, _, _, mul = make_case(lib, 3, hw, out_hw, seed=77)
    lv_up = resize(lib, logvar, out_hw, 1.0)
    ref = R.sigma_values(lv_up, mul)
    x = ref.astype(np.float64) * 1000.0
    near = np.abs((x - np.floor(x)) - 0.5) <= 8 * np.spacing(x.astype(np.float32)).astype(np.float64)
    assert near.mean() < 0.02, near.mean()  # from the reference alone: the window is about 0.4 % of a code
    got = R.rgb_to_code(export(lib, disp, logvar, None, out_hw, want=("rgb", "sigma"))["sigma"])
    want = R.disp_code(ref)
    assert want.min() > 100 and want.max() < 3000
    assert np.array_equal(got[~near], want[~near]), int((got[~near] != want[~near]).sum())
    assert (np.abs(got[near] - want[near]) <= 1).all()


def test_rejects_bad_arguments_without_launch():
    lib = L()
    p = 256  # a non-null, aligned address that is never dereferenced
    ok = dict(disp=p, logvar=p, B=1, H=4, W=4, gt=p, Hs=4, Ws=4, rgb=p, sigma=p, up=p, rows=p, work=p)

    def call(**kw):
        a = {**ok, **kw}
        lib.call("sd_disp_export", a["disp"], a["logvar"], a["B"], a["H"], a["W"], a["gt"], a["Hs"], a["Ws"], a["rgb"],
                 a["sigma"], a["up"], a["rows"], a["work"], None)

    for kw, msg in ((dict(disp=None), "null disp"), (dict(gt=None), "metrics need gt_rgb"),
                    (dict(logvar=None), "sigma_rgb needs logvar"), (dict(work=None), "work buffer"),
                    (dict(work=p + 4), "work buffer"), (dict(B=0), "bad batch"), (dict(B=-2), "bad batch"),
                    (dict(H=0), "bad model size"), (dict(W=-1), "bad model size"), (dict(Hs=0), "output size"),
                    (dict(Ws=0), "output size"), (dict(Hs=65536, Ws=65536), "output size"),
                    (dict(rgb=None, sigma=None, up=None, rows=None), "no output")):
        with pytest.raises(lib.StereoHipError, match=msg):
            call(**kw)
    assert lib.call("sd_disp_export_ws_bytes", 0, 4, 4) == -1
    assert lib.call("sd_disp_export_ws_bytes", 1, 0, 4) == -1
    assert lib.call("sd_disp_export_ws_bytes", 1, 65536, 65536) == -1
    assert lib.call("sd_disp_export_ws_bytes", 32, 540, 960) == 32 * 128 * 64


# ---------------------------------------------------------------------------------------------- end to end
MODEL_HW = (32, 48)


def write_tree(root):
    """Scene A: five PNG samples at 45x61. Scene B: two at 40x64. Smooth frames; the ground truth 20...60 px with zeros."""
    rng = np.random.default_rng(2)
    for scene, n, hw in (("sceneA", 5, (45, 61)), ("sceneB", 2, (40, 64))):
        data = root / scene / "dataset" / "data"
        for d in ("left/rgb", "right/rgb", "left/disparity"):
            (data / d).mkdir(parents=True, exist_ok=True)
        for f in range(n):
            left = rng.integers(0, 256, (*hw, 3), dtype=np.uint8)
            right = np.roll(left, 3, axis=1)
            gt = rng.uniform(20, 60, hw).astype(np.float32)
            gt[rng.random(hw) < 0.1] = 0
            Image.fromarray(left).save(data / "left/rgb" / f"{f:06d}.png")
            Image.fromarray(right).save(data / "right/rgb" / f"{f:06d}.png")
            Image.fromarray(R.encode(gt)).save(data / "left/disparity" / f"{f:06d}.png")


def tiny_model(precision):
    from oracle import unet_ref as U
    from stereo_depth_estimation_amd.model import StereoUNet

    st = U.make_state(8, seed=0, signed_gamma=True)
    m = StereoUNet(base_channels=8, precision=precision)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV).eval()


def expected_outputs(lib, model, items, batch_size):
    """Per item (disparity codes, upsampled d, reference sigma values, ground-truth bytes): model(x,
    return_uncertainty=True) on the sd_stereo_preprocess input, in the tool's batches, through the reference chain."""
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
        sig = R.sigma_values(resize(lib, lv[:, 0].cpu().numpy(), hw, 1.0), mul)
        for k, it in enumerate(its):
            out[it.relpath] = (R.encode(d_up[k]), d_up[k], sig[k], frames[2][k])
    return out


def assert_sigma_file(path, ref):
    from stereo_depth_estimation_amd import dataset as D

    got = R.rgb_to_code(D.read_rgb_uint8(path))
    x = ref.astype(np.float64) * 1000.0
    near = np.abs((x - np.floor(x)) - 0.5) <= 8 * np.spacing(x.astype(np.float32)).astype(np.float64)
    want = R.disp_code(ref)
    assert np.array_equal(got[~near], want[~near]) and (np.abs(got[near] - want[near]) <= 1).all(), path


def files_under(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_predict_end_to_end(tmp_path, precision, capsys):
    from stereo_depth_estimation_amd import dataset as D
    from stereo_depth_estimation_amd import predict as P

    lib = L()
    H, W = MODEL_HW
    root = tmp_path / "data"
    write_tree(root)
    model = tiny_model(precision)
    items = P.dataset_items(root)
    assert len(items) == 7
    want = expected_outputs(lib, model, items, 2)
    want_rows = np.stack([R.metric_rows(want[it.relpath][1][None], want[it.relpath][3][None])[0] for it in items])
    agg = P.aggregate_rows(want_rows)
    n_all = want_rows[:, 0].sum()

    def check_metrics(meta):
        assert meta["valid_pixels"] == agg["valid_pixels"] == int(n_all)
        for k in ("bad1", "bad2", "bad3", "d1"):
            assert meta[k] == agg[k], k
        for k in ("epe", "rmse"):
            assert abs(meta[k] - agg[k]) <= (n_all * 2.0 ** -53 + 2.0 ** -52) * agg[k], k

    # dataset mode, with sigma files
    out = tmp_path / "out"
    meta = P.predict_dataset(None, root, out, model=model, height=H, width=W, batch_size=2, write_sigma=True)
    printed = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(printed) == meta == json.loads((out / "predict_meta.json").read_text())
    names = [it.relpath.as_posix() for it in items]
    assert files_under(out) == sorted(names + [P.sigma_relpath(it.relpath).as_posix() for it in items]
                                      + ["metrics.jsonl", "predict_meta.json"])
    for it in items:
        codes, _, sig, _ = want[it.relpath]
        assert D.png_size(out / it.relpath) == codes.shape[:2]
        assert np.array_equal(D.read_rgb_uint8(out / it.relpath), codes), it.relpath
        assert_sigma_file(out / P.sigma_relpath(it.relpath), sig)
    assert (meta["mode"], meta["num_samples"], meta["num_batches"], meta["num_written"]) == ("dataset", 7, 4, 14)
    assert (meta["height"], meta["width"], meta["precision"], meta["base_channels"], meta["batch_size"],
            meta["write_sigma"], meta["png_level"]) == (H, W, precision, 8, 2, True, 1)
    assert meta["dataset_root"] == str(root.resolve()) and meta["output_root"] == str(out.resolve())
    assert meta["elapsed_seconds"] > 0
    check_metrics(meta)
    lines = [json.loads(s) for s in (out / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 7 and [r["sample"] for r in lines] == names
    for r, row in zip(lines, want_rows):
        assert r["valid_pixels"] == int(row[0]) and r["bad3"] == row[5] / row[0] and r["d1"] == row[6] / row[0]
        assert abs(r["epe"] - row[1] / row[0]) <= row[0] * 2.0 ** -52 * r["epe"]
    # the files are labels the loader reads: decoded, they are the upsampled prediction to within half a code
    back = R.decode(D.read_rgb_uint8(out / items[0].relpath))
    assert np.abs(back.astype(np.float64) - want[items[0].relpath][1]).max() <= 0.5e-3 + 1e-5

    # directory-pair mode on scene A's frames: the same disparity bytes, no metrics
    data_a = root / "sceneA" / "dataset" / "data"
    out2 = tmp_path / "out_pairs"
    meta2 = P.predict_pairs(None, data_a / "left" / "rgb", data_a / "right" / "rgb", out2, model=model, height=H,
                            width=W, batch_size=2)
    assert files_under(out2) == sorted([f"{f:06d}.png" for f in range(5)] + ["predict_meta.json"])
    for f in range(5):
        assert (out2 / f"{f:06d}.png").read_bytes() == (out / "sceneA" / f"{f:06d}.png").read_bytes()
    assert meta2["mode"] == "pairs" and meta2["num_samples"] == 5 and meta2["num_written"] == 5
    assert not ({"epe", "rmse", "bad1", "bad2", "bad3", "d1", "valid_pixels"} & set(meta2))

    # evaluate only: the same figures, nothing written anywhere
    before = files_under(tmp_path)
    meta3 = P.predict_dataset(None, root, None, model=model, height=H, width=W, batch_size=2)
    assert files_under(tmp_path) == before
    assert meta3["output_root"] is None and meta3["num_written"] == 0
    check_metrics(meta3)
    assert meta3["epe"] == meta["epe"] and meta3["rmse"] == meta["rmse"]  # one fixed summation order

    # max_samples and a batch size above the sample count
    meta4 = P.predict_dataset(None, root, None, model=model, height=H, width=W, batch_size=32, max_samples=3)
    assert meta4["num_samples"] == 3 and meta4["num_batches"] == 1
    assert meta4["valid_pixels"] == int(want_rows[:3, 0].sum())

    if precision == "fp32":  # the command line, from a checkpoint file: size from its args
        ck = tmp_path / "best.pt"
        torch.save({"epoch": 1, "model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()},
                    "args": {"height": H, "width": W}, "metrics": {}}, ck)
        meta5 = P.main(["--checkpoint", str(ck), "--dataset-root", str(root), "--base-channels", "8", "--batch-size",
                        "2", "--output-root", str(tmp_path / "out_cli"), "--png-level", "6"])
        assert (meta5["height"], meta5["width"], meta5["png_level"], meta5["checkpoint"]) == (H, W, 6, str(ck))
        check_metrics(meta5)
        for it in items:
            assert np.array_equal(D.read_rgb_uint8(tmp_path / "out_cli" / it.relpath), want[it.relpath][0])


def test_fp8_first_batch_calibrates_then_static_scales(golden_dir):
    """precision="fp8" on the reference-trained weights (tests/golden/trained_state.npz, base 32): the first run is the
    calibration forward, later runs use its scales. Held only to a gross-error bound against the fp32 model on the
    same frames (mean |d8 - d32| below 10 % of the mean disparity: e4m3 keeps 3 mantissa bits, 6 % per rounding, and
    the project's own bound for this path on these weights is 1 %, tests/test_gpu_configs.py); the point is that the
    path runs through Predictor and gives the same bytes twice."""
    from stereo_depth_estimation_amd.model import StereoUNet
    from stereo_depth_estimation_amd.predict import Predictor

    st = dict(np.load(golden_dir / "trained_state.npz"))
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:60, 0:80]
    base = (127 + 100 * np.sin(xx[None, ..., None] / 9.0 + yy[None, ..., None] / 7.0 + rng.uniform(0, 6, (3, 1, 1, 3))))
    left = np.clip(base + rng.integers(-10, 10, base.shape), 0, 255).astype(np.uint8)
    right = np.roll(left, -4, axis=2)
    l_d, r_d = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    codes = {}
    for precision in ("fp32", "fp8"):
        m = StereoUNet(base_channels=32, precision=precision)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
        p = Predictor(m.to(DEV), (64, 48))
        runs = []
        for _ in range(3):  # fp8: calibration, static scales, static scales
            out = p.run(l_d, r_d, sigma=True)
            torch.cuda.synchronize()
            runs.append(R.rgb_to_code(out["disp_rgb"].cpu().numpy()))
            assert out["rows"] is None and out["sigma_rgb"].shape == (3, 60, 80, 3)
        assert p._calibrated and np.array_equal(runs[1], runs[2])
        codes[precision] = runs[2].astype(np.float64)
    assert codes["fp32"].mean() > 100  # a disparity map, not zeros
    assert np.abs(codes["fp8"] - codes["fp32"]).mean() <= 0.10 * codes["fp32"].mean()
