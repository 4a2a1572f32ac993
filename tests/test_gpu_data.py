"""On-device data path (csrc/data.hip via stereo_depth_estimation_amd/dataset.py).

* sd_stereo_preprocess against items the REFERENCE's FoundationStereoDataset produced from PNG
  files (tests/golden/data_path.npz, gen_golden.py) and against the numpy restatement
  (oracle/data_ref.py) at a realistic downscale. Tolerance: 2e-6 absolute on the [0,1] RGB
  channels and 1e-6 relative on disparity (fp32 re-association of the bilinear sum only; the
  decode is exact), the valid mask exact.
* sd_stereo_from_cache against load_cached_sample (dataset.py:86-105): exact, through the 4-pixel
  kernel (aligned buffers, plane a multiple of 4) and the per-pixel one (5x7, 1x1, 3x6, 37x53 planes;
  24x32 with each pointer misaligned in turn), with the float16 specials (+-0, +-smallest
  subnormal, 65504, +-inf, NaN: valid exactly where > 0) and bytes 0 and 255 in every channel; no
  byte outside the outputs is written.
* sd_augment_rgb against the torchvision-0.25 restatement (oracle/aug_ref.py; parity unpinned by
  the reference) with the noise off: 2e-5 absolute against the fp32 restatement at one
  size, and against the FLOAT64 restatement over tests/data_kernels_ref.py's cases (sizes 5x7,
  37x53, 40x52, 96x96, 132x128, 132x252 so that each kernel's grid-stride loop runs again; blur
  3, 5, 9, 31 with ks/2 = H - 1 once; planted primaries, greys, two-channel ties, near-whites; the
  factors at the ends of their ranges, different for the two images of a pair). Tolerance of a case:
  8 x the fp32 CPU restatement's largest deviation from float64 on the case's inputs, floored at
  4 * 2^-24; that deviation is below 1e-5 for every case (tests/test_data_kernels_ref_cpu.py).
  Measured on an MI355X (every case prints its figures; run with -s):

    factor set   fp32-CPU deviation (smallest .. largest)   largest device deviation / allowed
    ends_a       4.8e-07 .. 9.1e-07                          0.13
    ends_b       2.3e-07 .. 9.6e-07                          0.18
    mid          4.8e-07 .. 9.4e-07                          0.14

  With noise on: the added field has mean 0 and the requested std (statistical; at 37x53 mean
  9.6e-05, std 0.0504 for 0.05), every plane its own field, and at odd H*W the last value of a plane
  and the first of the next are different draws (they shared one before the pair counter became
  plane * ceil(HW/2) + px/2). One image of a batch and its factors changed: the others keep their
  bytes.
* DeviceLoader end to end on a PNG tree, including the cache round trip (write on miss in the
  reference's format, read back as cached samples).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import data_kernels_ref as K
from conftest import write_stereo_tree
from oracle import aug_ref, data_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def L():
    from stereo_depth_estimation_amd import _lib

    _lib.load()
    return _lib


def _prep(lib, left, right, drgb, out_hw):
    B, Hs, Ws, _ = left.shape
    Ho, Wo = out_hw
    l_d, r_d, d_d = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (left, right, drgb))
    inp = torch.empty(B, 6, Ho, Wo, device=DEV)
    tgt = torch.empty(B, 1, Ho, Wo, device=DEV)
    val = torch.empty(B, 1, Ho, Wo, device=DEV, dtype=torch.bool)
    lib.call("sd_stereo_preprocess", l_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), B, Hs, Ws, Ho, Wo, inp.data_ptr(),
             tgt.data_ptr(), val.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    return inp.cpu().numpy(), tgt.cpu().numpy(), val.cpu().numpy()


def test_preprocess_matches_reference_dataset_items(golden_dir):
    lib = L()
    g = np.load(golden_dir / "data_path.npz")
    left = np.stack([g[f"src{i}_left"] for i in range(4)])
    right = np.stack([g[f"src{i}_right"] for i in range(4)])
    drgb = np.stack([g[f"src{i}_disp_rgb"] for i in range(4)])
    inp, tgt, val = _prep(lib, left, right, drgb, (24, 32))
    for i in range(4):
        assert np.abs(inp[i] - g[f"item{i}_input"]).max() <= 2e-6
        rt = g[f"item{i}_target"]
        assert np.abs(tgt[i] - rt).max() <= 1e-6 * (1 + np.abs(rt).max())
        assert np.array_equal(val[i], g[f"item{i}_valid"])


@pytest.mark.parametrize("src_hw,out_hw", [((480, 640), (240, 320)), ((375, 1242), (240, 320)), ((17, 23), (40, 50))])
def test_preprocess_matches_restatement(src_hw, out_hw):
    lib = L()
    rng = np.random.default_rng(7)
    B = 2
    left = rng.integers(0, 256, (B, *src_hw, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (B, *src_hw, 3), dtype=np.uint8)
    disp = rng.uniform(0, 200, (B, *src_hw)).astype(np.float32)
    disp[rng.random((B, *src_hw)) < 0.1] = 0
    drgb = data_ref.encode_disparity_to_rgb(disp)
    inp, tgt, val = _prep(lib, left, right, drgb, out_hw)
    for b in range(B):
        ref_in = np.concatenate([data_ref.load_rgb_from_uint8(left[b], out_hw),
                                 data_ref.load_rgb_from_uint8(right[b], out_hw)])
        ref_t = data_ref.load_disparity_from_rgb24(drgb[b], out_hw)
        assert np.abs(inp[b] - ref_in).max() <= 2e-6
        assert np.abs(tgt[b] - ref_t).max() <= 1e-6 * (1 + np.abs(ref_t).max())
        assert np.array_equal(val[b], ref_t > 0)


def test_from_cache_matches_load_cached_sample():
    lib = L()
    rng = np.random.default_rng(3)
    B, H, W = 3, 24, 32
    left = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    disp = rng.uniform(-1, 50, (B, H, W)).astype(np.float16)
    l_d, r_d = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    d_d = torch.from_numpy(disp).to(DEV).view(torch.int16)
    inp = torch.empty(B, 6, H, W, device=DEV)
    tgt = torch.empty(B, 1, H, W, device=DEV)
    val = torch.empty(B, 1, H, W, device=DEV, dtype=torch.bool)
    lib.call("sd_stereo_from_cache", l_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), B, H, W, inp.data_ptr(),
             tgt.data_ptr(), val.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    for b in range(B):
        ref_l = torch.from_numpy(left[b].astype(np.float32) / 255.0).permute(2, 0, 1)
        ref_r = torch.from_numpy(right[b].astype(np.float32) / 255.0).permute(2, 0, 1)
        ref_t = torch.from_numpy(disp[b].astype(np.float32)).unsqueeze(0)
        assert torch.equal(inp[b].cpu(), torch.cat([ref_l, ref_r]))
        assert torch.equal(tgt[b].cpu(), ref_t)
        assert torch.equal(val[b].cpu(), ref_t > 0)


def _augment(lib, x, params, ks, seed=1):
    B, _, H, W = x.shape
    xd = x.clone().to(DEV)
    pd = torch.tensor(params, dtype=torch.float32).reshape(2 * B, 7).to(DEV)
    work = torch.empty(B * 6 * H * W + 128 * B, device=DEV)
    lib.call("sd_augment_rgb", xd.data_ptr(), B, H, W, pd.data_ptr(), ks, seed, work.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    return xd.cpu()


def test_augment_matches_torchvision_restatement():
    lib = L()
    torch.manual_seed(0)
    B, H, W, ks = 3, 37, 53, 5
    x = torch.rand(B, 6, H, W)
    x[0, :, :4, :4] = 0.5  # grey patch: hue of equal channels
    params = []
    for im in range(2 * B):
        sigma = [0.0, 0.7, 1.9][im % 3]
        params.append([0.7 + 0.1 * im, 1.3 - 0.1 * im, 0.6 + 0.15 * im, [-0.08, 0.0, 0.05][im % 3], 0.8 + 0.07 * im,
                       sigma, 0.0])
    got = _augment(lib, x, params, ks)
    for im in range(2 * B):
        b, side = im // 2, im % 2
        img = x[b, side * 3:side * 3 + 3]
        p = params[im]
        ref = aug_ref.augment_rgb(img.clone(), p[0], p[1], p[2], p[3], p[4], p[5], ks)
        assert float((got[b, side * 3:side * 3 + 3] - ref).abs().max()) <= 2e-5, f"image {im}"


def test_augment_noise_statistics_and_clamp():
    lib = L()
    B, H, W = 2, 128, 160
    x = torch.full((B, 6, H, W), 0.5)
    std = 0.05
    params = [[1.0, 1.0, 1.0, 0.0, 1.0, 0.0, std]] * (2 * B)
    got = _augment(lib, x, params, 5, seed=11)
    d = (got - 0.5).flatten()
    assert abs(float(d.mean())) < 1e-3
    assert abs(float(d.std()) - std) < 1e-3
    again = _augment(lib, x, params, 5, seed=11)
    assert torch.equal(got, again)  # deterministic for a seed
    big = _augment(lib, x, [[1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 2.0]] * (2 * B), 5, seed=5)
    assert float(big.min()) >= 0.0 and float(big.max()) <= 1.0


@pytest.mark.parametrize("hw,ks,fs", K.aug_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_augment_matches_float64_restatement(hw, ks, fs):
    """Three pairs per case against oracle.aug_ref in float64; the tolerance is 8 x the fp32 CPU restatement's own
    deviation from float64 on the case's inputs (data_kernels_ref.aug_case), floored at 4 * 2^-24."""
    x, params, ref, dev32, tol = K.aug_case(hw, ks, fs)
    got = _augment(L(), x, params, ks)
    K.aug_check(f"augment[{hw[0]}x{hw[1]},ks={ks},{fs}]", got, ref, tol, dev32)


def test_augment_images_are_independent():
    """One image of a batch of three pairs and its factors change: the other five images keep their bytes (blur and
    noise on)."""
    lib = L()
    H, W, ks = 37, 53, 5
    x = K.make_aug_batch(H, W, seed=8)
    params = [row[:6] + [0.02] for row in K.aug_params("mid")]
    base = _augment(lib, x, params, ks, seed=3)
    for im in (0, 3):
        b, side = im // 2, im % 2
        x2, p2 = x.clone(), [list(r) for r in params]
        x2[b, 3 * side:3 * side + 3] = 1.0 - x2[b, 3 * side:3 * side + 3]
        p2[im] = [1.3, 0.6, 1.4, 0.4, 1.7, 1.1, 0.04]
        got = _augment(lib, x2, p2, ks, seed=3)
        for other in range(6):
            ob, os_ = other // 2, other % 2
            same = torch.equal(got[ob, 3 * os_:3 * os_ + 3], base[ob, 3 * os_:3 * os_ + 3])
            assert same == (other != im), (im, other)


def test_augment_noise_differs_across_plane_boundaries_at_odd_size():
    """5 x 7 (HW = 35, odd), flat 0.5, no blur, std 0.05: the last value of plane p and the first of plane p + 1 are
    different draws at each of the 11 boundaries (a chance equality has probability below 1e-5 per boundary; the seed
    is fixed). With the counter (plane*HW + px) >> 1 the last pixel of every even plane shared its draw with the
    first pixel of the next plane, across images at planes 2|3, 8|9 and across pairs at 5|6."""
    lib = L()
    B, H, W = 2, 5, 7
    x = torch.full((B, 6, H, W), 0.5)
    got = _augment(lib, x, [[1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.05]] * (2 * B), 3, seed=11).view(6 * B, H * W)
    assert float((got - 0.5).abs().min()) > 0  # the noise is on everywhere
    same = [p for p in range(6 * B - 1) if float(got[p, -1]) == float(got[p + 1, 0])]
    assert not same, f"planes sharing a draw with their successor: {same}"


def test_augment_noise_statistics_at_odd_size():
    """The statistical check of test_augment_noise_statistics_and_clamp at 37 x 53 (odd HW; 47k values: the mean of
    N(0, 0.05) over them has sigma 2.3e-4, the std 1.6e-4, so 1e-3 is above 4 sigma)."""
    lib = L()
    B, H, W = 4, 37, 53
    x = torch.full((B, 6, H, W), 0.5)
    std = 0.05
    params = [[1.0, 1.0, 1.0, 0.0, 1.0, 0.0, std]] * (2 * B)
    got = _augment(lib, x, params, 5, seed=11)
    d = (got - 0.5).flatten()
    print(f"noise 37x53: mean {float(d.mean()):.3g} std {float(d.std()):.4g}")
    assert abs(float(d.mean())) < 1e-3
    assert abs(float(d.std()) - std) < 1e-3
    assert torch.equal(got, _augment(lib, x, params, 5, seed=11))  # deterministic for a seed
    assert not torch.equal(got, _augment(lib, x, params, 5, seed=12))
    planes = (got - 0.5).view(6 * B, H * W)
    assert len({planes[p].numpy().tobytes() for p in range(6 * B)}) == 6 * B  # every plane its own field


# ------------------------------------------------------------------ sd_stereo_from_cache, both kernels
def _from_cache(lib, left, right, disp_bits, off=None):
    """Run sd_stereo_from_cache with every buffer `off[name]` bytes past a 256-byte-aligned allocation; returns
    (input, target as int32 bits, valid) as numpy arrays after checking that nothing outside the outputs was written."""
    off = {**{k: 0 for k in ("left", "right", "disp", "input", "target", "valid")}, **(off or {})}
    B, H, W, _ = left.shape
    n = B * H * W
    pad = 64

    def src(a, o):
        raw = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy())
        buf = torch.zeros(raw.numel() + pad, dtype=torch.uint8, device=DEV)
        buf[o:o + raw.numel()].copy_(raw)
        return buf, buf[o:].data_ptr()

    def dst(nbytes, o):
        buf = torch.full((nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[o:].data_ptr()

    lb, lp = src(left, off["left"])
    rb, rp = src(right, off["right"])
    db, dp = src(disp_bits, off["disp"])
    ib, ip = dst(n * 6 * 4, off["input"])
    tb, tp = dst(n * 4, off["target"])
    vb, vp = dst(n, off["valid"])
    for name, p, al in (("left", lp, 4), ("right", rp, 4), ("disp", dp, 8), ("input", ip, 16), ("target", tp, 16),
                        ("valid", vp, 4)):
        assert p % al == off[name] % al, name
    lib.call("sd_stereo_from_cache", lp, rp, dp, B, H, W, ip, tp, vp, lib.stream_handle())
    torch.cuda.synchronize()
    outs = []
    for buf, o, nbytes in ((ib, off["input"], n * 6 * 4), (tb, off["target"], n * 4), (vb, off["valid"], n)):
        h = buf.cpu().numpy()
        assert (h[:o] == 0xA5).all() and (h[o + nbytes:] == 0xA5).all()  # nothing written outside the output
        outs.append(h[o:o + nbytes].copy())
    return (outs[0].view(np.float32).reshape(B, 6, H, W), outs[1].view(np.int32).reshape(B, 1, H, W),
            outs[2].reshape(B, 1, H, W))


def _check_cache_decode(got, left, right, disp_bits):
    inp, tbits, valid = got
    ref_in, ref_t, ref_v = K.cache_decode_ref(left, right, disp_bits)
    assert np.array_equal(inp.view(np.int32), ref_in.view(np.int32))
    nan = np.isnan(ref_t)
    assert np.array_equal(np.isnan(tbits.view(np.float32)), nan)  # NaN by class ...
    assert np.array_equal(tbits[~nan], ref_t.view(np.int32)[~nan])  # ... everything else by bits (-0 keeps its sign)
    assert np.array_equal(valid, ref_v.astype(np.uint8))  # 0 / 1 bytes; NaN and -0 invalid


@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (8, 1, 1), (2, 3, 6), (2, 37, 53)])
def test_from_cache_per_pixel_kernel_at_planes_no_multiple_of_four(B, H, W):
    assert (H * W) % 4 != 0  # sd_stereo_from_cache takes k_stereo_from_cache, one pixel per thread
    left, right, disp = K.make_cache_batch(B, H, W, seed=H * W)
    _check_cache_decode(_from_cache(L(), left, right, disp), left, right, disp)


CACHE_OFFSETS = [{}, {"left": 1}, {"right": 1}, {"disp": 2}, {"valid": 1}, {"input": 4}, {"target": 4},
                 {"left": 1, "right": 1, "disp": 2, "valid": 1, "input": 4, "target": 4}]


def test_from_cache_misaligned_pointers_take_the_per_pixel_kernel_with_equal_bytes():
    """24 x 32 (the plane is a multiple of 4): aligned buffers take the 4-pixel kernel, any misaligned pointer the
    per-pixel one; both decode exactly, so both paths give equal bytes on the same data."""
    lib = L()
    B, H, W = 3, 24, 32
    left, right, disp = K.make_cache_batch(B, H, W, seed=5)
    base = _from_cache(lib, left, right, disp)
    _check_cache_decode(base, left, right, disp)
    for off in CACHE_OFFSETS[1:]:
        got = _from_cache(lib, left, right, disp, off)
        _check_cache_decode(got, left, right, disp)
        nan = np.isnan(base[1].view(np.float32))
        assert np.array_equal(got[0].view(np.int32), base[0].view(np.int32)) and np.array_equal(got[2], base[2]), off
        assert np.array_equal(got[1][~nan], base[1][~nan]), off


def test_from_cache_float16_specials():
    """+0, -0, +-smallest subnormal, 65504, +-inf and NaN through both kernels: valid exactly where the value is > 0."""
    lib = L()
    for (B, H, W), off in (((2, 24, 32), {}), ((2, 24, 32), {"disp": 2}), ((2, 3, 6), {})):
        left, right, disp = K.make_cache_batch(B, H, W, seed=9)
        inp, tbits, valid = _from_cache(lib, left, right, disp, off)
        n = len(K.F16_PLANTED)
        assert np.array_equal(disp.reshape(B, -1)[:, :n], np.broadcast_to(K.F16_PLANTED, (B, n)))
        assert np.array_equal(valid.reshape(B, -1)[:, :n].astype(bool), np.broadcast_to(K.F16_VALID, (B, n)))
        t = tbits.view(np.float32).reshape(B, -1)[:, :n]
        want = K.F16_PLANTED.view(np.float16).astype(np.float32)
        assert np.isnan(t[:, 7]).all()
        assert np.array_equal(t[:, :7].view(np.int32), np.broadcast_to(want[:7].view(np.int32), (B, 7)))


def test_device_loader_end_to_end_with_cache(tmp_path):
    from stereo_depth_estimation_amd import dataset as D

    ref = write_stereo_tree(tmp_path / "data", scenes=2, frames=3, hw=(45, 61), seed=2)
    samples = D.discover_samples(tmp_path / "data")
    ds = D.FoundationStereoDataset(samples, image_size=(24, 32), cache_root=tmp_path / "cache")
    loader = D.DeviceLoader(ds, batch_size=4, shuffle=False, num_workers=0, device=DEV)
    batches = list(loader)
    assert [b["input"].shape[0] for b in batches] == [4, 2]
    torch.cuda.synchronize()
    keys = sorted(ref)
    allin = torch.cat([b["input"] for b in batches]).cpu().numpy()
    allt = torch.cat([b["target"] for b in batches]).cpu().numpy()
    allv = torch.cat([b["valid_mask"] for b in batches]).cpu().numpy()
    for i, k in enumerate(keys):
        left, right, drgb = ref[k]
        ref_in = np.concatenate([data_ref.load_rgb_from_uint8(left, (24, 32)), data_ref.load_rgb_from_uint8(right, (24, 32))])
        ref_t = data_ref.load_disparity_from_rgb24(drgb, (24, 32))
        assert np.abs(allin[i] - ref_in).max() <= 2e-6
        assert np.abs(allt[i] - ref_t).max() <= 1e-6 * (1 + np.abs(ref_t).max())
        assert np.array_equal(allv[i], ref_t > 0)
    # the first pass wrote the reference's cache files; a second pass reads them (uint8 RGB, f16 disparity)
    files = sorted((tmp_path / "cache").rglob("*.npz"))
    assert len(files) == 6
    with np.load(files[0]) as c:
        assert c["left"].dtype == np.uint8 and c["left"].shape == (24, 32, 3) and c["disparity"].dtype == np.float16
    ds2 = D.FoundationStereoDataset(samples, image_size=(24, 32), cache_root=tmp_path / "cache", require_cache=True)
    b2 = torch.cat([b["input"] for b in D.DeviceLoader(ds2, batch_size=6, device=DEV)]).cpu().numpy()
    assert np.abs(b2 - np.round(allin * 255).clip(0, 255) / 255).max() <= 1 / 255 + 1e-6


def test_run_epoch_on_device_loader(tmp_path):
    from stereo_depth_estimation_amd import dataset as D
    from stereo_depth_estimation_amd.model import StereoUNet
    from stereo_depth_estimation_amd.optim import FusedAdamW
    from stereo_depth_estimation_amd.train import run_epoch

    write_stereo_tree(tmp_path, scenes=1, frames=4, hw=(40, 52), seed=4)
    ds = D.FoundationStereoDataset(D.discover_samples(tmp_path), image_size=(32, 48), augment=True,
                                   brightness_jitter=0.2, hue_jitter=0.05, blur_prob=0.5, blur_sigma_max=1.0,
                                   noise_std_max=0.02)
    torch.manual_seed(0)
    model = StereoUNet(in_channels=6, out_channels=1, base_channels=8).to(DEV)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    metrics, step = run_epoch(model, D.DeviceLoader(ds, batch_size=2, shuffle=True, device=DEV), DEV, optimizer=opt)
    assert step == 2 and set(metrics) == {"loss", "nll", "mae", "rmse", "sigma"}
    assert all(np.isfinite(v) for v in metrics.values())


def test_device_loader_native_reader_matches_dataloader_path(tmp_path):
    """DeviceLoader(native=True) (in-process C++ cache reader, two pinned buffer sets) yields the same batches, in
    the same shuffled order, as the DataLoader worker path over the same cache; it is the default for a
    require_cache dataset without augmentation."""
    from stereo_depth_estimation_amd import dataset as D

    write_stereo_tree(tmp_path / "data", scenes=2, frames=5, hw=(45, 61), seed=7)
    samples = D.discover_samples(tmp_path / "data")
    ds = D.FoundationStereoDataset(samples, image_size=(24, 32), cache_root=tmp_path / "cache")
    for _ in D.DeviceLoader(ds, batch_size=4, device=DEV):  # first pass writes the cache
        pass
    torch.cuda.synchronize()
    dsc = D.FoundationStereoDataset(samples, image_size=(24, 32), cache_root=tmp_path / "cache", require_cache=True)
    assert D.DeviceLoader(dsc, batch_size=3, device=DEV).native
    runs = {}
    for native in (True, False):
        ld = D.DeviceLoader(dsc, batch_size=3, shuffle=True, device=DEV, generator=torch.Generator().manual_seed(5),
                            native=native, num_workers=0 if native else 2)
        assert ld.native is native
        runs[native] = [{k: v.cpu() for k, v in b.items()} for b in ld]
    assert [b["input"].shape[0] for b in runs[True]] == [3, 3, 3, 1]
    for a, b in zip(runs[True], runs[False]):
        for k in ("input", "target", "valid_mask"):
            assert torch.equal(a[k], b[k]), k
    # with augmentation: the factors and noise seeds come from the global RNG in a num_workers=0 DataLoader's order
    dsa = D.FoundationStereoDataset(samples, image_size=(24, 32), cache_root=tmp_path / "cache", require_cache=True,
                                    augment=True, brightness_jitter=0.2, hue_jitter=0.05, blur_prob=0.5,
                                    blur_sigma_max=1.0, noise_std_max=0.02)
    runs = {}
    for native in (True, False):
        torch.manual_seed(11)
        ld = D.DeviceLoader(dsa, batch_size=4, shuffle=True, device=DEV, native=native, num_workers=0)
        runs[native] = [{k: v.cpu() for k, v in b.items()} for _ in range(2) for b in ld]  # two epochs
    assert len(runs[True]) == len(runs[False]) == 6
    for a, b in zip(runs[True], runs[False]):
        for k in ("input", "target", "valid_mask"):
            assert torch.equal(a[k], b[k]), ("aug", k)


def test_device_loader_native_png_matches_dataloader_path(tmp_path):
    """DeviceLoader(native=True) on an un-cached PNG dataset (frames decoded by the C++ reader, then the same
    sd_stereo_preprocess) equals the DataLoader path, plain and with augmentation (RNG in a num_workers=0 order)."""
    from stereo_depth_estimation_amd import dataset as D

    write_stereo_tree(tmp_path / "data", scenes=2, frames=5, hw=(45, 61), seed=9)
    samples = D.discover_samples(tmp_path / "data")
    for aug in (False, True):
        ds = D.FoundationStereoDataset(samples, image_size=(24, 32), augment=aug, brightness_jitter=0.2,
                                       hue_jitter=0.05, blur_prob=0.5, blur_sigma_max=1.0, noise_std_max=0.02)
        assert not D.DeviceLoader(ds, batch_size=3, device=DEV).native  # opt-in for PNG sources
        runs = {}
        for native in (True, False):
            torch.manual_seed(13)
            ld = D.DeviceLoader(ds, batch_size=3, shuffle=True, device=DEV, native=native, num_workers=0)
            runs[native] = [{k: v.cpu() for k, v in b.items()} for b in ld]
        assert [b["input"].shape[0] for b in runs[True]] == [3, 3, 3, 1]
        for a, b in zip(runs[True], runs[False]):
            for k in ("input", "target", "valid_mask"):
                assert torch.equal(a[k], b[k]), (aug, k)
