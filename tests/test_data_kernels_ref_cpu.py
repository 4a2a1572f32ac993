"""tests/data_kernels_ref.py and the dtype-generic oracle/aug_ref.py: the conditions the augmentation and cache-decode
cases promise, and that the GPU tests' checks reject the defects they are aimed at. No GPU."""

import numpy as np
import pytest
import torch

import data_kernels_ref as D
from oracle import aug_ref


@pytest.mark.parametrize("ks", [3, 5, 9, 31])
@pytest.mark.parametrize("sigma", [0.1, 0.7, 1.9, 4.0])
def test_float32_gaussian_kernel_is_bit_identical_to_the_old_spelling(ks, sigma):
    half = (ks - 1) * 0.5
    x = torch.linspace(-half, half, steps=ks)  # the spelling before the dtype argument
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    old = pdf / pdf.sum()
    assert old.dtype == torch.float32
    assert torch.equal(aug_ref._gaussian_kernel1d(ks, sigma), old)
    assert torch.equal(aug_ref._gaussian_kernel1d(ks, sigma, torch.float32), old)
    k64 = aug_ref._gaussian_kernel1d(ks, sigma, torch.float64)
    assert k64.dtype == torch.float64 and float((k64 - old.double()).abs().max()) < 1e-6


def test_augment_restatement_runs_in_float64_and_float32_alike():
    x = D.make_aug_batch(9, 11, seed=1)
    img = x[0, :3]
    a32 = aug_ref.augment_rgb(img.clone(), 0.9, 1.1, 0.8, 0.1, 1.2, 0.7, 5)
    a64 = aug_ref.augment_rgb(img.double(), 0.9, 1.1, 0.8, 0.1, 1.2, 0.7, 5)
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64
    assert float((a32.double() - a64).abs().max()) < 1e-5


def test_every_augmentation_case_is_well_conditioned():
    """The fp32 restatement's deviation from the float64 one, which the GPU test's tolerance is 8 x of, stays below
    DEV32_CAP = 1e-5 on every case: a condition on the inputs. (Without the lift of exact zeros ahead of gamma 0.1
    the hue round trip's residuals of a few 1e-8 come out of x**0.1 as 0.2.)"""
    worst = {}
    for hw, ks, fs in D.aug_cases():
        _, _, ref, dev32, tol = D.aug_case(hw, ks, fs)
        assert dev32 < D.DEV32_CAP, (hw, ks, fs, dev32)
        assert tol == max(8 * dev32, 4 * D.U32)
        assert float(ref.min()) >= 0.0 and float(ref.max()) <= 1.0
        worst[fs] = max(worst.get(fs, 0.0), dev32)
    print("fp32-CPU deviation, largest per factor set:", {k: f"{v:.3g}" for k, v in worst.items()})


@pytest.mark.parametrize("hw", list(D.AUG_SIZES))
def test_augmentation_images_hold_the_planted_pixels(hw):
    x = D.make_aug_batch(*hw, seed=3)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    for b in range(x.shape[0]):
        for side in range(2):
            px = x[b, 3 * side:3 * side + 3].reshape(3, -1).t()
            for want in D.PLANTED + D.NEAR_WHITE:
                assert bool((px == torch.tensor(want, dtype=torch.float32)).all(1).any()), (b, side, want)
            rest = px[(px != 0).all(1)]
            assert float(rest.min()) >= 0.05 - 1e-7  # what is not exactly 0 is 0.05 or more


def test_factor_sets_reach_the_ends_and_differ_within_each_pair():
    rows = [r for fs in D.FACTOR_SETS.values() for r in fs]
    col = lambda i: {round(r[i], 6) for r in rows}  # noqa: E731
    assert 0.0 in col(0) and 1.4 in col(0) and 0.0 in col(1) and 0.0 in col(2)
    assert {-0.5, 0.0, 0.5} <= col(3) and {0.0, 0.1, 1.0, 2.0} <= col(4) and {0.0, 0.1, 1.9} <= col(5)
    for fs in D.FACTOR_SETS.values():
        assert len(fs) == 6
        for b in range(3):
            assert all(fs[2 * b][i] != fs[2 * b + 1][i] for i in range(6))
    # the existing test's factors, unchanged
    assert D.FACTOR_SETS["mid"][4][:5] == [0.7 + 0.4, 1.3 - 0.4, 0.6 + 0.6, 0.0, 0.8 + 0.28]


@pytest.mark.parametrize("hw,ks", [((5, 7), 9), ((37, 53), 5), ((40, 52), 3)])
def test_augmentation_check_fails_swapped_factors_and_wrong_padding(hw, ks):
    """The GPU test's check, run on the fp32 restatement as the kernel: faithful it passes; with each pair's factors
    swapped, or the blur padded by edge replication or by a reflection that repeats the edge pixel (a reflect that
    clamps instead of mirroring about the edge), it fails."""
    for fs in D.FACTOR_SETS:
        x, params, ref, dev32, tol = D.aug_case(hw, ks, fs)
        D.aug_check("faithful", D.aug_restated(x, params, ks, torch.float32), ref, tol, dev32)
        for mutate in ("swap_lr", "replicate", "symmetric"):
            with pytest.raises(AssertionError):
                D.aug_check(mutate, D.aug_restated(x, params, ks, torch.float32, mutate), ref, tol, dev32)


def _old_counter(plane, HW, px):
    return (plane * HW + px) >> 1


def _new_counter(plane, HW, px):
    return plane * ((HW + 1) >> 1) + (px >> 1)


def test_noise_counter_is_one_per_pixel_pair_and_unchanged_for_even_planes():
    """k_aug_blur_noise draws one Box-Muller pair per two pixels of a plane. plane * ceil(HW/2) + px/2 is distinct over
    all (plane, pair) for every HW and equals the former (plane*HW + px) >> 1 when HW is even; the former gave the
    last pixel of an even plane and the first pair of the next plane the same counter when HW is odd."""
    for HW in (35, 37 * 53, 1):
        seen = {}
        for plane in range(12):
            for px in range(0, HW, 2):
                c = _new_counter(plane, HW, px)
                assert c not in seen, (HW, plane, px, seen.get(c))
                seen[c] = (plane, px)
    assert _old_counter(0, 35, 34) == _old_counter(1, 35, 0) == 17  # the collision
    for HW in (2, 36, 128 * 160, 240 * 320, 480 * 640):
        for plane in (0, 1, 2, 5, 11, 383):
            for px in (0, 2, HW - 2):
                assert _new_counter(plane, HW, px) == _old_counter(plane, HW, px)


@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (8, 1, 1), (2, 3, 6), (2, 37, 53), (3, 24, 32)])
def test_cache_cases_hold_the_specials_and_both_end_bytes(B, H, W):
    left, right, disp = D.make_cache_batch(B, H, W, seed=H * W)
    for a in (left, right):
        for c in range(3):
            assert (a[..., c] == 0).any() and (a[..., c] == 255).any()
    for bits in D.F16_PLANTED:
        assert (disp == bits).any(), hex(int(bits))
    inp, t, valid = D.cache_decode_ref(left, right, disp)
    assert inp.dtype == np.float32 and t.dtype == np.float32 and inp.shape == (B, 6, H, W) and t.shape == (B, 1, H, W)
    assert inp.min() == 0.0 and inp.max() == 1.0
    # the specials: valid exactly for the values > 0; NaN and -0 are invalid; the decode is exact
    sp_t = D.F16_PLANTED.view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(sp_t > 0, D.F16_VALID)
    assert np.signbit(sp_t[1]) and sp_t[1] == 0 and sp_t[2] == 2.0 ** -24 and sp_t[4] == 65504.0 and np.isnan(sp_t[7])
    for bits, ok in zip(D.F16_PLANTED, D.F16_VALID):
        sel = valid.reshape(-1)[disp.reshape(-1) == bits]
        assert sel.size and bool(sel.all()) == bool(ok) == bool(sel.any())
