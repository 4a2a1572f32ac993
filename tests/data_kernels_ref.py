"""Cases, float64 references and tolerances for the data path's element-wise kernels (csrc/data.hip): the colour
augmentation sd_augment_rgb and the cache decode sd_stereo_from_cache.

Everything here is NumPy / torch on the CPU and imports nothing from the package. The augmentation's statement is
oracle/aug_ref.py (torchvision's published tensor algorithms), run on float64 tensors; tests/test_data_kernels_ref_cpu.py
checks the conditions the cases promise, and tests/test_gpu_data.py holds the kernels to them.

Tolerance of an augmentation case (the project's `expf` rule, tests/test_gpu_train_kernels.py): 8 x the largest
deviation of the fp32 CPU restatement from the float64 one on the case's own inputs, floored at 4 * 2^-24. The kernel's
exp2/log2 and expf are not torch's, so it gets the same margin as the heads' expf. The deviation of every case stays
below DEV32_CAP (asserted on the CPU), so no case is ill-conditioned enough to let the bound go loose.
"""

from __future__ import annotations

import numpy as np
import torch

from oracle import aug_ref

U32 = 2.0 ** -24
DEV32_CAP = 1e-5

# primaries and secondaries, black, white, two greys, the three two-channel ties, two ramps
PLANTED = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0, 0, 0), (1, 1, 1), (.25, .25, .25),
           (.75, .75, .75), (.75, .75, .25), (.25, .75, .75), (.75, .25, .75), (1, .5, 0), (0, .5, 1)]
NEAR_WHITE = [(.9, .95, 1.0), (.99, .8, .97)]  # brightness 1.4 sends them over 1: the clamps

AUG_SIZES = {
    (5, 7): (3, 5, 9),  # odd HW; ks = 9: half-width 4 = H - 1
    (37, 53): (3, 5, 9, 31),
    (40, 52): (3, 5, 9),  # even HW
    (132, 128): (3, 5, 9),  # HW = 16896 > 64*256: the pointwise loop takes a second trip
    (96, 96): (3, 5, 9),  # HW = 9216 > 32*256: the mean's loop takes a second trip
    (132, 252): (3,),  # HW = 33264 > 2*64*256: the blur's loop (two pixels per thread) takes a second trip
}

# [brightness, contrast, saturation, hue, gamma, sigma] per image of three pairs (left, right, left, ...): the two
# images of a pair never share a value, so a left/right mix-up shows
FACTOR_SETS = {
    "ends_a": [[0.0, 1.2, 0.8, 0.1, 1.5, 0.0],  # brightness 0: a black image
               [1.1, 0.0, 1.3, -0.2, 1.0, 0.1],  # contrast 0: every pixel is the mean; sigma 0.1
               [0.9, 1.1, 0.0, 0.5, 2.0, 1.9],  # saturation 0: exact greys into the hue step; hue +0.5, gamma 2
               [1.0, 0.9, 1.2, -0.5, 1.0, 0.0],  # hue -0.5
               [1.0, 0.8, 1.0, 0.0, 0.1, 0.1],  # gamma 0.1, hue 0; contrast 0.8 lifts the exact zeros to 0.2 * mean
               [1.4, 1.3, 1.4, 0.05, 0.8, 1.9]],  # brightness 1.4: the clamps
    "ends_b": [[1.4, 0.7, 0.6, 0.5, 2.0, 1.9],
               [1.0, 1.0, 1.0, -0.5, 0.0, 0.0],  # gamma 0 on an image with exact zeros: 0**0 = 1
               [1.0, 0.8, 1.0, 0.5, 0.1, 1.9],  # gamma 0.1 behind a hue shift of 0.5 (zeros lifted as above)
               [0.8, 0.0, 0.0, 0.0, 1.0, 0.1],
               [1.2, 1.3, 0.0, -0.5, 2.0, 0.0],
               [0.0, 0.0, 1.0, 0.3, 0.0, 0.7]],  # black, then gamma 0: a white image
    # the factors of test_augment_matches_torchvision_restatement
    "mid": [[0.7 + 0.1 * im, 1.3 - 0.1 * im, 0.6 + 0.15 * im, [-0.08, 0.0, 0.05][im % 3], 0.8 + 0.07 * im,
             [0.0, 0.7, 1.9][im % 3]] for im in range(6)],
}


def aug_cases():
    return [(hw, ks, fs) for hw, kss in AUG_SIZES.items() for ks in kss for fs in FACTOR_SETS]


def make_aug_batch(H, W, seed, B=3):
    """[B][6][H][W] fp32 in [0, 1]: random pixels whose channels are 0.05 or more (a value that is not exactly 0 stays
    away from 0, where gamma 0.1 is ill-conditioned), with the PLANTED and NEAR_WHITE pixels written into every image
    at scattered positions (the first ones when the image has no more than that)."""
    g = torch.Generator().manual_seed(seed)
    x = 0.05 + 0.95 * torch.rand(B, 6, H, W, generator=g)
    pix = torch.tensor(PLANTED + NEAR_WHITE, dtype=torch.float32)
    n = len(pix)
    assert H * W >= n
    for b in range(B):
        for side in range(2):
            pos = torch.randperm(H * W, generator=g)[:n]
            x[b, 3 * side:3 * side + 3].view(3, H * W)[:, pos] = pix.t()
    return x


def aug_params(fs):
    """The 2B x 7 parameter rows of sd_augment_rgb for a factor set, noise off."""
    return [list(map(float, row)) + [0.0] for row in FACTOR_SETS[fs]]


def aug_restated(x, params, ks, dtype, mutate=None):
    """oracle.aug_ref.augment_rgb on every image of the batch in `dtype`; [B][6][H][W]. mutate: a defect for the
    tests of the check itself: 'swap_lr' applies each pair's factors to the other image, 'replicate' / 'symmetric'
    pad the blur by edge replication / by a reflection that repeats the edge pixel."""
    out = torch.empty(x.shape, dtype=dtype)
    for im in range(2 * x.shape[0]):
        b, side = im // 2, im % 2
        p = params[im ^ 1] if mutate == "swap_lr" else params[im]
        img = x[b, 3 * side:3 * side + 3].to(dtype).clone()
        if mutate in ("replicate", "symmetric") and p[5] > 0:
            img = aug_ref.augment_rgb(img, p[0], p[1], p[2], p[3], p[4], 0.0, ks)
            pad = ks // 2
            if mutate == "replicate":
                xp = torch.nn.functional.pad(img[None], [pad] * 4, mode="replicate")[0]
            else:
                H, W = img.shape[-2:]
                iy = torch.tensor([(-1 - i if i < 0 else (2 * H - 1 - i if i >= H else i)) for i in range(-pad, H + pad)])
                ix = torch.tensor([(-1 - i if i < 0 else (2 * W - 1 - i if i >= W else i)) for i in range(-pad, W + pad)])
                xp = img[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            k1 = aug_ref._gaussian_kernel1d(ks, p[5], dtype)
            k2 = torch.mm(k1[:, None], k1[None, :]).expand(3, 1, ks, ks)
            out[b, 3 * side:3 * side + 3] = torch.nn.functional.conv2d(xp[None], k2, groups=3)[0].clamp_(0.0, 1.0)
        else:
            out[b, 3 * side:3 * side + 3] = aug_ref.augment_rgb(img, p[0], p[1], p[2], p[3], p[4], p[5], ks)
    return out


_AUG = {}


def aug_case(hw, ks, fs):
    """(x, params, float64 reference, dev32, tol) of a case, computed once: dev32 the largest deviation of the fp32
    restatement from the float64 one, tol = max(8 * dev32, 4 * 2^-24)."""
    key = (hw, ks, fs)
    if key not in _AUG:
        x = make_aug_batch(*hw, seed=hw[0] * 1000 + hw[1])
        params = aug_params(fs)
        ref = aug_restated(x, params, ks, torch.float64)
        dev32 = float((aug_restated(x, params, ks, torch.float32).double() - ref).abs().max())
        _AUG[key] = (x, params, ref, dev32, max(8 * dev32, 4 * U32))
    return _AUG[key]


def aug_check(name, got, ref, tol, dev32):
    """|got - ref| <= tol over the whole batch, nothing NaN; prints the figures."""
    got = got.double()
    assert not bool(torch.isnan(got).any()), name
    dev = float((got - ref).abs().max())
    print(f"RATIO {name} dev/allowed={dev / tol:.3g} maxdev={dev:.3g} fp32-CPU deviation={dev32:.3g} allowed={tol:.3g}")
    assert dev <= tol, (name, dev, tol)
    return dev / tol


# ------------------------------------------------------------------ sd_stereo_from_cache (dataset.py:86-105)
F16_PLANTED = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7BFF, 0x7C00, 0xFC00, 0x7E00], dtype=np.uint16)
#                        +0      -0      min sub  -min sub 65504   +inf    -inf    NaN
F16_VALID = np.array([0, 0, 1, 0, 1, 1, 0, 0], dtype=bool)  # t > 0: NaN and -0 are invalid


def make_cache_batch(B, H, W, seed):
    """uint8 left/right [B][H][W][3] with bytes 0 and 255 in every channel, float16 disparities [B][H][W] (as uint16
    bits) with the F16_PLANTED specials at the front of every sample as far as they fit."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    right = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    for a in (left, right):
        flat = a.reshape(B, H * W, 3)
        flat[:, 0, :] = 0
        flat[:, -1, :] = 255
        if H * W == 1:  # one pixel per sample: the two bytes alternate over the batch
            flat[0::2, 0, :] = 0
    disp = rng.uniform(-1, 50, (B, H, W)).astype(np.float16).view(np.uint16)
    flat = disp.reshape(B, H * W)
    if H * W < len(F16_PLANTED):  # the specials in turn over the samples
        flat[:, 0] = F16_PLANTED[np.arange(B) % len(F16_PLANTED)]
    else:
        flat[:, :len(F16_PLANTED)] = F16_PLANTED
    return left, right, disp


def cache_decode_ref(left, right, disp_bits):
    """load_cached_sample: uint8 / 255 in fp32 (CHW, left then right), float16 -> float32, valid = t > 0."""
    lf = np.transpose(left.astype(np.float32) / np.float32(255.0), (0, 3, 1, 2))
    rf = np.transpose(right.astype(np.float32) / np.float32(255.0), (0, 3, 1, 2))
    t = disp_bits.view(np.float16).astype(np.float32)[:, None]
    with np.errstate(invalid="ignore"):
        valid = t > 0
    return np.concatenate([lf, rf], 1), t, valid
