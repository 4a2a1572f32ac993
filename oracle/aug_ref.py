"""ORACLE — test infrastructure only (see oracle/__init__.py).

Restatement of the colour augmentation the reference applies per image in
``FoundationStereoDataset._augment_rgb`` (``dataset.py:248-270``). The ops come from
torchvision 0.25.0 (pinned in the reference's ``uv.lock:2346-2347``; not installed here), so
this file restates torchvision's published tensor algorithms (``torchvision/transforms/
_functional_tensor.py``: ``_blend``, ``rgb_to_grayscale``, ``adjust_brightness/contrast/
saturation/hue/gamma``, ``_rgb2hsv``, ``_hsv2rgb``, ``gaussian_blur`` with
``_get_gaussian_kernel2d`` and reflect padding). No reference test pins these ops: parity for
the augmentation is "unpinned"  and rests on this restatement.
Tensors are CHW float32 in [0, 1] on the CPU; float64 tensors run through the same code and
give the float64 statement.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F


def _blend(img1: torch.Tensor, img2: torch.Tensor, ratio: float) -> torch.Tensor:
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 1.0)


def rgb_to_grayscale(img: torch.Tensor) -> torch.Tensor:
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)


def adjust_brightness(img, f):
    return _blend(img, torch.zeros_like(img), f)


def adjust_contrast(img, f):
    mean = torch.mean(rgb_to_grayscale(img), dim=(-3, -2, -1), keepdim=True)
    return _blend(img, mean, f)


def adjust_saturation(img, f):
    return _blend(img, rgb_to_grayscale(img), f)


def _rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - s * (1.0 - f))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=i.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def adjust_hue(img, hue_factor):
    if not (-0.5 <= hue_factor <= 0.5):
        raise ValueError(f"hue_factor ({hue_factor}) is not in [-0.5, 0.5].")
    hsv = _rgb2hsv(img)
    h, s, v = hsv.unbind(dim=-3)
    h = (h + hue_factor) % 1.0
    return _hsv2rgb(torch.stack((h, s, v), dim=-3))


def adjust_gamma(img, gamma, gain=1.0):
    if gamma < 0:
        raise ValueError("Gamma should be a non-negative real number")
    return (gain * img**gamma).clamp(0, 1)


def _gaussian_kernel1d(kernel_size: int, sigma: float, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    ksize_half = (kernel_size - 1) * 0.5
    x = torch.linspace(-ksize_half, ksize_half, steps=kernel_size, dtype=dtype)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(img, kernel_size: int, sigma: float):
    k1 = _gaussian_kernel1d(kernel_size, sigma, img.dtype)  # the image's type: float64 images give a float64 statement
    k2 = torch.mm(k1[:, None], k1[None, :])
    kernel = k2.expand(img.shape[-3], 1, kernel_size, kernel_size)
    pad = kernel_size // 2
    x = F.pad(img[None], [pad, pad, pad, pad], mode="reflect")
    return F.conv2d(x, kernel, groups=img.shape[-3])[0]


def augment_rgb(img, brightness, contrast, saturation, hue, gamma, blur_sigma, kernel_size, noise=None):
    """dataset.py:248-270 with the sampled factors given; noise (a field) optional."""
    img = adjust_brightness(img, brightness)
    img = adjust_contrast(img, contrast)
    img = adjust_saturation(img, saturation)
    img = adjust_hue(img, hue)
    img = adjust_gamma(img, gamma, gain=1.0)
    if blur_sigma > 0:
        img = gaussian_blur(img, kernel_size, blur_sigma)
    if noise is not None:
        img = img + noise
    return img.clamp_(0.0, 1.0)
