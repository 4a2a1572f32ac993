"""Float64 references and input builders for the training step's small kernels: the BatchNorm finalizes, reduces and
apply (csrc/bn.hip), the fused heads + loss + gradient (csrc/heads.hip), AdamW and the valid count (csrc/misc.hip),
the MaxPool2d forward (csrc/conv_fast.hip) and backward + skip add (csrc/bn.hip).

Everything here is NumPy / torch on the CPU and imports nothing from the package. Each operation is stated from the
contract in include/stereo_hip.h and the lines of the reference model it cites; tests/test_train_kernels_ref_cpu.py
ties every statement to independent torch float64 machinery (F.batch_norm + autograd, nn.BatchNorm2d,
torch.optim.AdamW), and tests/test_gpu_train_kernels.py holds the kernels to these statements.

Inputs are rounded to the path's storage type first (``store``), on both sides: the references then see exactly the
numbers the kernels load, and every difference is arithmetic.
"""

from __future__ import annotations

import math

import numpy as np
import torch

U32 = 2.0 ** -24  # unit roundoff of fp32 (round to nearest)
U64 = 2.0 ** -53
UBF16 = 2.0 ** -8  # unit roundoff of bf16 (8 significant bits): round to nearest errs by up to 2^-8 * |x| just above a
#                    power of two and 2^-9 * |x| just below one; truncation by up to twice that
EPS_BN = float(np.float32(1e-5))  # the C ABI takes `float eps` and `float momentum`: the kernels see fp32(1e-5),
MOMENTUM = float(np.float32(0.1))  # fp32(0.1); the references use the same two numbers
BRANCH_MARGIN = 1e-3
LV_MIN, LV_MAX = -6.0, 3.0
SOFTPLUS_THRESHOLD = 20.0


def store(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """x rounded to the storage type (what both the kernel and the reference read)."""
    return x.to(dtype)


def f64(x) -> torch.Tensor:
    return torch.as_tensor(x).double()


def bf16_store_interval(ref, tol32):
    """The bf16 values a round-to-nearest-even store can produce from an fp32 value within tol32 of ref: rounding is
    monotonic, so they are the bf16 numbers from RNE(ref - tol32) to RNE(ref + tol32). No constant is added for the
    store itself: where tol32 is far below the bf16 spacing the two ends coincide and the stored bits are pinned,
    which truncation (or rounding half away from zero on a tie) misses. One fp32 ulp is added to tol32 because torch
    converts float64 to bf16 through fp32."""
    ref = f64(ref)
    t = torch.as_tensor(tol32, dtype=torch.float64) + 2 * U32 * ref.abs()
    return (ref - t).float().to(torch.bfloat16).double(), (ref + t).float().to(torch.bfloat16).double()


# ------------------------------------------------------------------ BatchNorm (model.py:37-41)
def bn_autograd(y, gamma, beta, da, eps=EPS_BN):
    """relu(F.batch_norm(y, None, None, gamma, beta, training=True)) over y [P][C] in float64 and its backward for the
    upstream gradient da: (a, dy, dgamma, dbeta). The independent machinery the restatements below are checked with."""
    y = f64(y).clone().requires_grad_(True)
    g = f64(gamma).clone().requires_grad_(True)
    b = f64(beta).clone().requires_grad_(True)
    a = torch.relu(torch.nn.functional.batch_norm(y, None, None, g, b, training=True, eps=eps))
    dy, dg, db = torch.autograd.grad(a, (y, g, b), f64(da))
    return a.detach(), dy, dg, db


def bn_fwd_from_sums(s, ss, count, gamma, beta, eps=EPS_BN):
    """sd_bn_fwd_finalize: per-channel (sum, sumsq) over `count` pixels -> mean, var (biased, clamped at 0), invstd,
    scale = gamma*invstd, shift = beta - mean*scale."""
    s, ss, gamma, beta = f64(s), f64(ss), f64(gamma), f64(beta)
    mean = s / count
    var = (ss / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    return mean, var, invstd, scale, beta - mean * scale


def bn_running(rm, rv, mean, var, count, momentum):
    """The running-statistics update of nn.BatchNorm2d: momentum-weighted, the variance unbiased (count == 1: the
    biased one, there is nothing to correct with)."""
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return momentum * mean + (1.0 - momentum) * f64(rm), momentum * unbiased + (1.0 - momentum) * f64(rv)


def bn_eval_coeffs(rm, rv, gamma, beta, eps=EPS_BN):
    """sd_bn_eval_coeffs: mean = running_mean, invstd = 1/sqrt(running_var + eps), scale, shift."""
    rm, rv = f64(rm), f64(rv)
    invstd = 1.0 / torch.sqrt(rv + eps)
    scale = f64(gamma) * invstd
    return rm, invstd, scale, f64(beta) - rm * scale


def relu_mask(y, scale, shift):
    """[scale*y + shift > 0] as the kernels' fp32 fma decides it, for EVERY input: y and scale carry at most 24
    significant bits each, so their product is exact in float64 (48 <= 53 bits); the float64 sum with shift and the
    fma's single rounding of the same exact value both preserve its sign (rounding to nearest never crosses zero and
    maps only zero to zero; fp32 subnormals keep nonzero values of this size nonzero). A kernel that rounds the
    product before the add (separate multiply and add) differs where the exact sum is a rounding residual, which
    ``plant_mask_cases`` puts into the inputs. No element needs to be left out of a comparison."""
    return f64(y) * f64(scale) + f64(shift) > 0


def bn_bwd_sums(da, y, scale, shift, mean, invstd):
    """sd_bn_bwd_reduce summed over its rows: dz = da*[scale*y+shift > 0], xhat = (y-mean)*invstd ->
    (sum dz, sum dz*xhat, sum |dz|, sum |dz*xhat|) per channel (the last two for the rounding bounds)."""
    dz = torch.where(relu_mask(y, scale, shift), f64(da), torch.zeros((), dtype=torch.float64))
    t = dz * ((f64(y) - f64(mean)) * f64(invstd))
    return dz.sum(0), t.sum(0), dz.abs().sum(0), t.abs().sum(0)


def bn_bwd_coef(s1, s2, count, gamma, invstd, batch_stats=True):
    """sd_bn_bwd_finalize: coef[C][3] = {gamma*invstd, sum dz / N, sum dz*xhat / N} (eval mode: {gamma*invstd, 0, 0})."""
    k0 = f64(gamma) * f64(invstd)
    z = torch.zeros_like(k0)
    return torch.stack([k0, f64(s1) / count if batch_stats else z, f64(s2) / count if batch_stats else z], 1)


def bn_bwd_apply(da, y, scale, shift, mean, invstd, coef):
    """sd_bn_bwd_apply: dy = coef0*(dz - coef1 - xhat*coef2)."""
    dz = torch.where(relu_mask(y, scale, shift), f64(da), torch.zeros((), dtype=torch.float64))
    xh = (f64(y) - f64(mean)) * f64(invstd)
    c = f64(coef)
    return c[:, 0] * (dz - c[:, 1] - xh * c[:, 2])


def bn_bwd_restated(y, gamma, beta, da, eps=EPS_BN):
    """The whole train-mode backward through the restatements above: (dy, dgamma, dbeta)."""
    y = f64(y)
    P = y.shape[0]
    mean, _, invstd, scale, shift = bn_fwd_from_sums(y.sum(0), (y * y).sum(0), P, gamma, beta, eps)
    s1, s2, _, _ = bn_bwd_sums(da, y, scale, shift, mean, invstd)
    coef = bn_bwd_coef(s1, s2, P, gamma, invstd)
    return bn_bwd_apply(da, y, scale, shift, mean, invstd, coef), s2, s1


def make_bn_bwd_inputs(P, C, dtype, seed):
    """da, y [P][C] in the storage type and fp32 per-channel scale (both signs), shift, mean, invstd, with the exact
    mask cases planted (``plant_mask_cases``)."""
    g = torch.Generator().manual_seed(seed)
    y = store(torch.randn(P, C, generator=g), dtype)
    da = store(torch.randn(P, C, generator=g) + 0.25, dtype)
    scale = torch.rand(C, generator=g) + 0.5
    scale[1::3] *= -1
    shift = torch.randn(C, generator=g) * 0.3
    mean = torch.randn(C, generator=g) * 0.2
    invstd = torch.rand(C, generator=g) + 0.5
    plant_mask_cases(y, da, scale, shift)
    return da, y, scale, shift, mean, invstd


def plant_mask_cases(y, da, scale, shift):
    """In place, on pixel rows 0 and 1 where they exist:
    even channels: shift = 0 and y[0] = 0, so z == 0 exactly: masked out by `> 0`, let through by `>= 0`;
    odd channels (P >= 2): shift = -fp32(y[1]*scale), so the exact z is the rounding residual of the product: an fma
    sees its sign, a separate multiply and add sees 0. da is 1.5 at both, far above any summation bound."""
    P, C = y.shape
    shift[0::2] = 0.0
    y[0, 0::2] = 0.0
    da[0, 0::2] = 1.5
    if P >= 2:
        prod = y[1, 1::2].float() * scale[1::2]  # rounded to fp32
        shift[1::2] = -prod
        da[1, 1::2] = 1.5


def make_balanced_bn(P, C, seed):
    """The end-to-end chain's input: y[:, c] = m_c +- s_c*(0.25 + |u|) in balanced +- pairs, beta = 0, so every
    |z| = |gamma*xhat| stays away from 0 and the ReLU mask is the same under float64 and fp32 statistics; nothing has
    to be excluded. Returns fp32-representable y [P][C], gamma (both signs), beta, da."""
    assert P % 2 == 0
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(C, generator=g) * 0.5
    s = torch.rand(C, generator=g) + 0.5
    u = 0.25 + torch.randn(P // 2, C, generator=g).abs()
    y = torch.cat([m + s * u, m - s * u], 0)
    y = y[torch.randperm(P, generator=g)].float().contiguous()
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1
    da = torch.randn(P, C, generator=g).float()
    return y, gamma.float(), torch.zeros(C), da


def bn_min_abs_z(y, gamma, beta, eps=EPS_BN):
    y = f64(y)
    mean, _, _, scale, shift = bn_fwd_from_sums(y.sum(0), (y * y).sum(0), y.shape[0], gamma, beta, eps)
    return float((y * scale + shift).abs().min())


# ------------------------------------------------------------------ heads + loss (model.py:76-77,98,103; train.py:329-352)
INFER, LOSS, GRADS = 0, 1, 2


def valid_pixels(target, mask):
    """train.py:329-330: mask != 0 (any nonzero byte) and a finite target."""
    return (torch.as_tensor(mask) != 0) & torch.isfinite(torch.as_tensor(target))


def heads_ref(inp, mode):
    """Float64 statement by autograd. inp: dict with y [P][C] (storage type), scale, shift, wd, wl [C], bd, bl [1] fp32
    and, LOSS: target [P] fp32, mask [P] uint8; GRADS: gdisp, glogvar [P] fp32.
    Returns disp, logvar [P]; LOSS / GRADS also da [P][C], dwd, dwl [C], dbd, dbl, and LOSS metrics[5] =
    (sum nll, sum |d|, sum d^2, sum exp(lv/2), n) and n, plus the per-pixel head gradients gxd, gxl and the sums of
    absolute terms the rounding bounds need. With n == 0 the step is skipped: every gradient is zero."""
    y, sc, sh = f64(inp["y"]), f64(inp["scale"]), f64(inp["shift"])
    act = torch.relu(y * sc + sh).requires_grad_(mode != INFER)
    wd, wl, bd, bl = (f64(inp[k]).clone().requires_grad_(mode != INFER) for k in ("wd", "wl", "bd", "bl"))
    xd, xl = act @ wd + bd, act @ wl + bl
    disp = torch.nn.functional.softplus(xd, beta=1.0, threshold=SOFTPLUS_THRESHOLD)
    logvar = torch.clamp(xl, LV_MIN, LV_MAX)
    out = {"disp": disp.detach(), "logvar": logvar.detach(), "xd": xd.detach(), "xl": xl.detach(), "act": act.detach(),
           # per-pixel condition of the two dot products, sum |act*w| + |b|: one fp32 rounding of a value that depends
           # on them moves it by about 2^-24 times this (the GPU test's guard against a lucky yardstick sample)
           "s_d": (act.detach().abs() @ wd.detach().abs() + bd.detach().abs()),
           "s_l": (act.detach().abs() @ wl.detach().abs() + bl.detach().abs())}
    if mode == INFER:
        return out
    leaves = (act, wd, bd, wl, bl, xd, xl)  # xd, xl: the per-pixel head gradients, for the summation bounds
    if mode == LOSS:
        valid = valid_pixels(inp["target"], inp["mask"])
        n = int(valid.sum())
        out["n"] = n
        if n == 0:
            grads = [torch.zeros_like(v) for v in leaves]
            out["metrics"] = torch.zeros(5, dtype=torch.float64)
            out["metric_abs"] = torch.zeros(5, dtype=torch.float64)
            out["metric_scale"] = torch.zeros(5, dtype=torch.float64)
        else:
            t = f64(inp["target"])[valid]
            p, lv = disp[valid], logvar[valid]
            nll = (p - t).abs() * torch.exp(-lv) + lv
            grads = torch.autograd.grad(nll.mean(), leaves)
            d = (p - t).detach()
            lvd = lv.detach()
            out["metrics"] = torch.stack([nll.detach().sum(), d.abs().sum(), (d * d).sum(), torch.exp(0.5 * lvd).sum(),
                                          torch.tensor(float(n), dtype=torch.float64)])
            out["metric_abs"] = torch.stack([(d.abs() * torch.exp(-lvd) + lvd.abs()).sum(), d.abs().sum(),
                                             (d * d).sum(), torch.exp(0.5 * lvd).sum(),
                                             torch.zeros((), dtype=torch.float64)])
            k = (2.0 + out["s_d"] + out["s_l"])[valid]  # each term weighted by its pixel's condition
            out["metric_scale"] = torch.stack([((d.abs() * torch.exp(-lvd) + lvd.abs()) * k).sum(), (d.abs() * k).sum(),
                                               (d * d * k).sum(), (torch.exp(0.5 * lvd) * k).sum(),
                                               torch.zeros((), dtype=torch.float64)])
    else:
        grads = torch.autograd.grad((disp * f64(inp["gdisp"])).sum() + (logvar * f64(inp["glogvar"])).sum(), leaves)
    out["da"], out["dwd"], out["dbd"], out["dwl"], out["dbl"], out["gxd"], out["gxl"] = grads
    return out


def heads_fp32(inp, mode, flip=False):
    """The same formulas with torch fp32 operations on the CPU, as csrc/heads.hip spells them (explicit gradient, no
    autograd): its deviation from ``heads_ref`` on the same inputs is the yardstick for the device's expf / log1pf
    and summation order. flip: the channel sums taken in the opposite order (a second sample of the summation error).
    Returns the same keys as heads_ref (da in fp32)."""
    f = torch.float32
    y = torch.as_tensor(inp["y"]).to(f)
    act = torch.relu(y * inp["scale"].to(f) + inp["shift"].to(f))
    wd, wl, bd, bl = (inp[k].to(f) for k in ("wd", "wl", "bd", "bl"))
    if flip:
        xd = (act.flip(1) * wd.flip(0)).cumsum(1)[:, -1] + bd
        xl = (act.flip(1) * wl.flip(0)).cumsum(1)[:, -1] + bl
    else:
        xd, xl = (act * wd).cumsum(1)[:, -1] + bd, (act * wl).cumsum(1)[:, -1] + bl
    disp = torch.where(xd > SOFTPLUS_THRESHOLD, xd, torch.log1p(torch.exp(xd)))
    logvar = xl.clamp(LV_MIN, LV_MAX)
    out = {"disp": disp, "logvar": logvar}
    if mode == INFER:
        return out
    P = y.shape[0]
    gxd, gxl = torch.zeros(P, dtype=f), torch.zeros(P, dtype=f)
    z = torch.exp(xd)
    sp_grad = torch.where(xd > SOFTPLUS_THRESHOLD, torch.ones_like(xd), z / (z + 1))
    inside = (xl >= LV_MIN) & (xl <= LV_MAX)
    if mode == LOSS:
        valid = valid_pixels(inp["target"], inp["mask"])
        n = int(valid.sum())
        met = torch.zeros(5, dtype=torch.float64)
        if n:
            inv_n = torch.tensor(1.0, dtype=f) / torch.tensor(float(n), dtype=f)
            d = torch.where(valid, disp - inp["target"].to(f), torch.zeros((), dtype=f))
            e = torch.exp(-logvar)
            gp = torch.sign(d) * (inv_n * e)
            glv = inv_n - (inv_n * d.abs()) * e
            gxd = torch.where(valid, sp_grad * gp, gxd)
            gxl = torch.where(valid & inside, glv, gxl)
            nll = d.abs() * e + logvar
            met = torch.stack([nll[valid].sum(), d[valid].abs().sum(), (d[valid] * d[valid]).sum(),
                               torch.exp(0.5 * logvar[valid]).sum(), torch.tensor(float(n))]).double()
        out["n"], out["metrics"] = n, met
    else:
        gxd = sp_grad * inp["gdisp"].to(f)
        gxl = torch.where(inside, inp["glogvar"].to(f), gxl)
    out["da"] = gxd[:, None] * wd + gxl[:, None] * wl
    out["dwd"], out["dwl"] = (gxd[:, None] * act).sum(0), (gxl[:, None] * act).sum(0)
    out["dbd"], out["dbl"] = gxd.sum().reshape(1), gxl.sum().reshape(1)
    return out


def heads_near_branch(inp, mode):
    """Pixels within BRANCH_MARGIN of a branch point of the float64 reference: xl at -6 or 3 and, LOSS, p - t at 0."""
    r = heads_ref(inp, INFER)
    near = ((r["xl"] - LV_MIN).abs() < BRANCH_MARGIN) | ((r["xl"] - LV_MAX).abs() < BRANCH_MARGIN)
    if mode == LOSS:
        t = f64(inp["target"])
        near |= torch.isfinite(t) & ((r["disp"] - torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)).abs()
                                     < BRANCH_MARGIN)
    return near


def make_heads_inputs(P, C, dtype, mode, seed, all_masked=False, max_rounds=10):
    """Inputs for one heads call. Pixel rows of y are redrawn until no pixel sits within BRANCH_MARGIN of a branch point
    of the reference (``heads_near_branch``), so float64 and fp32 take the same branch everywhere and no pixel is left
    out of a comparison; the exact branch cases are planted separately (``make_heads_planted``). The heads' spread
    reaches both clamps of the log-variance and the softplus threshold. Returns (inputs, rounds used)."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.rand(C, generator=g) + 0.5
    scale[::4] *= -1
    shift = torch.randn(C, generator=g) * 0.3
    k = math.sqrt(C / 2.0)  # about C/2 channels pass the ReLU: xd, xl spread a few units whatever C
    inp = {"y": store(torch.randn(P, C, generator=g), dtype), "scale": scale, "shift": shift,
           "wd": torch.randn(C, generator=g) * (6.0 / k), "bd": torch.tensor([3.0]),
           "wl": torch.randn(C, generator=g) * (4.0 / k), "bl": torch.tensor([-1.0])}
    if mode == LOSS:
        target = torch.rand(P, generator=g) * 12.0
        mask = (torch.rand(P, generator=g) > 0.1).to(torch.uint8)
        for i, v in enumerate((float("nan"), float("inf"), float("-inf"))):
            target[5 + i::11] = v  # non-finite targets under mask 1 ...
            mask[5 + i::22] = 1
        mask[3::13] = 2  # ... nonzero bytes other than 1 count as valid, as in sd_count_valid
        mask[4::17] = 255
        if P <= 3:
            mask = torch.tensor([1, 2, 255], dtype=torch.uint8)[:P].clone()
        if all_masked:
            mask.zero_()
        inp["target"], inp["mask"] = target, mask
    elif mode == GRADS:
        inp["gdisp"] = torch.randn(P, generator=g)
        inp["glogvar"] = torch.randn(P, generator=g)
    rounds = 0
    while True:
        near = heads_near_branch(inp, mode)
        if not bool(near.any()):
            return inp, rounds
        rounds += 1
        assert rounds <= max_rounds, "heads input builder did not settle"
        inp["y"][near] = store(torch.randn(int(near.sum()), C, generator=g), dtype)


def make_heads_planted(C, dtype, case):
    """Exact branch cases on two pixels (y = 1, scale = 1, shift = 0, so act = 1):
    'lv_hi' / 'lv_lo'          wl = 0, bl = 3 / -6: xl sits on the clamp, the gradient flows;
    'lv_above' / 'lv_below'    wl = 0, bl = nextafter(3, +inf) / nextafter(-6, -inf): logvar clamped, gradient 0;
    'sp_equal'                 wd = 0, bd = 25, target = 25: p == t exactly above the softplus threshold, gradient 0;
    'sp_pass'                  wd = 0, bd = 25, target = 24: the threshold branch passes the gradient unchanged."""
    P = 2
    inp = {"y": store(torch.ones(P, C), dtype), "scale": torch.ones(C), "shift": torch.zeros(C),
           "wd": torch.linspace(-0.5, 0.7, C), "bd": torch.tensor([1.0]),
           "wl": torch.linspace(0.3, -0.2, C), "bl": torch.tensor([0.5]),
           "target": torch.tensor([2.0, 7.0]), "mask": torch.ones(P, dtype=torch.uint8)}
    if case.startswith("lv"):
        inp["wl"] = torch.zeros(C)
        bl = {"lv_hi": np.float32(3.0), "lv_lo": np.float32(-6.0),
              "lv_above": np.nextafter(np.float32(3.0), np.float32(np.inf)),
              "lv_below": np.nextafter(np.float32(-6.0), np.float32(-np.inf))}[case]
        inp["bl"] = torch.tensor([float(bl)], dtype=torch.float32)
    else:
        inp["wd"] = torch.zeros(C)
        inp["bd"] = torch.tensor([25.0])
        inp["target"] = torch.tensor([25.0 if case == "sp_equal" else 24.0, 24.0])
    return inp


def heads_bn_sums(da_stored, y, scale, shift, mean, invstd):
    """What sd_heads_bnsum adds up: the BatchNorm-backward sums over the da it stored (already rounded to the storage
    type). Returns bn_bwd_sums' four per-channel sums plus sum |dz*y| (the kernel forms sum dz*xhat as
    invstd*(sum dz*y - mean*sum dz), so its rounding scales with that)."""
    s1, s2, a1, a2 = bn_bwd_sums(da_stored, y, scale, shift, mean, invstd)
    dz = torch.where(relu_mask(y, scale, shift), f64(da_stored), torch.zeros((), dtype=torch.float64))
    return s1, s2, a1, a2, (dz * f64(y)).abs().sum(0)


# ------------------------------------------------------------------ AdamW (train.py:343,578)
def adamw_scalars(t, lr, wd, b1, b2):
    return 1.0 - lr * wd, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)


def adamw_step(p, g, m, v, t, lr, wd, b1, b2, eps):
    """One single-tensor AdamW update for step number t (1-based), float64, in the order k_adamw documents:
    param.mul_(1 - lr*wd); exp_avg.lerp_(grad, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(grad, grad, 1 - b2);
    denom = sqrt(exp_avg_sq)/sqrt(1 - b2^t) + eps; param.addcdiv_(exp_avg, denom, -lr/(1 - b1^t))."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    decay, step_size, bc2s = adamw_scalars(t, lr, wd, b1, b2)
    p = p * decay
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = torch.sqrt(v) / bc2s + eps
    return p - step_size * (m / denom), m, v


def adamw_tolerances(p0, g, m0, v0, t, lr, wd, b1, b2, eps):
    """Rounding bounds k * 2^-24 * (sum of |terms|) of one fp32 step from the state (p0, m0, v0), per element.
    m = m0 + w1*(g - m0): k = 4 (w1 as fp32, subtract, multiply, add); terms |m0|, w1*(|g| + |m0|).
    v = v0*b2 + w2*g*g:   k = 6 (b2 and w2 as fp32, three multiplies, add); terms b2*|v0|, w2*g^2 (all >= 0).
    p = p0*decay - step*(m/denom), denom = sqrt(v)/bc2s + eps: k = 20 on terms |p0*decay| and step*T_m/denom with
      T_m = |m0| + w1*(|g| + |m0|) >= |m|: decay, step, bc2s, eps as fp32 (4), the 4 of m, v's 6 halved by the square
      root (3) and the root itself (1), divide, add, divide, multiply, multiply, add (6), and 2 to spare for the
      second-order terms. Every term of denom is >= 0, so its relative error is the sum of the relative errors."""
    p0, g, m0, v0 = f64(p0), f64(g), f64(m0), f64(v0)
    decay, step_size, bc2s = adamw_scalars(t, lr, wd, b1, b2)
    w1, w2 = 1.0 - b1, 1.0 - b2
    tm = m0.abs() + w1 * (g.abs() + m0.abs())
    tol_m = 4 * U32 * tm
    v = v0 * b2 + w2 * g * g
    tol_v = 6 * U32 * v
    denom = torch.sqrt(v) / bc2s + eps
    tol_p = 20 * U32 * ((p0 * decay).abs() + step_size * tm / denom)
    return tol_p, tol_m, tol_v


# ------------------------------------------------------------------ MaxPool2d(2) of relu(bn(y)) (model.py:59,83-86)
def pool_windows(x, B, H, W):
    """NHWC rows [B*H*W][C] (or [B][H][W][C]) -> [B][H/2][W/2][4][C], window position k = 2*dy + dx."""
    C = x.shape[-1]
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)


def pool_unwindows(xw, B, H, W):
    """The inverse of ``pool_windows``: [B][H/2][W/2][4][C] -> [B][H][W][C]."""
    C = xw.shape[-1]
    return xw.reshape(B, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def bnrelu_pool_ref(y, scale, shift, B, H, W):
    """sd_bnrelu_pool: max over each 2x2 window of relu(scale*y + shift), float64, [B][H/2][W/2][C]."""
    a = torch.relu(f64(y) * f64(scale) + f64(shift))
    return pool_windows(a, B, H, W).max(3).values


def pool_bwd_ref(y, scale, shift, dskip, dpool, B, H, W):
    """sd_pool_bwd_add: da = dskip (0 when absent) + dpool at the arg-max of relu(scale*y + shift) over each 2x2
    window, the FIRST maximum in window order k = 2*dy + dx (numpy.argmax documents first occurrence).
    Returns (da [B][H][W][C] float64, argmax [B][H/2][W/2][C] int64)."""
    a = pool_windows(torch.relu(f64(y) * f64(scale) + f64(shift)), B, H, W)
    am = torch.from_numpy(np.argmax(a.numpy(), axis=3))
    hit = torch.arange(4).view(1, 1, 1, 4, 1) == am.unsqueeze(3)
    C = a.shape[-1]
    g = torch.where(hit, f64(dpool).reshape(B, H // 2, W // 2, 1, C), torch.zeros((), dtype=torch.float64))
    da = pool_unwindows(g, B, H, W)
    if dskip is not None:
        da = da + f64(dskip).reshape(B, H, W, C)
    return da, am


def pool_hit(am, B, H, W):
    """[B][H][W][C] bool: the positions ``pool_bwd_ref``'s arg-max selects."""
    return pool_unwindows(torch.arange(4).view(1, 1, 1, 4, 1) == am.unsqueeze(3), B, H, W)


def pool_top2_gap(y, scale, shift, B, H, W):
    """(smallest non-zero gap between the two largest relu(z) of any window, max |z|), z = scale*y + shift in float64."""
    z = f64(y) * f64(scale) + f64(shift)
    top = pool_windows(torch.relu(z), B, H, W).topk(2, dim=3).values
    gap = top[:, :, :, 0] - top[:, :, :, 1]
    nz = gap[gap > 0]
    return (float(nz.min()) if nz.numel() else math.inf), float(z.abs().max())


def pool_tie_shares(y, scale, shift, B, H, W):
    """Shares of window-channels with (an exact tie for a positive maximum, all four values zero after the ReLU)."""
    a = pool_windows(torch.relu(f64(y) * f64(scale) + f64(shift)), B, H, W)
    mx = a.max(3, keepdim=True).values
    ties = ((a == mx).sum(3) >= 2) & (mx.squeeze(3) > 0)
    return float(ties.double().mean()), float((mx == 0).double().mean())


def make_pool_inputs(B, H, W, C, dtype, seed):
    """Inputs of the pooling kernels, NHWC rows: y, dskip [B*H*W][C] and dpool [B*(H/2)*(W/2)][C] in the storage type,
    fp32 scale, shift, mean, invstd [C], and the (gap, max |z|) of ``pool_top2_gap``.
    y lies on a coarse grid, multiples of 2^-6 in [-4, 4] (exact in bf16: at most 8 significant bits), so exact ties
    inside a window are common; they are made commoner still: in about a third of the window-channels one position
    repeats another, and about 6 % of them are pushed to the non-positive side of their channel (all zero after the
    ReLU). |scale| is in [0.5, 1.5], every third channel negative. shift is about 0.3*N(0,1), placed half-way between
    two grid points of its channel: shift = scale*(m + 0.5)*2^-6 for an integer m, so no z = scale*y + shift is
    closer to 0 than |scale|*2^-7, and two unequal z of one channel differ by at least |scale|*2^-6: far above an
    fp32 rounding of z (2^-24 * 7), so an fp32 fma and float64 order every window the same way (the argument of
    ``relu_mask``). No window has to be left out of a comparison."""
    g = torch.Generator().manual_seed(seed)
    H2, W2 = H // 2, W // 2
    scale = torch.rand(C, generator=g) + 0.5
    scale[::3] *= -1
    m = torch.round(torch.randn(C, generator=g) * 0.3 * 64.0 / scale - 0.5)
    shift = (scale * ((m + 0.5) / 64.0)).float()
    k = torch.randint(-256, 257, (B, H2, W2, 4, C), generator=g, dtype=torch.int16)
    r = torch.rand(B, H2, W2, 1, C, generator=g)
    # one position repeats another (positions 0..3 in turn, by the same draw)
    src, dst = (r * 64).long() % 4, (r * 256).long() % 4
    copy = (r < 1.0 / 3.0) & (src != dst)
    k = torch.where(copy & (torch.arange(4).view(1, 1, 1, 4, 1) == dst), k.gather(3, src), k)
    # all four on the non-positive side: z = -|scale| * (|k| + 64) / 64 + shift
    neg = r > 0.94
    side = -torch.sign(scale).to(torch.int16)
    k = torch.where(neg, side * (k.abs() + 64).clamp_max(256), k)
    y = store(pool_unwindows(k, B, H, W).reshape(B * H * W, C).float() / 64.0, dtype)
    dskip = store(torch.randn(B * H * W, C, generator=g), dtype)
    dpool = store(torch.randn(B * H2 * W2, C, generator=g), dtype)
    dpool[dpool == 0] = 1.0  # a zero gradient would hide where the kernel put it
    mean = torch.randn(C, generator=g) * 0.2
    invstd = torch.rand(C, generator=g) + 0.5
    gap = pool_top2_gap(y, scale, shift, B, H, W)
    return {"y": y, "scale": scale, "shift": shift, "dskip": dskip, "dpool": dpool, "mean": mean, "invstd": invstd,
            "gap": gap[0], "zmax": gap[1]}
