"""tests/train_kernels_ref.py against independent torch float64 machinery (F.batch_norm + autograd, nn.BatchNorm2d,
nn.Conv2d heads + the oracle's masked NLL, torch.optim.AdamW), and the conditions its input builders promise. No GPU."""

from fractions import Fraction

import numpy as np
import pytest
import torch

import train_kernels_ref as R


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("P,C", [(64, 8), (333, 24)])
def test_bn_restatement_reproduces_autograd(P, C):
    """mean / invstd / scale / shift, the (sum dz, sum dz*xhat) sums, coef[C][3] and
    dy = coef0*(dz - coef1 - xhat*coef2) against relu(F.batch_norm(train)) and torch.autograd.grad, to 1e-12."""
    g = torch.Generator().manual_seed(P)
    y = torch.randn(P, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gamma[::3] *= -1
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    da = torch.randn(P, C, generator=g, dtype=torch.float64)
    a, dy, dgamma, dbeta = R.bn_autograd(y, gamma, beta, da)
    mean, var, invstd, scale, shift = R.bn_fwd_from_sums(y.sum(0), (y * y).sum(0), P, gamma, beta)
    assert _rel(torch.relu(y * scale + shift), a) <= 1e-12
    assert _rel(mean, y.mean(0)) <= 1e-12 and _rel(var, y.var(0, unbiased=False)) <= 1e-12
    assert torch.equal(R.relu_mask(y, scale, shift), a > 0)
    dy_r, dgamma_r, dbeta_r = R.bn_bwd_restated(y, gamma, beta, da)
    assert _rel(dy_r, dy) <= 1e-12 and _rel(dgamma_r, dgamma) <= 1e-12 and _rel(dbeta_r, dbeta) <= 1e-12
    # eval mode (batch_stats = 0): the statistics are constants, dy = gamma*invstd*dz
    coef0 = R.bn_bwd_coef(dbeta_r, dgamma_r, P, gamma, invstd, batch_stats=False)
    assert torch.equal(coef0[:, 1:], torch.zeros(C, 2, dtype=torch.float64))
    ye = y.clone().requires_grad_(True)
    ae = torch.relu(torch.nn.functional.batch_norm(ye, mean.clone(), var.clone(), gamma, beta, training=False,
                                                   eps=R.EPS_BN))
    (dye,) = torch.autograd.grad(ae, ye, da)
    rm, invstd_e, scale_e, shift_e = R.bn_eval_coeffs(mean, var, gamma, beta)
    assert _rel(R.bn_bwd_apply(da, y, scale_e, shift_e, rm, invstd_e, coef0), dye) <= 1e-12


def test_bn_running_statistics_follow_nn_batchnorm2d():
    """momentum 0.1, unbiased variance, num_batches_tracked + 1, against nn.BatchNorm2d in float64 over two steps."""
    C, B, H, W = 6, 3, 5, 4
    bn = torch.nn.BatchNorm2d(C, momentum=0.1).double().train()
    g = torch.Generator().manual_seed(1)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    for step in range(2):
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2 + 1
        bn(x)
        rows = x.permute(0, 2, 3, 1).reshape(-1, C)
        n = rows.shape[0]
        mean, var, _, _, _ = R.bn_fwd_from_sums(rows.sum(0), (rows * rows).sum(0), n, bn.weight, bn.bias)
        rm, rv = R.bn_running(rm, rv, mean, var, n, 0.1)
        assert _rel(rm, bn.running_mean) <= 1e-12 and _rel(rv, bn.running_var) <= 1e-12
        assert int(bn.num_batches_tracked) == step + 1
    one = torch.ones(C, dtype=torch.float64)
    assert torch.equal(R.bn_running(rm, rv, one, one * 3, 1, 0.1)[1], 0.1 * one * 3 + 0.9 * rv)  # count == 1: biased


def _fma_sign(y, sc, sh):
    """Sign of the exact y*sc + sh (the sign a correctly rounded fp32 fma returns), by rational arithmetic."""
    out = []
    for a, b, c in zip(y, sc, sh):
        v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        out.append(v > 0)
    return torch.tensor(out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_relu_mask_is_the_sign_of_a_true_fma_and_the_planted_cases_split_the_variants(dtype):
    P, C = 40, 16
    da, y, scale, shift, _, _ = R.make_bn_bwd_inputs(P, C, dtype, seed=3)
    mask = R.relu_mask(y, scale, shift)
    exact = _fma_sign(y.float().flatten().tolist(), scale.repeat(P).tolist(), shift.repeat(P).tolist()).view(P, C)
    assert torch.equal(mask, exact)
    # row 0, even channels: z == 0 exactly, masked out (and `>= 0` would let them through)
    z0 = y[0, 0::2].double() * scale[0::2].double() + shift[0::2].double()
    assert torch.equal(z0, torch.zeros_like(z0)) and not bool(mask[0, 0::2].any())
    assert float(da[0, 0::2].float().min()) == 1.5
    # row 1, odd channels: a separate multiply and add rounds z to 0; the fma keeps the residual's sign
    split = y[1, 1::2].float() * scale[1::2] + shift[1::2]
    assert torch.equal(split, torch.zeros_like(split))
    assert int(mask[1, 1::2].sum()) >= 1, "no positive rounding residual planted: the separate-multiply variant passes"


def test_balanced_bn_input_keeps_z_away_from_zero():
    y, gamma, beta, da = R.make_balanced_bn(4096, 32, seed=5)
    assert float(beta.abs().max()) == 0.0
    assert R.bn_min_abs_z(y, gamma, beta) > 1e-3
    a, _, _, _ = R.bn_autograd(y, gamma, beta, da)
    frac = float((a > 0).double().mean())
    assert 0.45 < frac < 0.55  # balanced: both sides of the ReLU are exercised


def _heads_by_modules(inp, mode):
    """The heads as the model spells them (two 1x1 nn.Conv2d, softplus, clamp) and the oracle's masked NLL, float64."""
    from oracle.unet_ref import masked_nll

    P, C = inp["y"].shape
    act = torch.relu(inp["y"].double() * inp["scale"].double() + inp["shift"].double())
    x = act.t().reshape(1, C, 1, P).clone().requires_grad_(True)
    hd, hl = torch.nn.Conv2d(C, 1, 1).double(), torch.nn.Conv2d(C, 1, 1).double()
    with torch.no_grad():
        hd.weight.copy_(inp["wd"].double().view(1, C, 1, 1))
        hl.weight.copy_(inp["wl"].double().view(1, C, 1, 1))
        hd.bias.copy_(inp["bd"].double())
        hl.bias.copy_(inp["bl"].double())
    disp = torch.nn.functional.softplus(hd(x), beta=1.0, threshold=20.0)
    logvar = torch.clamp(hl(x), -6.0, 3.0)
    out = {"disp": disp.detach().flatten(), "logvar": logvar.detach().flatten()}
    if mode == R.LOSS:
        loss, sums = masked_nll(disp, logvar, inp["target"].view(1, 1, 1, P), inp["mask"].view(1, 1, 1, P))
        out["metrics"] = torch.tensor([sums[k] for k in ("nll", "abs", "sq", "sigma", "n")], dtype=torch.float64)
    else:
        loss = (disp.flatten() * inp["gdisp"].double()).sum() + (logvar.flatten() * inp["glogvar"].double()).sum()
    loss.backward()
    out["da"] = x.grad.reshape(C, P).t()
    out["dwd"], out["dwl"] = hd.weight.grad.flatten(), hl.weight.grad.flatten()
    out["dbd"], out["dbl"] = hd.bias.grad, hl.bias.grad
    return out


@pytest.mark.parametrize("mode", [R.LOSS, R.GRADS])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_heads_reference_matches_the_model_spelling(mode, dtype):
    inp, _ = R.make_heads_inputs(777, 16, dtype, mode, seed=2)
    ref, mod = R.heads_ref(inp, mode), _heads_by_modules(inp, mode)
    keys = ["disp", "logvar", "da", "dwd", "dwl", "dbd", "dbl"] + (["metrics"] if mode == R.LOSS else [])
    for k in keys:
        assert _rel(ref[k], mod[k]) <= 1e-12, k
    if mode == R.LOSS:
        valid = R.valid_pixels(inp["target"], inp["mask"])
        assert ref["n"] == int(valid.sum()) and 0 < ref["n"] < 777
        # the cases the issue names are in the inputs
        t, m = inp["target"], inp["mask"]
        assert bool((torch.isnan(t) & (m != 0)).any()) and bool(((t == float("inf")) & (m != 0)).any())
        assert bool(((t == float("-inf")) & (m != 0)).any()) and bool((torch.isfinite(t) & (m == 0)).any())
        assert bool((m == 2).any()) and bool((m == 255).any())
        # both clamps and the softplus threshold are reached
        assert bool((ref["xl"] < -6).any()) and bool((ref["xl"] > 3).any()) and bool((ref["xd"] > 20).any())
    # the fp32 restatement is the same formula: it differs by rounding only
    for flip in (False, True):
        f32 = R.heads_fp32(inp, mode, flip=flip)
        for k in keys:
            assert _rel(f32[k].double(), ref[k]) <= 1e-4, (k, flip)


def test_heads_reference_with_nothing_valid_is_all_zero():
    inp, _ = R.make_heads_inputs(50, 8, torch.float32, R.LOSS, seed=4, all_masked=True)
    ref = R.heads_ref(inp, R.LOSS)
    assert ref["n"] == 0 and float(ref["da"].abs().max()) == 0.0 and float(ref["metrics"].abs().max()) == 0.0
    f32 = R.heads_fp32(inp, R.LOSS)
    assert float(f32["da"].abs().max()) == 0.0 and not bool(torch.isnan(f32["da"]).any())


@pytest.mark.parametrize("case,grad_key,flows", [
    ("lv_hi", "dbl", True), ("lv_lo", "dbl", True), ("lv_above", "dbl", False), ("lv_below", "dbl", False),
    ("sp_equal", "dbd", None), ("sp_pass", "dbd", True)])
def test_heads_planted_branch_cases(case, grad_key, flows):
    inp = R.make_heads_planted(8, torch.float32, case)
    ref = R.heads_ref(inp, R.LOSS)
    if case.startswith("lv"):
        want = {"lv_hi": 3.0, "lv_lo": -6.0, "lv_above": 3.0, "lv_below": -6.0}[case]
        assert torch.equal(ref["logvar"], torch.full((2,), want, dtype=torch.float64))
        on_clamp = float(ref["xl"][0]) == want
        assert on_clamp == flows
        assert (float(ref[grad_key].abs().sum()) > 0) == flows
    else:
        assert torch.equal(ref["disp"], torch.full((2,), 25.0, dtype=torch.float64))  # above the threshold: p = x
        n, e = 2, torch.exp(-ref["logvar"])
        # pixel 1 (target 24): sign(+1) * exp(-lv) / n passes through the threshold branch unchanged
        want = e[1] / n + (e[0] / n if case == "sp_pass" else 0.0)  # pixel 0 at p == t: sign(0) = 0
        assert abs(float(ref["dbd"]) - float(want)) <= 1e-15


@pytest.mark.parametrize("C,P,mode,dtype", [
    (8, 777, R.LOSS, torch.float32), (64, 777, R.LOSS, torch.bfloat16), (16, 777, R.GRADS, torch.bfloat16),
    (32, 777, R.INFER, torch.float32), (32, 262144 + 5, R.LOSS, torch.bfloat16), (8, 3, R.LOSS, torch.float32)])
def test_heads_builder_settles_and_leaves_no_pixel_near_a_branch(C, P, mode, dtype):
    inp, rounds = R.make_heads_inputs(P, C, dtype, mode, seed=C + P)
    assert rounds <= 10
    assert int(R.heads_near_branch(inp, mode).sum()) == 0  # the share of pixels left out of a comparison is zero
    assert inp["y"].dtype == dtype and inp["y"].shape == (P, C)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("step0", [0, 1000])
def test_adamw_restatement_matches_torch_optim(wd, step0):
    """Five steps of the float64 restatement against torch.optim.AdamW(foreach=False) in float64, to 1e-12."""
    g = torch.Generator().manual_seed(7)
    n, lr, b1, b2, eps = 257, 1e-3, 0.9, 0.999, 1e-8
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    if step0:
        m, v = torch.randn(n, generator=g, dtype=torch.float64) * 0.1, torch.rand(n, generator=g, dtype=torch.float64)
        param.grad = torch.zeros_like(param)
        opt.step()  # creates the state
        with torch.no_grad():
            param.copy_(p0)
        st = opt.state[param]
        st["exp_avg"].copy_(m)
        st["exp_avg_sq"].copy_(v)
        st["step"].fill_(step0)
    p = p0.clone()
    for k in range(5):
        grad = torch.randn(n, generator=g, dtype=torch.float64)
        param.grad = grad.clone()
        opt.step()
        p, m, v = R.adamw_step(p, grad, m, v, step0 + k + 1, lr, wd, b1, b2, eps)
        st = opt.state[param]
        assert _rel(p, param.detach()) <= 1e-12 and _rel(m, st["exp_avg"]) <= 1e-12
        assert _rel(v, st["exp_avg_sq"]) <= 1e-12 and int(st["step"]) == step0 + k + 1
    # a step in fp32 arithmetic stays inside the rounding bounds the GPU test uses
    pf, mf, vf = (x.float() for x in (p, m, v))
    grad = torch.randn(n, generator=g).float()
    t = step0 + 6
    decay, step_size, bc2s = (np.float32(x) for x in R.adamw_scalars(t, lr, wd, b1, b2))
    m1 = mf + np.float32(1 - b1) * (grad - mf)
    v1 = vf * np.float32(b2) + np.float32(1 - b2) * grad * grad
    p1 = pf * decay + (-step_size) * (m1 / (torch.sqrt(v1) / bc2s + np.float32(eps)))
    pr, mr, vr = R.adamw_step(pf, grad, mf, vf, t, lr, wd, b1, b2, eps)
    tp, tm, tv = R.adamw_tolerances(pf, grad, mf, vf, t, lr, wd, b1, b2, eps)
    assert bool(((p1.double() - pr).abs() <= tp).all()) and bool(((m1.double() - mr).abs() <= tm).all())
    assert bool(((v1.double() - vr).abs() <= tv).all())


# ------------------------------------------------------------------ MaxPool2d(2) of relu(bn(y)): forward, backward
def _pool_autograd(y, scale, shift, dpool, B, H, W):
    """F.max_pool2d on relu(scale*y + shift) in float64 (NCHW) and its backward: (pooled, grad), both NHWC."""
    C = y.shape[-1]
    a = torch.relu(y.double() * scale.double() + shift.double()).reshape(B, H, W, C)
    x = a.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    p = torch.nn.functional.max_pool2d(x, 2)
    p.backward(dpool.double().reshape(B, H // 2, W // 2, C).permute(0, 3, 1, 2))
    return p.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (2, 6, 10, 24), (3, 8, 12, 32)])
def test_pool_references_reproduce_max_pool2d_autograd_on_tie_free_inputs(B, H, W, C):
    g = torch.Generator().manual_seed(H * W)
    y = torch.randn(B * H * W, C, generator=g, dtype=torch.float64) + 0.8  # fine-grained and mostly positive: no ties
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    scale[::3] *= -1
    shift = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    dskip = torch.randn(B * H * W, C, generator=g, dtype=torch.float64)
    dpool = torch.randn(B * (H // 2) * (W // 2), C, generator=g, dtype=torch.float64)
    a = R.pool_windows(torch.relu(y * scale + shift), B, H, W)
    top = a.topk(2, dim=3).values
    keep = top[:, :, :, 0] > top[:, :, :, 1]  # tie-free windows (all-zero windows of the negative channels are ties)
    assert float(keep.double().mean()) > 0.5
    pooled, grad = _pool_autograd(y, scale, shift, dpool, B, H, W)
    assert torch.equal(R.bnrelu_pool_ref(y, scale, shift, B, H, W), pooled)
    full = R.pool_unwindows(keep.unsqueeze(3).expand(-1, -1, -1, 4, -1), B, H, W)
    for skip in (dskip, None):
        da, am = R.pool_bwd_ref(y, scale, shift, skip, dpool, B, H, W)
        want = grad + (0 if skip is None else skip.reshape(B, H, W, C))
        assert torch.equal(da[full], want[full])
        assert torch.equal(R.pool_hit(am, B, H, W)[full], (grad != 0)[full])
    assert torch.equal(R.pool_unwindows(R.pool_windows(y, B, H, W), B, H, W).reshape(-1, C), y)


def test_pool_reference_first_max_on_the_planted_ties():
    """The planted cases of test_gpu_ops.test_pool_bwd_first_max_tie_break_and_skip_add: y = 0 except one 5 at window
    position 1 and one -3; scale 1, shift 0. The numpy statement (first maximum) picks position 1 in the window with
    the 5 and position 0 in every other window-channel, all of which are four-way ties at 0 after the ReLU. ATen's
    float64 CPU max_pool2d backward makes the same choice here (checked below), so the two agree on these ties too;
    the numpy statement remains the contract."""
    B, H, W, C = 1, 4, 4, 8
    y = torch.zeros(B, H, W, C, dtype=torch.float64)
    y[0, 0, 1, 0] = 5.0
    y[0, 2, 2, 1] = -3.0
    dpool = torch.arange(B * 2 * 2 * C, dtype=torch.float64) + 1
    one, zero = torch.ones(C), torch.zeros(C)
    da, am = R.pool_bwd_ref(y.reshape(-1, C), one, zero, None, dpool.reshape(-1, C), B, H, W)
    want = torch.zeros(B, 2, 2, C, dtype=torch.int64)
    want[0, 0, 0, 0] = 1
    assert torch.equal(am, want)
    _, grad = _pool_autograd(y.reshape(-1, C), one, zero, dpool.reshape(-1, C), B, H, W)
    assert torch.equal(da, grad)


POOL_SHAPES = [(1, 2, 2, 8), (2, 6, 10, 24), (3, 8, 12, 32), (1, 4, 4, 2048), (2, 16, 20, 256), (1, 128, 128, 512)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_input_builder_keeps_its_promises(shape, dtype):
    """y on the 2^-6 grid in [-4, 4] and exact in the storage type; |scale| in [0.5, 1.5], every third negative; the
    gap between the two largest relu(z) of a window is 0 or far above an fp32 rounding; with 1000 window-channels
    or more, at least 5 % tie exactly for a positive maximum and at least 5 % are all zero after the ReLU."""
    B, H, W, C = shape
    inp = R.make_pool_inputs(B, H, W, C, dtype, seed=sum(shape))
    k = inp["y"].double() * 64
    assert torch.equal(k, k.round()) and float(k.abs().max()) <= 256
    s = inp["scale"]
    assert bool((s[::3] < 0).all()) and bool((s.abs() >= 0.5).all()) and bool((s.abs() <= 1.5).all())
    assert int((s > 0).sum()) == C - len(s[::3])
    assert inp["scale"].dtype == inp["shift"].dtype == torch.float32
    assert inp["gap"] > 8 * R.U32 * inp["zmax"]
    assert inp["gap"] >= 0.5 * 2.0 ** -7 * (1 - 1e-6)  # |scale| * 2^-7 at the least
    assert not bool((inp["dpool"] == 0).any())
    ties, zeros = R.pool_tie_shares(inp["y"], s, inp["shift"], B, H, W)
    print(f"pool builder {shape} {dtype}: ties {ties:.3f} all-zero {zeros:.3f} gap {inp['gap']:.3g}")
    if B * (H // 2) * (W // 2) * C >= 1000:
        assert ties >= 0.05 and zeros >= 0.05
    # the ordering argument, checked directly: an fp32 fma (the float64 value rounded once) orders every window alike
    z64 = inp["y"].double() * s.double() + inp["shift"].double()
    a32 = R.pool_windows(torch.relu(z64.float()), B, H, W)
    a64 = R.pool_windows(torch.relu(z64), B, H, W)
    assert torch.equal(torch.from_numpy(np.argmax(a32.numpy(), 3)), torch.from_numpy(np.argmax(a64.numpy(), 3)))
    assert torch.equal(a32 == a32.max(3, keepdim=True).values, a64 == a64.max(3, keepdim=True).values)


def _emulated_pool(inp, B, H, W, dtype, skip, variant="ok"):
    """What a kernel computes, in fp32 on the CPU: z by one rounding of the exact fma, the arg-max of relu(z) (first
    maximum), one fp32 add, a round-to-nearest-even store; `variant` swaps in one defect. Returns (pooled, da)."""
    scale = inp["scale"].abs() if variant == "abs_scale" else inp["scale"]
    z = (inp["y"].double() * scale.double() + inp["shift"].double()).float()
    a = R.pool_windows(z if variant == "pre_relu" else torch.relu(z), B, H, W).numpy()
    am = 3 - np.argmax(a[:, :, :, ::-1], 3) if variant == "last_max" else np.argmax(a, 3)
    hit = R.pool_hit(torch.from_numpy(am.copy()), B, H, W).reshape(inp["y"].shape)
    C = inp["y"].shape[1]
    dp = R.pool_unwindows(inp["dpool"].float().reshape(B, H // 2, W // 2, 1, C).expand(-1, -1, -1, 4, -1), B, H, W)
    o = (inp["dskip"].float() if skip else torch.zeros(inp["y"].shape)) + torch.where(hit, dp.reshape(hit.shape),
                                                                                      torch.zeros(()))
    pooled = R.pool_windows(torch.relu(z), B, H, W).max(3).values.reshape(-1, C)
    if variant == "trunc":
        cut = lambda t: (t.view(torch.int32) & -65536).view(torch.float32).to(dtype)  # noqa: E731
        return cut(pooled.contiguous()), cut(o.contiguous())
    return pooled.to(torch.bfloat16), o.to(dtype)


@pytest.mark.parametrize("shape", [(2, 6, 10, 24), (3, 8, 12, 32)])
def test_pool_checks_pass_a_correct_kernel_and_fail_each_defect(shape):
    """The GPU tests' own check functions, run here on an fp32 emulation of the kernels: the faithful one passes every
    check; a last-max tie-break, an arg-max taken before the ReLU or on |scale|, and a truncating bf16 store fail."""
    from test_gpu_train_kernels import check_pool_bwd, check_pool_fwd

    B, H, W, C = shape
    for prec, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        inp = R.make_pool_inputs(B, H, W, C, dtype, seed=sum(shape))
        for skip in (True, False):
            pooled, da = _emulated_pool(inp, B, H, W, dtype, skip)
            check_pool_bwd("emulated", da, inp, B, H, W, prec, skip)
            for variant in ("last_max", "pre_relu", "abs_scale"):
                _, bad = _emulated_pool(inp, B, H, W, dtype, skip, variant)
                with pytest.raises(AssertionError):
                    check_pool_bwd(variant, bad, inp, B, H, W, prec, skip)
        if prec == "bf16":
            check_pool_fwd("emulated", pooled, inp, B, H, W, need_trunc_share=False)
            tp, tda = _emulated_pool(inp, B, H, W, dtype, True, "trunc")
            with pytest.raises(AssertionError):
                check_pool_fwd("trunc", tp, inp, B, H, W, need_trunc_share=False)
            with pytest.raises(AssertionError):
                check_pool_bwd("trunc", tda, inp, B, H, W, prec, True)
            _, absd = _emulated_pool(inp, B, H, W, dtype, True, "abs_scale")
            pa = R.pool_windows(torch.relu((inp["y"].double() * inp["scale"].abs().double()
                                            + inp["shift"].double()).float()), B, H, W).max(3).values.reshape(-1, C)
            with pytest.raises(AssertionError):
                check_pool_fwd("abs_scale", pa.to(torch.bfloat16), inp, B, H, W, need_trunc_share=False)
