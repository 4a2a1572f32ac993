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
