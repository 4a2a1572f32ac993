"""The training step's small kernels through the C ABI against the float64 statements of tests/train_kernels_ref.py
(needs an MI355X): the BatchNorm finalizes, reduces and apply (csrc/bn.hip), the fused heads + loss + gradient
(csrc/heads.hip), AdamW and the valid count (csrc/misc.hip), the MaxPool2d forward sd_bnrelu_pool (csrc/conv_fast.hip)
and backward + skip add + fused BatchNorm-backward sums sd_pool_bwd_add (csrc/bn.hip).

Tolerances (u = 2^-24; none is fitted to the kernels' output):
  exact     counts, step, scratch, num_batches_tracked, the single-rank bit identities, zeros the contract promises;
  formula   fp32 outputs of a short fixed formula: k * u * (sum of |terms|), k and the terms next to each assert;
            fp64 accumulations add (adds) * 2^-53 * (sum of |terms|);
  bf16      stored outputs must be the round-to-nearest-even bf16 of an fp32 value inside the fp32 bound: between
            RNE(ref - tol) and RNE(ref + tol), nothing added for the store (where tol is far below the bf16 spacing
            the bits are pinned). A flat 2^-9 * |value| cannot serve: bf16 has 8 significant bits, so a correct
            round-to-nearest store errs by up to 2^-8 * |x| just above a power of two (2^-9 * |x| only just below
            one); the kernels' stores measured up to 1.99 * 2^-9 * |ref| and never above half a bf16 ulp. The
            reference truncated to bf16 fails the check on more than a quarter of the elements (asserted);
  sums      fp32 sums over pixels: (n + m + 2) * u * sum |term|, n the sequential adds of a thread, m the adds of the
            in-block reduction, sum |term| in float64 from the reference;
  expf      per-pixel values through expf / log1pf (disp, the loss gradient, the metric terms): 8 x the deviation of
            the torch fp32 CPU restatement (train_kernels_ref.heads_fp32, both channel orders) from float64 on the
            same inputs (the largest over the output), exactly that at P >= 64. With P = 1, 2 or 3 pixels the
            measurement is a sample of a handful of values and can be 0 (a clamped logvar, a correctly rounded sum)
            while another order of the same sum is one rounding off, so there a deviation below ONE fp32 rounding of
            the element's own inputs is raised to it: u * s, with s the element's condition in float64 from the
            reference: disp: s_d = sum |act*wd| + |bd|; logvar: s_l = sum |act*wl| + |bl|; a gradient or metric
            term g: |g| * (2 + s_d + s_l) (exp(-lv) turns lv's absolute error into a relative one), summed for the
            sums. Sums of such values add the `sums` bound.
  pooling   the inputs sit on a 2^-6 grid whose windows an fp32 fma and float64 order alike
            (train_kernels_ref.make_pool_inputs; the gap between a window's two largest values is 0 or above
            8 * u * max|z|, asserted), so the winner is the reference's in every window: forward = the bf16 interval of
            one fma rounding (u * |ref|); backward = dskip bit for bit off the arg-max (exactly 0 without dskip), one
            fp32 add (u * |ref|) at it, exactly dpool without dskip; fused sums = the `sums` rule with n = 4 adds per
            loop trip and m = 256/(C/8), evaluated on the da the kernel stored, + 3 roundings for dz*xhat.
            tests/test_train_kernels_ref_cpu.py runs these checks on an fp32 emulation: a last-max tie-break, an
            arg-max before the ReLU or on |scale| and a truncating store each fail them.

Measured on an MI355X (every test prints its figures; run with -s): the fp32 CPU restatement's deviation from float64
where the rule uses one (smallest .. largest over the cases with P >= 64), and the largest device deviation as a
fraction of the allowed one over all cases of the test. bf16 stored outputs reach 1.0 of (half a bf16 ulp + the fp32
bound) by construction (a value next to a rounding tie); their check is the interval, which they all meet.

  test / output                          fp32-CPU deviation       largest device deviation / allowed
  bn_fwd_finalize mean, invstd           -                        0.97, 0.97   (k = 1: one rounding)
  bn_fwd_finalize scale, shift           -                        0.90, 0.48
  bn_fwd_finalize running mean, var      -                        0.48, 0.49
  bn_eval_coeffs invstd, scale, shift    -                        0.53, 0.51, 0.35   (mean: exact)
  bn_rows_sum64                          -                        0 (equal to math.fsum); finalize64: bit-identical
  bn_bwd_finalize64 dgamma, dbeta, coef0 -                        0.84, 0.77, 0.73
  bn_bwd_finalize dgamma, dbeta, coef    -                        0.99, 0.93, 0.97   (k = 1)
  bn_bwd_reduce sum dz, sum dz*xhat      -                        0.16, 0.54
  chan_sum                               -                        0.19
  bn_bwd_apply fp32 / bf16               -                        0.46 / interval met
  bn chain dy, dgamma, dbeta             -                        0.066, 0.0010, 0.00077
  heads disp                             1.3e-06 .. 3.7e-06       0.21
  heads logvar                           5.6e-07 .. 1.9e-06       0.29
  heads da fp32 / bf16                   2.3e-08 .. 1.6e-05       0.19 / interval met
  heads dwd, dwl                         4.1e-07 .. 3.7e-05       0.086, 0.11
  heads dbd, dbl                         1.7e-08 .. 2.4e-05       0.072, 0.087
  heads metrics (sums; once and twice)   3.2e-04 .. 5.6           0.051
  heads_bnsum sum dz, sum dz*xhat        (from da's)              0.081, 0.081   (other outputs as sd_heads)
  count_valid                            -                        exact
  adamw p, m, v                          -                        0.19, 0.67, 0.59
  bnrelu_pool (bf16)                     -                        interval met (1.0 of half a bf16 ulp), all bits pinned
  pool_bwd_add da fp32 / bf16            -                        1.0 (an add that rounds by half an ulp of a power of
                                                                  two) / interval met; without dskip: exact
  pool_bwd_add sum dz, sum dz*xhat       (from the stored da)     fp32 0.17, 0.20; bf16 0.0026, 0.25
  pool_bwd_add past one sweep (bf16)     -                        768 rows x 256 < 262144 items at (1,128,128,512):
                                                                  da interval met; sums 0.00011, 0.0038
  pool forward / backward winner         -                        interval met, all bits pinned
"""

import math

import numpy as np
import pytest
import torch

import train_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32, U64, UBF16 = R.U32, R.U64, R.UBF16
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def L():
    from stereo_depth_estimation_amd import _lib

    return _lib


def _sd(prec):
    return L().SD_F32 if prec == "fp32" else L().SD_BF16


def _d(t):
    return None if t is None else t.data_ptr()


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (tol == 0: exact), nothing NaN; prints the largest deviation / allowed."""
    got, ref = got.detach().double().cpu(), R.f64(ref)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), name
    dev = (got - ref).abs()
    ratio = float(torch.where(dev == 0, torch.zeros_like(dev), dev / tol.clamp_min(1e-300)).max()) if dev.numel() else 0.0
    print(f"RATIO {name} dev/allowed={ratio:.3g} maxdev={float(dev.max()):.3g}")
    bad = dev > tol
    assert not bool(bad.any()), (name, ratio, int(bad.sum()), float(dev.max()))
    return ratio


def _check_bf16(name, got, ref, tol32):
    """A bf16 output must be the round-to-nearest-even of an fp32 value within tol32 of ref
    (train_kernels_ref.bf16_store_interval): nothing is allowed for the store itself."""
    got, ref = got.detach().double().cpu(), R.f64(ref)
    assert not bool(torch.isnan(got).any()), name
    lo, hi = R.bf16_store_interval(ref, tol32)
    half_ulp = torch.where(ref == 0, torch.zeros_like(ref), torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-300))) - 8))
    dev = (got - ref).abs()
    ratio = float((dev / (half_ulp + tol32).clamp_min(1e-300)).max())
    print(f"RATIO {name} dev/(half ulp + allowed)={ratio:.3g} pinned={float((lo == hi).double().mean()):.3f}")
    bad = (got < lo) | (got > hi)
    assert not bool(bad.any()), (name, ratio, int(bad.sum()))
    return ratio


# ------------------------------------------------------------------ 1. sd_bn_fwd_finalize, sd_bn_eval_coeffs
def _make_stat_rows(rows, C, npix, seed):
    """fp32 (sum, sumsq) rows of `npix` pixels each, channel 0 built so that sumsq/count falls just below mean^2."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(C, generator=g) * 2.0
    sd = torch.rand(C, generator=g) + 0.3
    x = m + sd * torch.randn(rows, npix, C, generator=g)
    stats = torch.stack([x.double().sum(1).float(), (x.double() ** 2).sum(1).float()], 2)  # [rows][C][2]
    count = rows * npix
    stats[:, 0, :] = 0.0
    stats[0, 0, 0] = 2.0 * count  # mean = 2 exactly
    stats[0, 0, 1] = float(np.nextafter(np.float32(4.0 * count), np.float32(0)))  # sumsq/count < 4 = mean^2
    return stats.contiguous(), count


def _fwd_tolerances(stats, count, gamma, beta, rm, rv, momentum):
    """mean   = (float)mean64:                 k = 1 on |mean|
    invstd = (float)(1/sqrt(var + eps)):       k = 1 on |invstd|
    scale  = gamma*invstd:                     k = 2 on |scale| (invstd's rounding, the multiply)
    shift  = beta - (float)mean*scale:         k = 5 on |beta| + |mean*scale| (mean, scale's 2, multiply, subtract)
    running = (float)(mom*stat + (1-mom)*run): k = 2 on mom*|stat| + (1-mom)*|run| (the result; fp32 momentum's 1-mom)
    plus the fp64 accumulation of the rows ((rows + 8) adds) carried through each formula to first order."""
    s, ss = stats[:, :, 0].double(), stats[:, :, 1].double()
    rows = stats.shape[0]
    mean, var, invstd, scale, shift = R.bn_fwd_from_sums(s.sum(0), ss.sum(0), count, gamma, beta)
    e_mean = U64 * (rows + 8) * s.abs().sum(0) / count
    e_var = U64 * (rows + 8) * (ss.abs().sum(0) / count + 2 * mean * mean) + 2 * mean.abs() * e_mean
    r_is = 0.5 * e_var / (var + R.EPS_BN)
    ms = (mean * scale).abs()
    tol = {"mean": U32 * mean.abs() + e_mean, "invstd": invstd * (U32 + r_is), "scale": scale.abs() * (2 * U32 + r_is),
           "shift": 5 * U32 * (beta.double().abs() + ms) + ms * r_is + scale.abs() * e_mean}
    ref = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift}
    if rm is not None:
        ref["rm"], ref["rv"] = R.bn_running(rm, rv, mean, var, count, momentum)
        unb = var * count / (count - 1.0) if count > 1 else var
        tol["rm"] = 2 * U32 * (momentum * mean.abs() + (1 - momentum) * rm.double().abs()) + e_mean
        tol["rv"] = 2 * U32 * (momentum * unb + (1 - momentum) * rv.double().abs()) + 2 * e_var
    return ref, tol


@pytest.mark.parametrize("C", [8, 24, 512])
@pytest.mark.parametrize("rows", [1, 255, 257, 1000])
def test_bn_fwd_finalize(rows, C):
    lib, s = L(), L().stream_handle()
    stats, count = _make_stat_rows(rows, C, 3, seed=rows + C)
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    gamma[::3] *= -1
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ref, tol = _fwd_tolerances(stats, count, gamma, beta, rm0, rv0, R.MOMENTUM)
    assert float(ref["invstd"][0]) == 1.0 / math.sqrt(R.EPS_BN)  # channel 0 reaches the clamp to var = 0
    st, gm, bt, rm, rv = _dev(stats, gamma, beta, rm0, rv0)
    nbt = torch.tensor([7], dtype=torch.int64, device=DEV)
    out = torch.full((4, C), float("nan"), device=DEV)
    lib.call("sd_bn_fwd_finalize", _d(st), rows, C, float(count), _d(gm), _d(bt), _d(rm), _d(rv), _d(nbt), R.MOMENTUM,
             R.EPS_BN, _d(out[0]), _d(out[1]), _d(out[2]), _d(out[3]), s)
    torch.cuda.synchronize()
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        _check(f"fwd_finalize[{rows},{C}].{k}", out[i], ref[k], tol[k])
    _check(f"fwd_finalize[{rows},{C}].running_mean", rm, ref["rm"], tol["rm"])
    _check(f"fwd_finalize[{rows},{C}].running_var", rv, ref["rv"], tol["rv"])
    assert int(nbt) == 8  # advanced by exactly 1, not by C
    # NULL running pointers: the same coefficients, nothing else touched
    out2 = torch.full((4, C), float("nan"), device=DEV)
    rm_before, rv_before = rm.clone(), rv.clone()
    lib.call("sd_bn_fwd_finalize", _d(st), rows, C, float(count), _d(gm), _d(bt), None, None, None, R.MOMENTUM,
             R.EPS_BN, _d(out2[0]), _d(out2[1]), _d(out2[2]), _d(out2[3]), s)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(rm, rm_before) and torch.equal(rv, rv_before) and int(nbt) == 8


def test_bn_fwd_finalize_count_one_uses_the_biased_variance():
    lib, s = L(), L().stream_handle()
    C = 8
    g = torch.Generator().manual_seed(2)
    x = torch.randn(C, generator=g)
    stats = torch.stack([x, (x.double() ** 2).float()], 1).view(1, C, 2).contiguous()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ref, tol = _fwd_tolerances(stats, 1, gamma, beta, rm0, rv0, R.MOMENTUM)
    st, gm, bt, rm, rv = _dev(stats, gamma, beta, rm0, rv0)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((4, C), float("nan"), device=DEV)
    lib.call("sd_bn_fwd_finalize", _d(st), 1, C, 1.0, _d(gm), _d(bt), _d(rm), _d(rv), _d(nbt), R.MOMENTUM, R.EPS_BN,
             _d(out[0]), _d(out[1]), _d(out[2]), _d(out[3]), s)
    torch.cuda.synchronize()
    for i, k in enumerate(("mean", "invstd", "scale", "shift")):
        _check(f"fwd_finalize[count=1].{k}", out[i], ref[k], tol[k])
    _check("fwd_finalize[count=1].running_var", rv, ref["rv"], tol["rv"])
    _check("fwd_finalize[count=1].running_mean", rm, ref["rm"], tol["rm"])
    assert int(nbt) == 1


@pytest.mark.parametrize("C", [8, 264, 512])
def test_bn_eval_coeffs(C):
    lib, s = L(), L().stream_handle()
    g = torch.Generator().manual_seed(C)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) * 2 + 1e-3
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    mean, invstd, scale, shift = R.bn_eval_coeffs(rm, rv, gamma, beta)
    out = torch.full((4, C), float("nan"), device=DEV)
    keep = _dev(rm, rv, gamma, beta)
    lib.call("sd_bn_eval_coeffs", *[_d(t) for t in keep], C, R.EPS_BN, _d(out[0]), _d(out[1]), _d(out[2]), _d(out[3]), s)
    torch.cuda.synchronize()
    _check(f"eval_coeffs[{C}].mean", out[0], mean, 0.0)  # a copy
    # invstd = 1/sqrtf(rv + eps): k = 3 (eps as fp32 and the add, the root halving both, the divide)
    _check(f"eval_coeffs[{C}].invstd", out[1], invstd, 3 * U32 * invstd)
    _check(f"eval_coeffs[{C}].scale", out[2], scale, 4 * U32 * scale.abs())  # k = 4: invstd's 3, the multiply
    # shift = beta - rm*scale: k = 6 on |beta| + |rm*scale| (scale's 4, the multiply, the subtract)
    _check(f"eval_coeffs[{C}].shift", out[3], shift, 6 * U32 * (beta.double().abs() + (mean * scale).abs()))


# ------------------------------------------------------------------ 2. the fp64 SyncBatchNorm forms
@pytest.mark.parametrize("rows,C", [(1, 8), (257, 24), (1000, 8)])
def test_bn_rows_sum64_and_finalize64(rows, C):
    lib, s = L(), L().stream_handle()
    stats, count = _make_stat_rows(rows, C, 3, seed=rows)
    g = torch.Generator().manual_seed(3)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    st, gm, bt = _dev(stats, gamma, beta)
    sums = torch.full((2 * C + 1,), float("nan"), dtype=torch.float64, device=DEV)
    lib.call("sd_bn_rows_sum64", _d(st), rows, C, float(count), _d(sums), s)
    torch.cuda.synchronize()
    assert float(sums[2 * C]) == float(count)
    # channel sums against math.fsum of the rows, to float64 rounding: ceil(rows/256) + 8 adds per value
    flat = stats.double().view(rows, 2 * C)
    exact = torch.tensor([math.fsum(flat[:, j].tolist()) for j in range(2 * C)], dtype=torch.float64)
    _check(f"rows_sum64[{rows},{C}]", sums[:2 * C], exact, (rows // 256 + 9) * U64 * flat.abs().sum(0))
    # single rank: finalize64 of these sums == the fp32-row finalize, bit for bit, forward ...
    outs = []
    for use64 in (False, True):
        rm, rv = _dev(rm0, rv0)
        nbt = torch.tensor([3], dtype=torch.int64, device=DEV)
        o = torch.full((4, C), float("nan"), device=DEV)
        tail = (_d(gm), _d(bt), _d(rm), _d(rv), _d(nbt), R.MOMENTUM, R.EPS_BN, _d(o[0]), _d(o[1]), _d(o[2]), _d(o[3]), s)
        if use64:
            lib.call("sd_bn_fwd_finalize64", _d(sums), C, *tail)
        else:
            lib.call("sd_bn_fwd_finalize", _d(st), rows, C, float(count), *tail)
        torch.cuda.synchronize()
        assert int(nbt) == 4
        outs.append((o, rm, rv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # ... and backward (the same rows read as BatchNorm-backward partials)
    invstd = outs[0][0][1].contiguous()
    bw = []
    for use64 in (False, True):
        o = torch.full((2, C), float("nan"), device=DEV)
        coef = torch.full((C, 3), float("nan"), device=DEV)
        if use64:
            lib.call("sd_bn_bwd_finalize64", _d(sums), _d(sums), C, _d(gm), _d(invstd), 1, _d(o[0]), _d(o[1]), _d(coef), s)
        else:
            lib.call("sd_bn_bwd_finalize", _d(st), rows, C, float(count), _d(gm), _d(invstd), 1, _d(o[0]), _d(o[1]),
                     _d(coef), s)
        torch.cuda.synchronize()
        bw.append((o, coef))
    assert torch.equal(bw[0][0], bw[1][0]) and torch.equal(bw[0][1], bw[1][1])


def test_bn_bwd_finalize64_local_and_global_sums():
    """dgamma/dbeta come from the local sums, coef from the global sums and the global count; batch_stats = 0
    gives coef = {gamma*invstd, 0, 0}."""
    lib, s = L(), L().stream_handle()
    C = 24
    g = torch.Generator().manual_seed(4)
    local = torch.randn(2 * C + 1, generator=g, dtype=torch.float64) * 50
    glob = torch.randn(2 * C + 1, generator=g, dtype=torch.float64) * 200
    local[2 * C], glob[2 * C] = 1000.0, 4096.0
    gamma, invstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    lo, gl, gm, iv = _dev(local, glob, gamma, invstd)
    k0 = gamma.double() * invstd.double()
    for batch_stats in (1, 0):
        o = torch.full((2, C), float("nan"), device=DEV)
        coef = torch.full((C, 3), float("nan"), device=DEV)
        lib.call("sd_bn_bwd_finalize64", _d(lo), _d(gl), C, _d(gm), _d(iv), batch_stats, _d(o[0]), _d(o[1]), _d(coef), s)
        torch.cuda.synchronize()
        ref = R.bn_bwd_coef(glob[0:2 * C:2], glob[1:2 * C:2], 4096.0, gamma, invstd, bool(batch_stats))
        # each a single fp32 rounding of a float64 value (k = 1; the fp64 divide adds 2^-53)
        _check(f"bwd_finalize64[{batch_stats}].dgamma", o[0], local[1:2 * C:2], U32 * local[1:2 * C:2].abs())
        _check(f"bwd_finalize64[{batch_stats}].dbeta", o[1], local[0:2 * C:2], U32 * local[0:2 * C:2].abs())
        _check(f"bwd_finalize64[{batch_stats}].coef0", coef[:, 0], k0, U32 * k0.abs())
        if batch_stats:
            _check("bwd_finalize64.coef12", coef[:, 1:], ref[:, 1:], (U32 + 2 * U64) * ref[:, 1:].abs())
        else:
            assert torch.equal(coef[:, 1:].cpu(), torch.zeros(C, 2))


# ------------------------------------------------------------------ 3. sd_bn_bwd_reduce, sd_chan_sum
def _ppi(C):
    return 256 // (C // 8)


def _reduce_cases():
    out = []
    for C in (8, 24, 32, 512, 2048):
        for P in sorted({1, max(1, _ppi(C) - 1), 777}):
            out += [(C, P, "fp32"), (C, P, "bf16")]
    # grid-stride: more pixels than 1024 rows take in one sweep
    return out + [(32, 3 * 65536 + 19, "fp32"), (32, 3 * 65536 + 19, "bf16"), (2048, 1500, "fp32"), (2048, 1500, "bf16")]


def _sum_adds(lib, P, C):
    """(n, m, rows) of k_chan_reduce: n sequential adds per thread, m = ppi adds of the block's row sum."""
    rows = lib.call("sd_chan_reduce_rows", P, C)
    assert rows == min(1024, -(-P // _ppi(C)))
    return -(-P // (rows * _ppi(C))), _ppi(C), rows


@pytest.mark.parametrize("C,P,prec", _reduce_cases())
def test_bn_bwd_reduce_and_chan_sum(C, P, prec):
    lib, s = L(), L().stream_handle()
    da, y, scale, shift, mean, invstd = R.make_bn_bwd_inputs(P, C, DTYPES[prec], seed=C + P)
    s1, s2, a1, a2 = R.bn_bwd_sums(da, y, scale, shift, mean, invstd)
    n, m, rows = _sum_adds(lib, P, C)
    if P > 1024 * _ppi(C):
        assert n >= 2  # the grid-stride loop runs again
    dda, dy_, sc, sh, mu, iv = _dev(da, y, scale, shift, mean, invstd)
    part = torch.full((rows, C, 2), float("nan"), device=DEV)
    lib.call("sd_bn_bwd_reduce", _sd(prec), _d(dda), _d(dy_), _d(sc), _d(sh), _d(mu), _d(iv), P, C, _d(part), s)
    torch.cuda.synchronize()
    got = part.double().sum(0).cpu()
    # z == 0 exactly (row 0, even channels: da = 1.5 there) must be masked out; the residual cases follow the fma
    _check(f"bwd_reduce[{C},{P},{prec}].sum_dz", got[:, 0], s1, (n + m + 2) * U32 * a1)
    _check(f"bwd_reduce[{C},{P},{prec}].sum_dz_xhat", got[:, 1], s2, (n + m + 2) * U32 * a2)
    part2 = torch.full((rows, C, 2), float("nan"), device=DEV)
    out = torch.full((C,), float("nan"), device=DEV)
    lib.call("sd_chan_sum", _sd(prec), _d(dda), P, C, _d(part2), _d(out), s)
    torch.cuda.synchronize()
    ref = da.double().sum(0)
    # + 1: the fp64 row sum is rounded to fp32 once
    _check(f"chan_sum[{C},{P},{prec}]", out, ref, (n + m + 2) * U32 * da.double().abs().sum(0) + U32 * ref.abs())


# ------------------------------------------------------------------ 4. sd_bn_bwd_finalize, sd_bn_bwd_apply
@pytest.mark.parametrize("rows,C", [(1, 8), (255, 24), (257, 512), (1000, 32)])
@pytest.mark.parametrize("batch_stats", [1, 0])
def test_bn_bwd_finalize(rows, C, batch_stats):
    lib, s = L(), L().stream_handle()
    g = torch.Generator().manual_seed(rows)
    part = torch.randn(rows, C, 2, generator=g)
    gamma, invstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    count = 37.0 * rows
    pt, gm, iv = _dev(part, gamma, invstd)
    o = torch.full((2, C), float("nan"), device=DEV)
    coef = torch.full((C, 3), float("nan"), device=DEV)
    lib.call("sd_bn_bwd_finalize", _d(pt), rows, C, count, _d(gm), _d(iv), batch_stats, _d(o[0]), _d(o[1]), _d(coef), s)
    torch.cuda.synchronize()
    p64 = part.double()
    s1, s2 = p64[:, :, 0].sum(0), p64[:, :, 1].sum(0)
    e1, e2 = (U64 * (rows + 8) * p64[:, :, i].abs().sum(0) for i in (0, 1))  # the fp64 accumulation
    ref = R.bn_bwd_coef(s1, s2, count, gamma, invstd, bool(batch_stats))
    # every output is one fp32 rounding (k = 1) of a float64 value, coef0 one fp32 multiply (k = 1)
    _check(f"bwd_finalize[{rows},{C}].dbeta", o[1], s1, U32 * s1.abs() + e1)
    _check(f"bwd_finalize[{rows},{C}].dgamma", o[0], s2, U32 * s2.abs() + e2)
    _check(f"bwd_finalize[{rows},{C}].coef0", coef[:, 0], ref[:, 0], U32 * ref[:, 0].abs())
    if batch_stats:
        _check(f"bwd_finalize[{rows},{C}].coef1", coef[:, 1], ref[:, 1], U32 * ref[:, 1].abs() + e1 / count)
        _check(f"bwd_finalize[{rows},{C}].coef2", coef[:, 2], ref[:, 2], U32 * ref[:, 2].abs() + e2 / count)
    else:
        assert torch.equal(coef[:, 1:].cpu(), torch.zeros(C, 2))


def _apply_tolerance(da, y, scale, shift, mean, invstd, coef, prec):
    """dy = k0*(dz - k1 - xhat*k2), xhat = (y - mean)*invstd: k = 6 fp32 operations (subtract, multiply, multiply,
    subtract, subtract, multiply) on the terms |k0|*(|dz| + |k1| + |xhat*k2|)."""
    c = coef.double()
    dz = torch.where(R.relu_mask(y, scale, shift), da.double(), torch.zeros((), dtype=torch.float64))
    xh = (y.double() - mean.double()) * invstd.double()
    tol = 6 * U32 * c[:, 0].abs() * (dz.abs() + c[:, 1].abs() + (xh * c[:, 2]).abs())
    return R.bn_bwd_apply(da, y, scale, shift, mean, invstd, coef), tol


def _apply_cases():
    out = [(C, P, prec) for C in (8, 24, 32, 512, 2048) for P in (1, 300) for prec in ("fp32", "bf16")]
    return out + [(32, 8192 * 64 + 77, "bf16")]  # past one sweep of the 8192-block grid


@pytest.mark.parametrize("C,P,prec", _apply_cases())
def test_bn_bwd_apply(C, P, prec):
    lib, s = L(), L().stream_handle()
    da, y, scale, shift, mean, invstd = R.make_bn_bwd_inputs(P, C, DTYPES[prec], seed=2 * C + P)
    s1, s2, _, _ = R.bn_bwd_sums(da, y, scale, shift, mean, invstd)
    coef = R.bn_bwd_coef(s1, s2, P, scale.sign() * 0.8, invstd).float()
    ref, tol = _apply_tolerance(da, y, scale, shift, mean, invstd, coef, prec)
    keep = _dev(da, y, scale, shift, mean, invstd, coef)
    dy = torch.full((P, C), float("nan"), dtype=DTYPES[prec], device=DEV)
    lib.call("sd_bn_bwd_apply", _sd(prec), *[_d(t) for t in keep], P, C, _d(dy), s)
    torch.cuda.synchronize()
    if prec == "fp32":
        _check(f"bwd_apply[{C},{P},{prec}]", dy, ref, tol)
        return
    _check_bf16(f"bwd_apply[{C},{P},{prec}]", dy, ref, tol)  # the round-to-nearest-even of the fp32 value
    if P == 300:
        # the check tells round-to-nearest from truncation: the reference truncated to bf16 is outside it
        trunc = (ref.float().view(torch.int32) & -65536).view(torch.float32).double()
        lo, hi = R.bf16_store_interval(ref, tol)
        assert float(((trunc < lo) | (trunc > hi)).double().mean()) > 0.25


# ------------------------------------------------------------------ 5. the BatchNorm chain, end to end
def test_bn_chain_matches_autograd():
    """fp32 (sum, sumsq) rows of 64-pixel blocks -> sd_bn_fwd_finalize -> sd_bn_bwd_reduce -> sd_bn_bwd_finalize ->
    sd_bn_bwd_apply against autograd float64 dy, dgamma, dbeta, on the balanced input whose ReLU mask does not depend
    on the precision of the statistics. The bound carries each stage's rounding bound through the next stage to
    first order (products of two 2^-24 terms are dropped; the factor 2 at the end covers them)."""
    lib, s = L(), L().stream_handle()
    P, C, blk = 4096, 32, 64
    y, gamma, beta, da = R.make_balanced_bn(P, C, seed=5)
    _, dy_ref, dgamma_ref, dbeta_ref = R.bn_autograd(y, gamma, beta, da)
    y64 = y.double()
    rows = P // blk
    yb = y64.view(rows, blk, C)
    stats = torch.stack([yb.sum(1).float(), (yb * yb).sum(1).float()], 2).contiguous()
    st, gm, bt, dy_in, dda = _dev(stats, gamma, beta, y, da)
    coefs = torch.full((4, C), float("nan"), device=DEV)
    lib.call("sd_bn_fwd_finalize", _d(st), rows, C, float(P), _d(gm), _d(bt), None, None, None, R.MOMENTUM, R.EPS_BN,
             _d(coefs[0]), _d(coefs[1]), _d(coefs[2]), _d(coefs[3]), s)
    mean_d, invstd_d, scale_d, shift_d = (coefs[i] for i in range(4))
    rr = lib.call("sd_chan_reduce_rows", P, C)
    part = torch.full((rr, C, 2), float("nan"), device=DEV)
    lib.call("sd_bn_bwd_reduce", L().SD_F32, _d(dda), _d(dy_in), _d(scale_d), _d(shift_d), _d(mean_d), _d(invstd_d), P, C,
             _d(part), s)
    grads = torch.full((2, C), float("nan"), device=DEV)
    coef = torch.full((C, 3), float("nan"), device=DEV)
    lib.call("sd_bn_bwd_finalize", _d(part), rr, C, float(P), _d(gm), _d(invstd_d), 1, _d(grads[0]), _d(grads[1]),
             _d(coef), s)
    dy = torch.full((P, C), float("nan"), device=DEV)
    lib.call("sd_bn_bwd_apply", L().SD_F32, _d(dda), _d(dy_in), _d(scale_d), _d(shift_d), _d(mean_d), _d(invstd_d),
             _d(coef), P, C, _d(dy), s)
    torch.cuda.synchronize()
    # float64 quantities of the exact computation
    mean, var, invstd, scale, shift = R.bn_fwd_from_sums(y64.sum(0), (y64 * y64).sum(0), P, gamma, beta)
    xh = (y64 - mean) * invstd
    dz = torch.where(R.relu_mask(y, scale, shift), da.double(), torch.zeros((), dtype=torch.float64))
    s1, s2 = dz.sum(0), (dz * xh).sum(0)
    k0, k1, k2 = scale, s1 / P, s2 / P
    # forward: each row sum carries one fp32 rounding; mean and invstd one more
    d_mean = U32 * stats[:, :, 0].double().abs().sum(0) / P + U32 * mean.abs()
    d_var = U32 * stats[:, :, 1].double().sum(0) / P + 2 * mean.abs() * d_mean
    r_is = 0.5 * d_var / (var + R.EPS_BN) + U32
    r_sc = r_is + U32
    d_shift = scale.abs() * d_mean + (mean * scale).abs() * (r_sc + 2 * U32)
    d_z = y64.abs() * scale.abs() * r_sc + d_shift + U32 * (y64 * scale + shift).abs()
    assert float(d_z.max()) < 1e-3 < float((y64 * scale + shift).abs().min())  # the device's mask is the reference's
    d_xh = xh.abs() * (r_is + 2 * U32) + invstd * d_mean
    n, m = -(-P // (rr * _ppi(C))), _ppi(C)
    t_s1 = (n + m + 2) * U32 * dz.abs().sum(0)
    t_s2 = (dz.abs() * d_xh).sum(0) + (n + m + 2) * U32 * (dz * xh).abs().sum(0)
    _check("chain.dbeta", grads[1], dbeta_ref, 2 * (t_s1 + U32 * s1.abs()))
    _check("chain.dgamma", grads[0], dgamma_ref, 2 * (t_s2 + U32 * s2.abs()))
    d_k1, d_k2 = t_s1 / P + U32 * k1.abs(), t_s2 / P + U32 * k2.abs()
    t_dy = (r_is + U32) * dy_ref.abs() + k0.abs() * (d_k1 + d_xh * k2.abs() + xh.abs() * d_k2) \
        + 6 * U32 * k0.abs() * (dz.abs() + k1.abs() + (xh * k2).abs())
    _check("chain.dy", dy, dy_ref, 2 * t_dy)


# ------------------------------------------------------------------ 6. sd_heads, sd_heads_bnsum
_HEADS_REF = {}


def _heads_case(C, P, prec, mode, all_masked=False, planted=None):
    """Inputs, the float64 reference and the per-output allowed deviation (module docstring, `expf`), computed once
    per case and shared between sd_heads and sd_heads_bnsum."""
    key = (C, P, prec, mode, all_masked, planted)
    if key in _HEADS_REF:
        return _HEADS_REF[key]
    if planted:
        inp = R.make_heads_planted(C, DTYPES[prec], planted)
    else:
        inp, _ = R.make_heads_inputs(P, C, DTYPES[prec], mode, seed=1000 * mode + C + P, all_masked=all_masked)
    ref = R.heads_ref(inp, mode)
    f32 = [R.heads_fp32(inp, mode, flip=f) for f in (False, True)]
    keys = ["disp", "logvar"] + ([] if mode == R.INFER else ["da", "dwd", "dwl", "dbd", "dbl"]) \
        + (["metrics"] if mode == R.LOSS else [])
    allowed, dev32 = {}, {}
    scale = {"disp": ref["s_d"], "logvar": ref["s_l"]}  # what one fp32 rounding upstream moves each value by, / u
    if mode != R.INFER:
        kpx = 2.0 + ref["s_d"] + ref["s_l"]
        gd, gl = ref["gxd"].abs() * kpx, ref["gxl"].abs() * kpx
        scale.update({"da": ref["da"].abs() * kpx[:, None], "dwd": gd @ ref["act"], "dwl": gl @ ref["act"],
                      "dbd": gd.sum().reshape(1), "dbl": gl.sum().reshape(1)})
    if mode == R.LOSS:
        scale["metrics"] = ref["metric_scale"]
    for k in keys:
        dev32[k] = max(float((f[k].double() - ref[k]).abs().max()) for f in f32)
        guard = U32 * scale[k] if P < 64 else torch.zeros_like(scale[k])  # a handful of pixels: see the docstring
        allowed[k] = 8 * torch.clamp(guard, min=dev32[k])
    out = (inp, ref, allowed, dev32)
    if P <= 1024:
        _HEADS_REF[key] = out
    return out


def _run_heads(inp, C, P, prec, mode, bnsum, null_outputs=False):
    lib, s = L(), L().stream_handle()
    rows = lib.call("sd_heads_rows", P)
    NV = 2 * C + 7
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    n = int(R.valid_pixels(inp["target"], inp["mask"]).sum()) if mode == R.LOSS else 0
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    disp = None if null_outputs else torch.full((P,), float("nan"), device=DEV)
    logvar = None if null_outputs else torch.full((P,), float("nan"), device=DEV)
    da = None if (null_outputs or mode == R.INFER) else torch.full((P, C), float("nan"), dtype=DTYPES[prec], device=DEV)
    part = None if mode == R.INFER else torch.full((rows, NV), float("nan"), device=DEV)
    args = (_sd(prec), mode, _d(d["y"]), _d(d["scale"]), _d(d["shift"]), P, C, _d(d["wd"]), _d(d["bd"]), _d(d["wl"]),
            _d(d["bl"]), _d(disp), _d(logvar), _d(d.get("target")), _d(d.get("mask")),
            _d(count) if mode == R.LOSS else None, _d(d.get("gdisp")), _d(d.get("glogvar")), _d(da), _d(part))
    out = {"disp": disp, "logvar": logvar, "da": da, "part": part, "rows": rows, "count": count}
    if bnsum:
        g = torch.Generator().manual_seed(9)
        out["mean"], out["invstd"] = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
        mu, iv = _dev(out["mean"], out["invstd"])
        out["bnpart"] = torch.full((rows, C, 2), float("nan"), device=DEV)
        lib.call("sd_heads_bnsum", *args, _d(mu), _d(iv), _d(out["bnpart"]), s)
    else:
        lib.call("sd_heads", *args, s)
    torch.cuda.synchronize()
    return out


def _finalize(out, C, mode, null_dwd=False, times=1):
    lib, s = L(), L().stream_handle()
    g = torch.full((2 * C + 2,), float("nan"), device=DEV)
    metrics = torch.zeros(5, dtype=torch.float64, device=DEV)
    for _ in range(times):
        lib.call("sd_heads_finalize", _d(out["part"]), out["rows"], C, None if null_dwd else _d(g[:C]), _d(g[2 * C:]),
                 _d(g[C:2 * C]), _d(g[2 * C + 1:]), _d(metrics) if mode == R.LOSS else None,
                 _d(out["count"]) if mode == R.LOSS else None, s)
    torch.cuda.synchronize()
    return {"dwd": g[:C], "dwl": g[C:2 * C], "dbd": g[2 * C:2 * C + 1], "dbl": g[2 * C + 1:], "metrics": metrics}


def _check_heads(tag, out, inp, ref, allowed, C, P, prec, mode, bnsum):
    _check(f"{tag}.disp", out["disp"], ref["disp"], allowed["disp"])
    _check(f"{tag}.logvar", out["logvar"], ref["logvar"], allowed["logvar"])
    if mode == R.INFER:
        return
    if prec == "bf16":  # stored: the round-to-nearest-even of an fp32 value within the allowed deviation
        _check_bf16(f"{tag}.da", out["da"], ref["da"], allowed["da"])
    else:
        _check(f"{tag}.da", out["da"], ref["da"], allowed["da"])
    # sums: a lane adds LPP pixels per iteration of its block's 256-pixel step (n), then <= 6 shuffle adds and 3 wave
    # adds (m = 9); the rows are added in fp64 and rounded to fp32 once
    lpp = C // 8
    n, m = -(-P // (out["rows"] * 256)) * lpp, 9
    gxd, gxl, act = ref["gxd"].abs(), ref["gxl"].abs(), ref["act"]
    terms = {"dwd": gxd @ act, "dwl": gxl @ act, "dbd": gxd.sum().reshape(1), "dbl": gxl.sum().reshape(1)}
    fin = _finalize(out, C, mode)
    for k in ("dwd", "dwl", "dbd", "dbl"):
        _check(f"{tag}.{k}", fin[k], ref[k].reshape(-1), allowed[k] + (n + m + 3) * U32 * terms[k])
    if mode == R.LOSS:
        n_valid = ref["n"]
        tol_m = allowed["metrics"] + (n // lpp + 6 + 3 + 2) * U32 * ref["metric_abs"]
        tol_m[4] = 0.0
        _check(f"{tag}.metrics", fin["metrics"], ref["metrics"], tol_m)
        fin2 = _finalize(out, C, mode, null_dwd=True, times=2)  # finalize adds into metrics; NULL dwd is skipped
        _check(f"{tag}.metrics_x2", fin2["metrics"], 2 * ref["metrics"], 2 * tol_m)
        assert float(fin2["metrics"][4]) == 2.0 * n_valid
        assert bool(torch.isnan(fin2["dwd"]).all()) and torch.equal(fin2["dwl"], fin["dwl"])
    if bnsum:
        da_stored = ref["da"].to(DTYPES[prec])
        s1, s2, a1, a2, ay = R.heads_bn_sums(da_stored, inp["y"], inp["scale"], inp["shift"], out["mean"], out["invstd"])
        got = out["bnpart"].double().sum(0).cpu()
        # both stored values are roundings (<= u_store * |x| each) of values within allowed["da"] of each other
        mask = R.relu_mask(inp["y"], inp["scale"], inp["shift"]).double()
        u_store = UBF16 if prec == "bf16" else U32
        d_da = (allowed["da"] + 2 * u_store * (ref["da"].abs() + allowed["da"])) * mask
        xh = ((inp["y"].double() - out["mean"].double()) * out["invstd"].double()).abs()
        _check(f"{tag}.bn_sum_dz", got[:, 0], s1, d_da.sum(0) + (n + m + 2) * U32 * a1)
        # the kernel forms sum dz*xhat as invstd*(sum dz*y - mean*sum dz): 3 more operations, on those terms
        cancel = out["invstd"].double().abs() * (ay + out["mean"].double().abs() * a1)
        _check(f"{tag}.bn_sum_dz_xhat", got[:, 1], s2, (d_da * xh).sum(0) + (n + m + 5) * U32 * cancel)


def _heads_cases():
    out = [(C, P, prec, mode) for C in (8, 16, 32, 64) for P in (1, 3, 777) for prec in ("fp32", "bf16")
           for mode in (R.INFER, R.LOSS, R.GRADS)]
    # two and three iterations of the 262144-pixel step: the pipelined loop drops a whole trailing iteration and a
    # partial group
    return out + [(C, P, prec, R.LOSS) for C in (32, 8) for P in (262144 + 5, 2 * 262144 + 77) for prec in ("fp32", "bf16")]


@pytest.mark.parametrize("C,P,prec,mode", _heads_cases())
def test_heads(C, P, prec, mode):
    inp, ref, allowed, dev32 = _heads_case(C, P, prec, mode)
    print("DEV32", f"heads[{C},{P},{prec},{mode}]", {k: f"{v:.3g}" for k, v in dev32.items()})
    for bnsum in ((False,) if mode == R.INFER else (False, True)):
        tag = f"heads{'_bnsum' if bnsum else ''}[{C},{P},{prec},{mode}]"
        out = _run_heads(inp, C, P, prec, mode, bnsum)
        _check_heads(tag, out, inp, ref, allowed, C, P, prec, mode, bnsum)
        if P > 262144:
            assert out["rows"] == 1024 and P > out["rows"] * 256  # the step of every C: a second iteration runs
    if mode == R.LOSS and P == 3:
        # disp, logvar and da may be NULL in LOSS mode: the same partials, bit for bit
        full, bare = _run_heads(inp, C, P, prec, mode, False), _run_heads(inp, C, P, prec, mode, False, null_outputs=True)
        assert torch.equal(full["part"], bare["part"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 32, 64])
def test_heads_with_nothing_valid(C, prec):
    """count == 0 with everything masked: da all zeros, partials all zeros, nothing NaN (NaN-filled buffers)."""
    P = 300
    inp, ref, _, _ = _heads_case(C, P, prec, R.LOSS, all_masked=True)
    assert ref["n"] == 0
    for bnsum in (False, True):
        out = _run_heads(inp, C, P, prec, R.LOSS, bnsum)
        assert int(out["count"]) == 0
        assert torch.equal(out["da"].float().cpu(), torch.zeros(P, C))
        assert torch.equal(out["part"].cpu(), torch.zeros(out["rows"], 2 * C + 7))
        if bnsum:
            assert torch.equal(out["bnpart"].cpu(), torch.zeros(out["rows"], C, 2))
        fin = _finalize(out, C, R.LOSS)
        assert torch.equal(fin["metrics"].cpu(), torch.zeros(5, dtype=torch.float64))
        assert float(torch.cat([fin[k] for k in ("dwd", "dwl", "dbd", "dbl")]).abs().max()) == 0.0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("case", ["lv_hi", "lv_lo", "lv_above", "lv_below", "sp_equal", "sp_pass"])
def test_heads_planted_branch_cases(case, C, prec):
    """xl exactly on a clamp (the gradient flows), one ulp outside (gradient 0, logvar clamped), p == t exactly above
    the softplus threshold (gradient 0) and the threshold branch passing the gradient unchanged."""
    P = 2
    inp, ref, allowed, _ = _heads_case(C, P, prec, R.LOSS, planted=case)
    for bnsum in (False, True):
        tag = f"heads{'_bnsum' if bnsum else ''}[{case},{C},{prec}]"
        out = _run_heads(inp, C, P, prec, R.LOSS, bnsum)
        _check_heads(tag, out, inp, ref, allowed, C, P, prec, R.LOSS, bnsum)
        fin = _finalize(out, C, R.LOSS)
        if case.startswith("lv"):
            assert torch.equal(out["logvar"].cpu().double(), ref["logvar"])  # the clamp value itself
            flows = case in ("lv_hi", "lv_lo")
            assert (float(fin["dbl"].abs().sum()) > 0) == flows and (float(ref["dbl"].abs().sum()) > 0) == flows
            if not flows:
                assert float(fin["dwl"].abs().max()) == 0.0
        else:
            assert torch.equal(out["disp"].cpu().double(), ref["disp"])  # x above the threshold: p = x = 25
            assert float(fin["dbd"]) > 0


# ------------------------------------------------------------------ 7. sd_count_valid
def _count_inputs(P, seed):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(P, generator=g) * 10
    mask = (torch.rand(P, generator=g) > 0.2).to(torch.uint8)
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"))):
        target[i::7] = v
    mask[1::5] = 2
    mask[2::9] = 255
    if P <= 5:
        mask[:] = torch.tensor([1, 2, 255, 0, 1], dtype=torch.uint8)[:P]
        target[:] = torch.tensor([1.0, 2.0, float("nan"), 3.0, float("inf")])[:P]
        target[0] = 0.5
    return target, mask


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 1027, 4 * (4 * 65536 + 300) + 3])
@pytest.mark.parametrize("ncount", [1, 2, 4])
@pytest.mark.parametrize("offset", ["aligned", "target+1", "mask+1"])
def test_count_valid(P, ncount, offset):
    lib, s = L(), L().stream_handle()
    target, mask = _count_inputs(P, seed=P)
    want = int(R.valid_pixels(target, mask).sum())  # the pixels the heads reference treats as valid
    tbuf = torch.zeros(P + 1, device=DEV)
    mbuf = torch.zeros(P + 4, dtype=torch.uint8, device=DEV)
    to, mo = (1 if offset == "target+1" else 0), (1 if offset == "mask+1" else 0)
    t, m = tbuf[to:to + P], mbuf[mo:mo + P]
    t.copy_(target)
    m.copy_(mask)
    assert t.data_ptr() % 16 == 4 * to and m.data_ptr() % 4 == mo
    # clear == NULL: a stale count is overwritten
    buf = torch.full((8,), 12345, dtype=torch.int32, device=DEV)
    lib.call("sd_count_valid", _d(t), _d(m), P, _d(buf), ncount, None, s)
    torch.cuda.synchronize()
    assert buf.cpu().tolist() == [want] * ncount + [12345] * (8 - ncount)
    # clear set: count is added to from zero, the other slot is zeroed
    buf = torch.tensor([0, 0, 0, 0, 99, 98, 97, 96], dtype=torch.int32, device=DEV)
    lib.call("sd_count_valid", _d(t), _d(m), P, _d(buf), ncount, _d(buf[4:]), s)
    torch.cuda.synchronize()
    assert buf.cpu().tolist() == [want] * ncount + [0] * (4 - ncount) + [0] * ncount + [99, 98, 97, 96][ncount:]


# ------------------------------------------------------------------ 8. sd_adamw
@pytest.mark.parametrize("n", [1, 255, 257, 2 * 262144 + 77])
@pytest.mark.parametrize("step0", [0, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw(n, step0, wd):
    """Five consecutive steps; each step is compared with the float64 restatement applied to the state the device
    held before it (one step's rounding, train_kernels_ref.adamw_tolerances). count == NULL on even steps, a nonzero
    count on odd ones; then *count == 0 changes nothing."""
    lib, s = L(), L().stream_handle()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    g = torch.Generator().manual_seed(n + step0)
    p = torch.randn(n, generator=g).to(DEV)
    if step0:
        m, v = (torch.randn(n, generator=g) * 0.1).to(DEV), (torch.rand(n, generator=g) * 0.5 + 1e-3).to(DEV)
    else:
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.tensor([step0], dtype=torch.int32, device=DEV)
    scratch = torch.zeros(4, device=DEV)
    some = torch.tensor([5], dtype=torch.int32, device=DEV)
    worst = 0.0
    for k in range(5):
        grad = torch.randn(n, generator=g).to(DEV)
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
        lib.call("sd_adamw", _d(p), _d(grad), _d(m), _d(v), n, lr, wd, b1, b2, eps, _d(step), _d(some) if k % 2 else None,
                 _d(scratch), s)
        torch.cuda.synchronize()
        t = step0 + k + 1
        assert int(step) == t and scratch.view(torch.int32).cpu().tolist() == [0, 0, 0, 0]
        pr, mr, vr = R.adamw_step(p0, grad.cpu(), m0, v0, t, lr, wd, b1, b2, eps)
        tp, tm, tv = R.adamw_tolerances(p0, grad.cpu(), m0, v0, t, lr, wd, b1, b2, eps)
        worst = max(worst, _check(f"adamw[{n},{step0},{wd}].p@{t}", p, pr, tp),
                    _check(f"adamw[{n},{step0},{wd}].m@{t}", m, mr, tm), _check(f"adamw[{n},{step0},{wd}].v@{t}", v, vr, tv))
    # a skipped step (*count == 0): nothing changes, *step stays, scratch stays 0
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    before = (p.clone(), m.clone(), v.clone())
    lib.call("sd_adamw", _d(p), _d(grad), _d(m), _d(v), n, lr, wd, b1, b2, eps, _d(step), _d(zero), _d(scratch), s)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v)))
    assert int(step) == step0 + 5 and scratch.view(torch.int32).cpu().tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ 9. sd_bnrelu_pool, sd_pool_bwd_add
# (1,2,2,8): one window, cpr = C/8 = 1; (2,6,10,24): cpr = 3 does not divide 256; (1,4,4,2048): cpr = 256, the largest C
POOL_SHAPES = [(1, 2, 2, 8), (2, 6, 10, 24), (3, 8, 12, 32), (1, 4, 4, 2048), (2, 16, 20, 256)]
POOL_FWD_LARGE = (5, 128, 128, 1024)  # B*(H/2)*(W/2)*(C/8) = 2621440 > 8192*256: the grid-stride loop runs again
_POOL = {}


def _pool_case(shape, prec):
    key = (shape, prec)
    if key not in _POOL:
        inp = R.make_pool_inputs(*shape, DTYPES[prec], seed=sum(shape))
        # the condition the ordering argument rests on (train_kernels_ref.make_pool_inputs)
        assert inp["gap"] > 8 * U32 * inp["zmax"], (shape, inp["gap"], inp["zmax"])
        _POOL[key] = inp
    return _POOL[key]


def _pool_large_case(shape):
    """One sample from the builder; sample b is that sample rolled by b windows along W (the windows stay aligned, the
    samples differ), so a large batch costs one sample's random draws. The references are still taken per sample."""
    B, H, W, C = shape
    one = R.make_pool_inputs(1, H, W, C, torch.bfloat16, seed=H + C)
    assert one["gap"] > 8 * U32 * one["zmax"]
    inp = dict(one)
    for k, (h, w) in (("y", (H, W)), ("dskip", (H, W)), ("dpool", (H // 2, W // 2))):
        v = one[k].view(h, w, C)
        step = 2 if h == H else 1
        inp[k] = torch.stack([torch.roll(v, step * b, 1) for b in range(B)]).reshape(B * h * w, C)
    return inp


def _sample(inp, b, H, W):
    """Sample b of a batched pool input as a B = 1 input."""
    n, n2 = H * W, (H // 2) * (W // 2)
    out = dict(inp)
    out.update(y=inp["y"][b * n:(b + 1) * n], dskip=inp["dskip"][b * n:(b + 1) * n], dpool=inp["dpool"][b * n2:(b + 1) * n2])
    return out


def _trunc_bf16(ref):
    return (ref.float().view(torch.int32) & -65536).view(torch.float32).double()


def check_pool_fwd(tag, got, inp, B, H, W, need_trunc_share=True):
    """sd_bnrelu_pool's output (CPU tensor [B*(H/2)*(W/2)][C]) against the float64 statement: the fp32 value has one
    fma rounding (tol32 = u*|ref|), nothing is allowed for the store. Pure CPU logic (also run on mutants by
    test_train_kernels_ref_cpu.py)."""
    ref = R.bnrelu_pool_ref(inp["y"], inp["scale"], inp["shift"], B, H, W).reshape(got.shape)
    tol = U32 * ref.abs()
    _check_bf16(tag, got, ref, tol)
    if need_trunc_share:  # the check tells round-to-nearest from truncation
        lo, hi = R.bf16_store_interval(ref, tol)
        t = _trunc_bf16(ref)
        assert float(((t < lo) | (t > hi)).double().mean()) > 0.25, tag


def check_pool_bwd(tag, da, inp, B, H, W, prec, skip):
    """sd_pool_bwd_add's da (CPU tensor [B*H*W][C] in the storage type) against ``pool_bwd_ref``.
    Off the arg-max: da == dskip bit for bit (exactly 0 without dskip). At the arg-max: one fp32 add, tol = u*|ref|
    (bf16: the round-to-nearest-even of such a value); without dskip exactly dpool. Pure CPU logic."""
    ref, am = R.pool_bwd_ref(inp["y"], inp["scale"], inp["shift"], inp["dskip"] if skip else None, inp["dpool"], B, H, W)
    ref = ref.reshape(da.shape)
    hit = R.pool_hit(am, B, H, W).reshape(da.shape)
    assert not bool(torch.isnan(da.float()).any()), tag
    if not skip:
        print(f"RATIO {tag} exact")
        assert torch.equal(da.double(), ref), (tag, int((da.double() != ref).sum()))
        return
    bits = torch.int32 if prec == "fp32" else torch.int16
    off_bad = (da.view(bits) != inp["dskip"].view(bits)) & ~hit
    assert not bool(off_bad.any()), (tag, "off the arg-max", int(off_bad.sum()))
    tol = torch.where(hit, U32 * ref.abs(), torch.zeros((), dtype=torch.float64))
    if prec == "fp32":
        _check(tag, da, ref, tol)
    else:
        _check_bf16(tag, da, ref, tol)


def _pool_dev(inp):
    return {k: v.to(DEV).contiguous() for k, v in inp.items() if torch.is_tensor(v)}


def _run_pool_fwd(d, B, H, W, C):
    out = torch.full((B * (H // 2) * (W // 2), C), float("nan"), dtype=torch.bfloat16, device=DEV)
    L().call("sd_bnrelu_pool", L().SD_BF16, _d(d["y"]), _d(d["scale"]), _d(d["shift"]), B, H, W, C, _d(out),
             L().stream_handle())
    torch.cuda.synchronize()
    return out.cpu()


def _run_pool_bwd(d, B, H, W, C, prec, skip, fused):
    lib = L()
    rows = lib.call("sd_pool_bwd_rows", B, H, W, C)
    da = torch.full((B * H * W, C), float("nan"), dtype=DTYPES[prec], device=DEV)
    part = torch.full((rows, C, 2), float("nan"), device=DEV) if fused else None
    lib.call("sd_pool_bwd_add", _sd(prec), _d(d["y"]), _d(d["scale"]), _d(d["shift"]), _d(d["dskip"]) if skip else None,
             _d(d["dpool"]), B, H, W, C, _d(da), _d(d["mean"]) if fused else None, _d(d["invstd"]) if fused else None,
             _d(part), lib.stream_handle())
    torch.cuda.synchronize()
    return da.cpu(), (part.double().sum(0).cpu() if fused else None), rows


def _check_pool_sums(tag, got, sums, rows, total, C):
    """partials summed over rows against bn_bwd_sums of the da the kernel stored: the `sums` rule with n = 4 adds per
    loop trip of a thread (one per window position) and m = 256/cpr adds of the in-block reduction; sum dz*xhat has
    k = 3 more roundings per term ((y - mean), * invstd, the product)."""
    s1, s2, a1, a2 = sums
    n, m = 4 * -(-total // (rows * 256)), 256 // (C // 8)
    _check(f"{tag}.sum_dz", got[:, 0], s1, (n + m + 2) * U32 * a1)
    _check(f"{tag}.sum_dz_xhat", got[:, 1], s2, (n + m + 2 + 3) * U32 * a2)


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_bnrelu_pool(shape):
    B, H, W, C = shape
    inp = _pool_case(shape, "bf16")
    got = _run_pool_fwd(_pool_dev(inp), B, H, W, C)
    check_pool_fwd(f"bnrelu_pool{list(shape)}", got, inp, B, H, W, need_trunc_share=got.numel() >= 1000)


def test_bnrelu_pool_past_one_grid_sweep():
    B, H, W, C = POOL_FWD_LARGE
    assert B * (H // 2) * (W // 2) * (C // 8) > 8192 * 256
    inp = _pool_large_case(POOL_FWD_LARGE)
    got = _run_pool_fwd(_pool_dev(inp), B, H, W, C)
    n2 = (H // 2) * (W // 2)
    for b in range(B):  # the float64 reference sample by sample
        check_pool_fwd(f"bnrelu_pool{list(POOL_FWD_LARGE)}@{b}", got[b * n2:(b + 1) * n2], _sample(inp, b, H, W), 1, H, W)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_bwd_add(shape, prec, skip, fused):
    B, H, W, C = shape
    inp = _pool_case(shape, prec)
    tag = f"pool_bwd{list(shape)}[{prec},{'skip' if skip else 'noskip'},{'fused' if fused else 'plain'}]"
    d = _pool_dev(inp)
    if fused and 256 % (C // 8):
        # C/8 = 3 does not divide 256: the fused request is an error and nothing is launched
        lib = L()
        da = torch.full((B * H * W, C), float("nan"), dtype=DTYPES[prec], device=DEV)
        part = torch.full((lib.call("sd_pool_bwd_rows", B, H, W, C), C, 2), float("nan"), device=DEV)
        with pytest.raises(lib.StereoHipError, match="C/8 dividing 256"):
            lib.call("sd_pool_bwd_add", _sd(prec), _d(d["y"]), _d(d["scale"]), _d(d["shift"]), _d(d["dskip"]),
                     _d(d["dpool"]), B, H, W, C, _d(da), _d(d["mean"]), _d(d["invstd"]), _d(part), lib.stream_handle())
        torch.cuda.synchronize()
        assert bool(torch.isnan(da.float()).all()) and bool(torch.isnan(part).all())
        return
    da, got, rows = _run_pool_bwd(d, B, H, W, C, prec, skip, fused)
    check_pool_bwd(tag, da, inp, B, H, W, prec, skip)
    if fused:
        sums = R.bn_bwd_sums(da, inp["y"], inp["scale"], inp["shift"], inp["mean"], inp["invstd"])
        _check_pool_sums(tag, got, sums, rows, B * (H // 2) * (W // 2) * (C // 8), C)


def test_pool_bwd_add_past_one_grid_sweep():
    """bf16, with dskip and the fused sums, at the smallest batch of 128 x 128 x 512 samples whose work exceeds the
    resident-block cap (a runtime query), so every thread's loop runs more than once."""
    lib = L()
    H, W, C = 128, 128, 512
    per = (H // 2) * (W // 2) * (C // 8)
    B = next((b for b in (1, 2, 3, 4, 6, 8) if lib.call("sd_pool_bwd_rows", b, H, W, C) * 256 < b * per), None)
    assert B is not None
    rows = lib.call("sd_pool_bwd_rows", B, H, W, C)
    assert rows * 256 < B * per
    print(f"pool_bwd large case: B={B} rows={rows}")
    inp = _pool_large_case((B, H, W, C))
    da, got, rows2 = _run_pool_bwd(_pool_dev(inp), B, H, W, C, "bf16", True, True)
    assert rows2 == rows
    n = H * W
    sums = None
    for b in range(B):  # the float64 reference sample by sample
        one = _sample(inp, b, H, W)
        check_pool_bwd(f"pool_bwd[{B},{H},{W},{C}]@{b}", da[b * n:(b + 1) * n], one, 1, H, W, "bf16", True)
        s = R.bn_bwd_sums(da[b * n:(b + 1) * n], one["y"], inp["scale"], inp["shift"], inp["mean"], inp["invstd"])
        sums = s if sums is None else tuple(a + c for a, c in zip(sums, s))
    _check_pool_sums(f"pool_bwd[{B},{H},{W},{C}]", got, sums, rows, B * per, C)


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_pool_forward_and_backward_agree_on_the_winner(shape):
    """bf16: relu(fma(y, scale, shift)) at the position where sd_pool_bwd_add put dpool, rounded to bf16, is the element
    sd_bnrelu_pool stored (dpool is nowhere 0 and dskip absent, so da != 0 marks the position)."""
    B, H, W, C = shape
    inp = _pool_case(shape, "bf16")
    d = _pool_dev(inp)
    da, _, _ = _run_pool_bwd(d, B, H, W, C, "bf16", False, False)
    fwd = _run_pool_fwd(d, B, H, W, C)
    put = R.pool_windows(da.double() != 0, B, H, W)
    assert torch.equal(put.sum(3), torch.ones_like(put.sum(3)))  # one position per window and channel
    z = R.pool_windows(torch.relu(inp["y"].double() * inp["scale"].double() + inp["shift"].double()), B, H, W)
    at = (z * put).sum(3).reshape(fwd.shape)
    _check_bf16(f"pool_winner{list(shape)}", fwd, at, U32 * at.abs())
