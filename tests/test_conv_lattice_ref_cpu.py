"""The lattice reference of the exact conv tests is right, and its checks can fail (CPU only).

1. The float64 statements of conv_lattice_ref.py equal PyTorch's own operators on the lattice inputs, exactly.
2. The lattice claim: fp32 evaluations in two different summation orders both equal the float64 result bit for bit for
   the generated cases of test_gpu_conv_exact.py, so no summation order of a kernel can matter.
3. An fp32/bf16 emulation of a kernel passes the equality checks of test_gpu_conv_exact.py, and each of ten subtle
   defects applied to it fails them; two of them are shown to pass the max-norm bounds of test_gpu_ops.py at the same
   shape on that file's random data.
"""

import pytest
import torch
import torch.nn.functional as F

import conv_lattice_ref as R
import test_gpu_conv_exact as T

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ 1. statements
def test_rne_bf16_matches_torch_and_truncation_differs():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g) * 1000, torch.tensor([257.0, 259.0, 258.0, -257.0, 0.0, 1.0 + 2 ** -8,
                                                                         1.0 + 3 * 2 ** -8, 3.3895e38, 2.0 ** -130])])
    x = x.double()
    assert torch.equal(R.rne_bf16(x), x.float().to(BF).double())
    assert float(R.rne_bf16(torch.tensor([257.0], dtype=R.F64))) == 256.0  # tie -> even
    assert float(R.rne_bf16(torch.tensor([259.0], dtype=R.F64))) == 260.0
    assert float(R.trunc_bf16(torch.tensor([259.0], dtype=R.F64))) == 258.0
    assert R.step_of(torch.tensor([0.75, 4.0, 0.0])) == 0.25


@pytest.mark.parametrize("B,H,W,ci,co", [(2, 9, 11, 8, 16), (1, 1, 1, 8, 8), (3, 2, 5, 16, 8)])
def test_conv_statements_equal_torch(B, H, W, ci, co):
    x = R.bn_relu(R.acts(B, ci, H, W, 1), *R.bn_affine(ci, 2))
    w = R.weights((co, ci, 3, 3), 3)
    dy = R.acts(B, co, H, W, 4)
    assert torch.equal(R.conv3x3(x, w), F.conv2d(x, w, padding=1))
    assert torch.equal(R.conv3x3_dgrad(dy, w), torch.nn.grad.conv2d_input(x.shape, w, dy, padding=1))
    assert torch.equal(R.conv3x3_wgrad(x, dy), torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=1))
    assert torch.equal(R.chan_sums(dy)[:, 0], dy.sum((0, 2, 3)))
    wt = R.weights((ci, co, 2, 2), 5, exp=-2)
    bias = R.int_bias(co, 6)
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, wt, bias))
    ref = F.conv_transpose2d(xg, wg, bg, stride=2)
    assert torch.equal(R.convT(x, wt, bias), ref.detach())
    dout = R.acts(B, co, 2 * H, 2 * W, 7)
    ref.backward(dout)
    assert torch.equal(R.convT_dgrad(dout, wt), xg.grad)
    assert torch.equal(R.convT_wgrad(x, dout), wg.grad)
    assert torch.equal(R.chan_sums(dout)[:, 0], bg.grad)
    xp = R.acts(B, ci, 2 * H, 2 * W, 8)
    assert torch.equal(R.pool2(xp), F.max_pool2d(xp, 2))


def test_bn_backward_statement_equals_autograd():
    """The masked part exactly (autograd through relu(scale*y + shift) on lattice parameters), and the whole apply
    against autograd through a float64 training BatchNorm + ReLU, whose batch statistics are not on the lattice (hence
    1e-12 relative here, the only tolerance of this file)."""
    B, C, H, W = 2, 8, 6, 7
    bb = R.BnBwd(B, C, H, W, 11)
    y = bb.y.clone().requires_grad_(True)
    torch.relu(y * bb.scale.view(1, -1, 1, 1) + bb.shift.view(1, -1, 1, 1)).backward(bb.da)
    zero = torch.zeros(C, dtype=R.F64)
    coef = torch.stack([bb.scale, zero, zero], 1)
    assert torch.equal(R.bn_bwd_dy(bb.da, bb.y, bb.scale, bb.shift, zero, zero + 1, coef), y.grad)
    g = torch.Generator().manual_seed(1)
    gamma = torch.randn(C, generator=g).double()
    beta = torch.randn(C, generator=g).double()
    y = bb.y.clone().requires_grad_(True)
    torch.relu(F.batch_norm(y, None, None, gamma, beta, training=True, eps=1e-5)).backward(bb.da)
    mean, var = bb.y.mean((0, 2, 3)), bb.y.var((0, 2, 3), unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    sums = R.bn_bwd_sums(bb.da, bb.y, scale, shift, mean, invstd) / (B * H * W)
    coef = torch.stack([scale, sums[:, 0], sums[:, 1]], 1)
    dy = R.bn_bwd_dy(bb.da, bb.y, scale, shift, mean, invstd, coef)
    assert torch.allclose(dy, y.grad, rtol=1e-12, atol=1e-12)


def test_pack_layouts_read_back_the_weights():
    w = R.weights((16, 8, 3, 3), 1)
    p = R.pack_conv3(w, 8, False, 128).reshape(16, 128)
    assert torch.equal(p[:, :72].reshape(16, 9, 8).permute(0, 2, 1).reshape(16, 8, 3, 3), w) and float(p[:, 72:].abs().max()) == 0
    dy = R.acts(1, 16, 5, 6, 3)
    pd = R.pack_conv3(w, 8, True, 192)[:, :144].reshape(8, 9, 16)  # [ci][tap][o]: the dgrad as a forward conv
    assert torch.equal(R.conv3x3(dy, pd.permute(0, 2, 1).reshape(8, 16, 3, 3)), R.conv3x3_dgrad(dy, w))
    ws = R.split_weights((16, 8, 3, 3), 4)
    ps = R.pack_conv3_split(ws, 8, 192)[:, :144].reshape(16, 9, 2, 8)
    assert torch.equal((ps[:, :, 0] + ps[:, :, 1]).permute(0, 2, 1).reshape(16, 8, 3, 3), ws)
    wt = R.weights((8, 4, 2, 2), 5)
    assert torch.equal(R.pack_convT(wt, False, 64)[:, :8].reshape(4, 4, 8).permute(2, 1, 0).reshape(8, 4, 2, 2), wt)
    assert torch.equal(R.pack_convT(wt, True, 64)[:, :16].reshape(8, 4, 4).permute(0, 2, 1).reshape(8, 4, 2, 2), wt)


# ------------------------------------------------------------------------------------------------ 2. the lattice claim
# Every statement, on every generated case of test_gpu_conv_exact.py (every parameter list, none left out), evaluated in
# fp32 in two different summation orders: order A is ATen's own operator in float32, order B a hand-written loop with
# the taps permuted, the channels or images reversed and plain fp32 adds. Both must equal the float64 result bit for bit.
def _eq(a, want):
    assert a.dtype == torch.float32 and torch.equal(a.double(), want)


def _conv_b(x, w):
    """fp32 conv, order B: taps outermost in a permuted order, the channels reversed, fp32 adds between taps."""
    B, C, H, W = x.shape
    p = F.pad(x.float(), (1, 1, 1, 1)).flip(1)
    wf = w.float().flip(1)
    out = torch.zeros(B, w.shape[0], H, W)
    for kh in (2, 0, 1):
        for kw in (1, 2, 0):
            out += torch.einsum("bihw,oi->bohw", p[:, :, kh:kh + H, kw:kw + W], wf[:, :, kh, kw])
    return out


def _both_conv(x, w, want):
    _eq(F.conv2d(x.float(), w.float(), padding=1), want)
    _eq(_conv_b(x, w), want)


def _both_dgrad(dy, w, want):
    _eq(torch.nn.grad.conv2d_input(want.shape, w.float(), dy.float(), padding=1), want)
    _eq(_conv_b(dy, w.flip(2, 3).transpose(0, 1)), want)


def _both_wgrad(x, dy, want):
    _eq(torch.nn.grad.conv2d_weight(x.float(), want.shape, dy.float(), padding=1), want)
    B, C, H, W = x.shape
    p = F.pad(x.float(), (1, 1, 1, 1))
    d = dy.float()
    b = torch.zeros(want.shape)
    for bi in reversed(range(B)):  # image-outer running fp32 sums, the last image first, the rows in two halves
        for rows in (slice(H // 2, H), slice(0, H // 2)):
            for kh in (1, 2, 0):
                for kw in (2, 1, 0):
                    q = p[bi, :, kh:kh + H, kw:kw + W][:, rows]
                    b[:, :, kh, kw] += torch.einsum("ohw,ihw->oi", d[bi][:, rows], q)
    _eq(b, want)


def _both_sums(v, want):
    """Per-channel fp32 sums of v [B][C][H][W] against want [C]: torch.sum's pairwise order and a reversed running sum."""
    f = v.float().permute(1, 0, 2, 3).reshape(v.shape[1], -1)
    _eq(f.sum(1), want)
    _eq(torch.cumsum(f.flip(1), 1)[:, -1], want)


def _both_stats(stored, want):
    _both_sums(stored, want[:, 0])
    _both_sums(stored.float().square().double(), want[:, 1])


def _v32(t):
    return t.float().view(1, -1, 1, 1)


def _both_bn_sums(stored, y, sc, sh, mu, inv, want):
    """The BatchNorm-backward sums in fp32 with a fused and an unfused mask and xhat, each in two sum orders."""
    y32, d32 = y.float(), stored.float()
    for z in (torch.addcmul(_v32(sh), y32, _v32(sc)), y32 * _v32(sc) + _v32(sh)):
        dz = torch.where(z > 0, d32, torch.zeros_like(d32))
        for xhat in ((y32 - _v32(mu)) * _v32(inv), torch.addcmul(-_v32(mu) * _v32(inv), y32, _v32(inv))):
            _both_sums(dz.double(), want[:, 0])
            _both_sums((dz * xhat).double(), want[:, 1])


def _both_bn_dy(bb):
    """The BatchNorm-backward apply in fp32, unfused and with fused multiply-adds (addcmul), against the float64 dy."""
    y, da, c = bb.y.float(), bb.da.float(), bb.coef
    for fused in (False, True):
        z = torch.addcmul(_v32(bb.shift), y, _v32(bb.scale)) if fused else y * _v32(bb.scale) + _v32(bb.shift)
        dz = torch.where(z > 0, da, torch.zeros_like(da))
        xhat = (y - _v32(bb.mean)) * _v32(bb.invstd)
        if fused:
            dy = _v32(c[:, 0]) * torch.addcmul(dz - _v32(c[:, 1]), xhat, -_v32(c[:, 2]))
        else:
            dy = _v32(c[:, 0]) * dz - _v32(c[:, 0]) * _v32(c[:, 1]) - _v32(c[:, 0]) * (xhat * _v32(c[:, 2]))
        _eq(dy, bb.dy)


def _both_convT(x, wt, bias, want):
    _eq(F.conv_transpose2d(x.float(), wt.float(), bias.float(), stride=2), want)
    B, C, h, w_ = x.shape
    acc = torch.zeros(B, wt.shape[1], 2 * h, 2 * w_)
    xf, wf = x.float().flip(1), wt.float().flip(0)
    for a in (1, 0):
        for b in (0, 1):
            acc[:, :, a::2, b::2] = torch.einsum("bihw,io->bohw", xf, wf[:, :, a, b])
    _eq(acc + _v32(bias), want)


def _both_convT_dgrad(dout, wt, want):
    _eq(F.conv2d(dout.float(), wt.float(), stride=2), want)
    acc = torch.zeros(want.shape)
    for a, b in ((1, 1), (0, 1), (1, 0), (0, 0)):
        acc += torch.einsum("bohw,io->bihw", dout[:, :, a::2, b::2].float().flip(1), wt[:, :, a, b].float().flip(1))
    _eq(acc, want)


def _both_convT_wgrad(x, dout, dw, db):
    xg = x.float()
    wg = torch.zeros(dw.shape, requires_grad=True)
    bg = torch.zeros(db.shape, requires_grad=True)
    F.conv_transpose2d(xg, wg, bg, stride=2).backward(dout.float())
    _eq(wg.grad, dw)
    _eq(bg.grad, db)
    acc = torch.zeros(dw.shape)
    for bi in reversed(range(x.shape[0])):
        for a in (1, 0):
            for b in (1, 0):
                acc[:, :, a, b] += torch.einsum("ihw,ohw->io", xg[bi], dout[bi, :, a::2, b::2].float())
    _eq(acc, dw)
    _both_sums(dout, db)


def _fwd_both(case, stats):
    S, w, out = case[:3]
    x = S.x()
    if len(case) == 4:  # output affine: fused and unfused on each order of the accumulator
        aff = case[3]
        for acc in (F.conv2d(x.float(), w.float(), padding=1), _conv_b(x, w)):
            _eq(torch.addcmul(_v32(aff[1]), acc, _v32(aff[0])), out)
            _eq(acc * _v32(aff[0]) + _v32(aff[1]), out)
    else:
        _both_conv(x, w, out)
    if stats:
        _both_stats(R.rne_bf16(out), R.chan_sums(R.rne_bf16(out)))
        _both_stats(out, R.chan_sums(out))  # what the fp32 path sums


@pytest.mark.parametrize("B,H,W,ci,co,pool,bn", T.FWD)
def test_two_orders_forward(B, H, W, ci, co, pool, bn):
    _fwd_both(T._fwd_case(B, H, W, (ci,), co, (bn,), pool, "round"), False)
    _fwd_both(T._fwd_case(B, H, W, (ci,), co, (bn,), pool, "stats"), True)


@pytest.mark.parametrize("env,B,H,W,chans,co,bn", T.FWD_ENV)
def test_two_orders_forward_variants(env, B, H, W, chans, co, bn):
    _fwd_both(T._fwd_case(B, H, W, chans, co, bn, False, "round"), False)
    _fwd_both(T._fwd_case(B, H, W, chans, co, bn, False, "stats"), True)


@pytest.mark.parametrize("B,H,W,c0,c1,co", T.DUAL)
def test_two_orders_dual_source_and_dgrad(B, H, W, c0, c1, co):
    _fwd_both(T._fwd_case(B, H, W, (c0, c1), co, (False, True), False, "round"), False)
    N = c0 + c1
    dy, w, dx = T._dgrad_case(B, H, W, co, N, "round")
    _both_dgrad(dy, w, dx)
    if N == 32 or N % 64 == 0:
        dy, w, dx = T._dgrad_case(B, H, W, co, N, "stats")
        _both_dgrad(dy, w, dx)
        _both_stats(R.rne_bf16(dx), R.chan_sums(R.rne_bf16(dx)))


@pytest.mark.parametrize("B,H,W,ci,co", T.WGRAD)
def test_two_orders_wgrad(B, H, W, ci, co):
    S, dy, dw = T._wgrad_case(B, H, W, (ci,), co, (False,))
    _both_wgrad(S.x(), dy, dw)


@pytest.mark.parametrize("env,B,H,W,chans,co", T.WGRAD_BN)
def test_two_orders_wgrad_bn_sources(env, B, H, W, chans, co):
    S, dy, dw = T._wgrad_case(B, H, W, chans, co, (True,) * len(chans))
    _both_wgrad(S.x(), dy, dw)


@pytest.mark.parametrize("env,B,H,W,chans,co", T.BNBWD)
def test_two_orders_wgrad_fused_bn_backward(env, B, H, W, chans, co):
    S, bb, dw = T._bnbwd_case(B, H, W, chans, co)
    _both_bn_dy(bb)
    _both_wgrad(S.x(), bb.dy, dw)


@pytest.mark.parametrize("B,h,w_,ci,co", T.CONVT)
def test_two_orders_convT(B, h, w_, ci, co):
    S, wt, bias, out, dout, dx = T._convT_case(B, h, w_, ci, co, True)
    _both_convT(S.x(), wt, bias, out)
    _both_convT_dgrad(dout, wt, dx)
    S, dout, dw, db = T._convT_wgrad_case(B, h, w_, ci, co)
    _both_convT_wgrad(S.x(), dout, dw, db)


@pytest.mark.parametrize("env,B,h,w_,ci,co,bn", T.CONVT_ENV)
def test_two_orders_convT_routes(env, B, h, w_, ci, co, bn):
    S, wt, bias, out = T._convT_case(B, h, w_, ci, co, bn)[:4]
    _both_convT(S.x(), wt, bias, out)


def test_two_orders_convT_split():
    S, wt, bias, out = T._convT_case(2, 12, 20, 64, 32, True, True)
    _both_convT(S.x(), wt, bias, out)


@pytest.mark.parametrize("B,H,W,ci,co,convt", T.BNSUM)
def test_two_orders_bnsum(B, H, W, ci, co, convt):
    dout, w, dx, y, (sc, sh, mu, inv), sums = T._bnsum_case(B, H, W, ci, co, convt)
    if convt:
        _both_convT_dgrad(dout, w, dx)
    else:
        _both_conv(dout, w, dx)
    _both_bn_sums(R.rne_bf16(dx), y, sc, sh, mu, inv, sums)


@pytest.mark.parametrize("wsplit", [True, False])
@pytest.mark.parametrize("B,H,W,chans,co,bn,epi", T.EX)
def test_two_orders_ex(wsplit, B, H, W, chans, co, bn, epi):
    sums = epi == "stats" and not wsplit
    _fwd_both(T._fwd_case(B, H, W, chans, co, bn, False, "stats" if sums else "round", wsplit,
                          21 if epi == "affine" else None), sums)


@pytest.mark.parametrize("H,W,chans,co,wsplit,affine", T.EX_WS)
def test_two_orders_ex_split_k(H, W, chans, co, wsplit, affine):
    _fwd_both(T._fwd_case(1, H, W, chans, co, (True,) * len(chans), False, "round", wsplit, 22 if affine else None), False)


@pytest.mark.parametrize("B,H,W,dec", [(2, 16, 64, False), (1, 8, 32, False), (3, 24, 48, False), (2, 16, 64, True),
                                       (1, 8, 16, True), (3, 24, 48, True)])
def test_two_orders_fused_backwards(B, H, W, dec):
    bb, S, w, dw, dx, sums, prev = T._bwd_fused_case(B, H, W, dec)
    _both_bn_dy(bb)
    _both_wgrad(S.x(), bb.dy, dw)
    _both_dgrad(bb.dy, w, dx)
    if dec:
        _both_sums(R.rne_bf16(dx)[:, :32], sums)
    else:
        yp, (psc, psh) = S.parts[0]
        _both_bn_sums(R.rne_bf16(dx), yp, psc, psh, prev[0], prev[1], sums)


# ------------------------------------------------------------------------------------------------ 3. emulation, defects
def _stage(v):
    """A bf16 staging store of an fp32 value, as the kernels do (PyTorch's conversion: RNE)."""
    return v.to(BF).float()


def emu_source(S, swap_second=False, mask_ge=False):
    xs = []
    for k, (y, bn) in enumerate(S.parts):
        v = _stage(y.float())
        if bn is not None:
            z = torch.addcmul(bn[1].float().view(1, -1, 1, 1), v, bn[0].float().view(1, -1, 1, 1))  # one fma
            v = _stage(torch.where(z > 0, z, torch.zeros_like(z)))
        if S.pool:
            v = F.max_pool2d(v, 2)
        if swap_second and k == 1:
            v = v.clone()
            v[:, [2, 3]] = v[:, [3, 2]]
        xs.append(v)
    return torch.cat(xs, 1)


def emu_conv(x, w, drop_corner_tap=None, neighbour_halo=False):
    """fp32 accumulation of bf16 operands over a zero halo. drop_corner_tap (an input channel): that channel's centre
    tap is skipped at pixel (0, 0) of image 0, one (tap, channel) product per output. neighbour_halo: the halo row
    above image b > 0 holds the last row of image b - 1."""
    B, C, H, W = x.shape
    p = F.pad(x, (1, 1, 1, 1))
    if neighbour_halo:
        p[1:, :, 0, 1:-1] = x[:-1, :, H - 1, :]
    wq = _stage(w.float())
    acc = torch.zeros(B, w.shape[0], H, W)
    for kh in range(3):
        for kw in range(3):
            q = p[:, :, kh:kh + H, kw:kw + W]
            if drop_corner_tap is not None and kh == 1 and kw == 1:
                q = q.clone()
                q[0, drop_corner_tap, 0, 0] = 0.0
            acc += torch.einsum("bihw,oi->bohw", q, wq[:, :, kh, kw])
    return acc


def emu_store(acc, prec, truncate=False):
    if prec == "fp32":
        return acc
    if truncate:
        return (acc.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)
    return acc.to(BF)


def emu_wgrad(x, dy, skip_last_pixel=None):
    """fp32 sums of bf16 products over every pixel. skip_last_pixel: True, or one x channel: the last pixel of the last
    image (the end of the last, ragged tile) is left out of the sums of every x channel, or of that one."""
    B, C, H, W = x.shape
    p = F.pad(x, (1, 1, 1, 1))
    d = _stage(dy.float())
    cut = d.clone()
    cut[B - 1, :, H - 1, W - 1] = 0.0
    dw = torch.zeros(dy.shape[1], C, 3, 3)
    for kh in range(3):
        for kw in range(3):
            q = p[:, :, kh:kh + H, kw:kw + W]
            dw[:, :, kh, kw] = torch.einsum("bohw,bihw->oi", cut if skip_last_pixel is True else d, q)
            if skip_last_pixel is not None and skip_last_pixel is not True:
                c = skip_last_pixel
                dw[:, c, kh, kw] = torch.einsum("bohw,bhw->o", cut, q[:, c])
    return dw


def _bits(t64, prec):
    return R.expected(t64, prec)


def test_emulated_forward_passes_and_defects_fail():
    """On the GPU file's (2, 15, 20, 40 -> 128) BN+ReLU case the emulation stores the expected bits in both modes; a
    (tap, channel) product dropped at one corner pixel, a neighbour image's row in the halo, a truncating store and
    STATS taken from the fp32 accumulator each fail. On the random data of test_gpu_ops.py at its (1, 30, 40, 64 -> 192)
    shape the dropped product passes the old bound 5e-3 * (1 + max|ref|) (about 0.027) whenever the corner activation
    is below about 0.2 (the largest of the 192 weights of a (tap, channel) pair is about 0.12): shown for the first
    channel whose corner value is below 0.1."""
    B, H, W, ci, co = 2, 15, 20, 40, 128
    S, w, out = T._fwd_case(B, H, W, (ci,), co, (True,), False, "round")
    x = emu_source(S)
    assert torch.equal(x.double(), S.x())
    cz = int((x[0, :, 0, 0] != 0).nonzero()[0])  # a channel the ReLU leaves non-zero at the corner
    for prec in ("fp32", "bf16"):
        assert torch.equal(emu_store(emu_conv(x, w), prec), _bits(out, prec))
        assert not torch.equal(emu_store(emu_conv(x, w, drop_corner_tap=cz), prec), _bits(out, prec))
        assert not torch.equal(emu_store(emu_conv(x, w, neighbour_halo=True), prec), _bits(out, prec))
    bad = emu_store(emu_conv(x, w, drop_corner_tap=cz), "bf16")
    assert int((bad != _bits(out, "bf16")).sum()) <= co  # one pixel's channels only, of 76800 elements
    assert not torch.equal(emu_store(emu_conv(x, w), "bf16", truncate=True), _bits(out, "bf16"))
    # the old check at this shape, on its data (test_conv3x3_fwd_with_bn_pool_gather_and_stats): the defect passes
    H, W, ci, co = 30, 40, 64, 192
    torch.manual_seed(0)
    y = torch.randn(1, ci, H, W).to(BF).float()
    wr = (torch.randn(co, ci, 3, 3) / (3 * ci ** 0.5)).to(BF).float()
    ref = F.conv2d(y, wr, padding=1)
    c = int((y[0, :, 0, 0].abs() < 0.1).nonzero()[0])
    got = emu_conv(y, wr, drop_corner_tap=c).to(BF).float()
    assert float((got - ref).abs().max()) <= 5e-3 * (1 + float(ref.abs().max()))
    assert not torch.equal(got, emu_conv(y, wr).to(BF).float())
    # STATS of the accumulator instead of the stored value: every STATS lattice rounds stored values in every channel
    # (a condition of the case), so the accumulator's sums differ in every channel
    S, w, out = T._fwd_case(2, 12, 20, (16,), 32, (False,), False, "stats")
    acc = emu_conv(emu_source(S), w)
    stored = emu_store(acc, "bf16").double()
    want = R.chan_sums(R.rne_bf16(out))
    assert torch.equal(R.chan_sums(stored), want)
    assert bool((R.chan_sums(acc.double()) != want).any(1).all())


def test_emulated_wgrad_passes_and_skipped_pixel_fails():
    """The (1, 30, 40, 40 -> 128) shape: the last pixel of the last (ragged) tile skipped, for every x channel or for
    one, fails the equality. On test_gpu_ops.py's random data the old bound 1e-2 * (1 + max|ref|) is 1.77 there: it
    passes the defect whenever the lost products max|dy| * max|x| stay below that, shown for the first x channel where
    they do; skipped for all 40 channels at once, the largest of the 128 x 160 lost products is 7.0 on that data, which
    the old bound does catch."""
    B, H, W, ci, co = 1, 30, 40, 40, 128
    S, dy, dw = T._wgrad_case(B, H, W, (ci,), co, (False,))
    x = emu_source(S)
    assert torch.equal(emu_wgrad(x, dy), _bits(dw, "fp32"))
    assert not torch.equal(emu_wgrad(x, dy, skip_last_pixel=True), _bits(dw, "fp32"))
    for c in range(ci):
        assert not torch.equal(emu_wgrad(x, dy, skip_last_pixel=c), _bits(dw, "fp32"))
    torch.manual_seed(2)
    xr = torch.randn(B, ci, H, W).to(BF).float()
    dr = torch.randn(B, co, H, W).to(BF)
    ref = torch.nn.grad.conv2d_weight(xr, (co, ci, 3, 3), dr.float(), padding=1)
    bound = 1e-2 * (1 + float(ref.abs().max()))
    lost = float(dr[B - 1, :, H - 1, W - 1].float().abs().max()) * xr[B - 1, :, H - 2:, W - 2:].abs().amax((1, 2))
    c = int((lost < 0.9 * bound).nonzero()[0])
    got = emu_wgrad(xr, dr, skip_last_pixel=c)
    assert not torch.equal(got, emu_wgrad(xr, dr))
    assert float((got - ref).abs().max()) <= bound
    assert float((emu_wgrad(xr, dr, skip_last_pixel=True) - ref).abs().max()) > bound


def test_cat_channel_swap_and_split_offset_fail():
    B, H, W, c0, c1, co = 1, 16, 32, 8, 24, 32
    S, w, out = T._fwd_case(B, H, W, (c0, c1), co, (False, True), False, "round")
    assert torch.equal(emu_store(emu_conv(emu_source(S), w), "bf16"), _bits(out, "bf16"))
    assert not torch.equal(emu_store(emu_conv(emu_source(S, swap_second=True), w), "bf16"), _bits(out, "bf16"))
    dy, wd, dx = T._dgrad_case(B, H, W, co, c0 + c1, "round")
    wf = wd.flip(2, 3).transpose(0, 1).contiguous()  # the dgrad as a forward conv of dy
    full = emu_store(emu_conv(_stage(dy.float()), wf), "bf16")
    assert torch.equal(full[:, :c0], _bits(dx[:, :c0], "bf16")) and torch.equal(full[:, c0:], _bits(dx[:, c0:], "bf16"))
    off = c0 + 8  # n_split off by 8: the second output starts 8 channels late, its last 8 columns stay NaN
    ds = torch.full((B, c1, H, W), float("nan"), dtype=BF)
    ds[:, :c1 - 8] = full[:, off:]
    assert not torch.equal(ds, _bits(dx[:, c0:], "bf16"))
    assert not torch.equal(full[:, 8:off], _bits(dx[:, :c0], "bf16"))


def test_relu_mask_at_zero_fails():
    """z >= 0 instead of z > 0 in the BatchNorm-backward mask: differs exactly where the lattice plants z == 0."""
    S, bb, dw = T._bnbwd_case(2, 10, 14, (32,), 64)
    v = lambda t: t.float().view(1, -1, 1, 1)  # noqa: E731
    y, da = bb.y.float(), bb.da.float()
    z = torch.addcmul(v(bb.shift), y, v(bb.scale))
    xhat = (y - v(bb.mean)) * v(bb.invstd)
    for ge in (False, True):
        dz = torch.where((z >= 0) if ge else (z > 0), da, torch.zeros_like(da))
        dy = _stage(v(bb.coef[:, 0]) * (dz - v(bb.coef[:, 1]) - xhat * v(bb.coef[:, 2])))
        ok = torch.equal(dy.to(BF), _bits(bb.dy, "bf16")) and torch.equal(emu_wgrad(emu_source(S), dy), _bits(dw, "fp32"))
        assert ok == (not ge)


def test_convT_transposed_phases_and_ignored_lo_half_fail():
    B, h, w_, ci, co = 2, 5, 7, 32, 16
    S, wt, bias, out, dout, dx = T._convT_case(B, h, w_, ci, co, True)
    x = emu_source(S)

    def fwd(wq, transpose):
        acc = torch.zeros(B, co, 2 * h, 2 * w_)
        for a in range(2):
            for b in range(2):
                t = torch.einsum("bihw,io->bohw", x, wq[:, :, a, b])
                if transpose:
                    acc[:, :, b::2, a::2] = t
                else:
                    acc[:, :, a::2, b::2] = t
        return acc + bias.float().view(1, -1, 1, 1)

    assert torch.equal(fwd(wt.float(), False).to(BF), _bits(out, "bf16"))
    assert not torch.equal(fwd(wt.float(), True).to(BF), _bits(out, "bf16"))
    S, ws, bias, out = T._convT_case(2, 12, 20, 64, 32, True, True)
    x = emu_source(S)
    B, h, w_, co = 2, 12, 20, 32
    hi, lo = (t.float() for t in R.split_hi_lo(ws))
    assert torch.equal((fwd(hi, False) + (fwd(lo, False) - bias.float().view(1, -1, 1, 1))).to(BF), _bits(out, "bf16"))
    assert not torch.equal(fwd(hi, False).to(BF), _bits(out, "bf16"))
    # the same for the 3x3 split conv
    S, w3, out3 = T._fwd_case(1, 32, 64, (32,), 32, (True,), False, "round", True)
    hi, lo = R.split_hi_lo(w3)
    x3 = emu_source(S)
    assert torch.equal((emu_conv(x3, hi) + emu_conv(x3, lo)).to(BF), _bits(out3, "bf16"))
    assert not torch.equal(emu_conv(x3, hi).to(BF), _bits(out3, "bf16"))
