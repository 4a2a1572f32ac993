"""Lattice inputs and float64 statements for the conv, ConvTranspose and weight-gradient kernels (CPU only).

The inputs live on a lattice (small integers times powers of two) chosen so that every product, every partial sum in
any order and every value a kernel stages in bf16 is exactly representable. A correct kernel then produces the float64
result exactly in fp32 mode and its round-to-nearest-even bf16 in bf16 mode, at every element, whatever its summation
order, split-K plan, MFMA shape or block assignment: the comparisons need no tolerance, and anything dropped, doubled
or taken from the wrong neighbour is a wrong integer.

The exactness conditions are asserted here (require_*), per case, before anything is compared. They are conditions,
not measurements: a case that breaks one gets a smaller amplitude (fit()), never a relaxed check.

numpy / torch float64 only; no project code is imported. Tensors are NCHW as in PyTorch.
"""

import numpy as np
import torch

F64 = torch.float64
LIMIT = float(2 ** 24)  # integers below it are exact in fp32, and so is every partial sum of terms whose |.| sum is


class LatticeError(AssertionError):
    """An exactness condition does not hold for a case (fit() then tries the next smaller amplitude)."""


# ------------------------------------------------------------------------------------------------ number formats
def _f32_bits(x):
    f = x.to(torch.float32)
    if not torch.equal(f.double(), x.double()):
        raise LatticeError("value not exactly representable in fp32")
    return f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(b):
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(torch.float32).double()


def rne_bf16(x):
    """Round-to-nearest-even bf16 of fp32-exact float64 values, on the integer bit pattern; returned as float64."""
    b = _f32_bits(x)
    return _from_bits(((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16)


def trunc_bf16(x):
    """bf16 by truncation toward zero (the defect a store without rounding has)."""
    return _from_bits(_f32_bits(x) & 0xFFFF0000)


def is_bf16(x):
    return bool(torch.equal(rne_bf16(x), x.double()))


def expected(x, prec):
    """The bits a correct kernel stores for the exact float64 result x: fp32 -> x itself, bf16 -> RNE_bf16(x)."""
    if prec == "fp32":
        _f32_bits(x)
        return x.to(torch.float32)
    r = rne_bf16(x)
    out = r.to(torch.bfloat16)
    assert torch.equal(out.double(), r)
    return out


def rounding_share(x):
    """Share of elements where truncation toward zero and RNE give different bf16 values."""
    return float((trunc_bf16(x) != rne_bf16(x)).double().mean())


def step_of(*tensors):
    """The lattice step: the largest power of two that every non-zero element is an integer multiple of."""
    lo = None
    for t in tensors:
        v = t.detach().double().reshape(-1).numpy()
        v = v[v != 0]
        if v.size == 0:
            continue
        m, e = np.frexp(np.abs(v))
        mi = (m * 2.0 ** 53).astype(np.int64)
        low = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
        k = int((e.astype(np.int64) - 53 + low).min())
        lo = k if lo is None else min(lo, k)
    return 2.0 ** (0 if lo is None else lo)


# ------------------------------------------------------------------------------------------------ conditions
def require_bf16(x, what):
    """A value a kernel stages or stores in bf16 before the final output round-trips unchanged."""
    if not is_bf16(x):
        raise LatticeError(f"{what}: not exactly representable in bf16")


def require_sum_exact(abs_sum, step, what):
    """sum |term| < 2^24 lattice steps, over the full sum (abs_sum: that sum per output, in float64): every partial
    sum in every order is then an exact fp32 value."""
    m = float(abs_sum.abs().max()) / step if abs_sum.numel() else 0.0
    if not m < LIMIT:
        raise LatticeError(f"{what}: sum |term| = {m:.4g} steps >= 2^24")


def require_rounding(x, what):
    """The bf16 store's rounding is exercised: truncation differs from RNE on more than a tenth of the elements."""
    s = rounding_share(x)
    if not s > 0.1:
        raise LatticeError(f"{what}: truncation differs from RNE on {s:.3f} of the elements only")


def fit(build, ladder):
    """build(amp) for the first amplitude of the (descending) ladder whose exactness conditions hold."""
    err = None
    for amp in ladder:
        try:
            out = build(amp)
            fit.last = amp  # the rung taken (for reports)
            return out
        except LatticeError as e:
            err = e
    raise AssertionError(f"no amplitude of {ladder} satisfies the lattice conditions: {err}")


# ------------------------------------------------------------------------------------------------ generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, amp):
    return torch.randint(-amp, amp + 1, shape, generator=g).to(F64)


def acts(B, C, H, W, seed, amp=8, zero_window=True, spikes=0):
    """Integer activations / upstream gradients, |v| <= amp. The interior stays below amp - 1; the first and last row
    and column carry +-(amp - 1) only and the four corners +-amp with a sign pattern of their own, so a value taken
    from the wrong side, the wrong row or across the image edge changes the result; one 5x5 block is zero in every
    channel (an all-zero 3x3 window); no two adjacent rows, columns or channels are equal (asserted).
    spikes (an amplitude, for grids of at least 16 pixels): six single pixels carry, in up to 16 channels, integers with
    spikes/2 <= |v| <= spikes. The low-amplitude lattices that keep sums of squares over many pixels exact get them so
    that some outputs of every channel still need more than 8 bits and the bf16 store rounds them."""
    assert amp >= 3
    g = _gen(seed)
    x = _ints(g, (B, C, H, W), amp - 2)
    edge = (torch.randint(0, 2, (B, C, H, W), generator=g).to(F64) * 2 - 1) * (amp - 1)
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    x = torch.where(m, edge, x)
    if spikes and H * W >= 16:
        ch = torch.randperm(C, generator=g)[:16]
        for k in range(6):
            i = int(torch.randint(0, H, (1,), generator=g)) if H < 4 else int(torch.randint(1, H - 1, (1,), generator=g))
            j = int(torch.randint(0, W, (1,), generator=g)) if W < 4 else int(torch.randint(1, W - 1, (1,), generator=g))
            mag = torch.randint(spikes // 2, spikes + 1, (len(ch),), generator=g).to(F64)
            x[k % B, ch, i, j] = mag * (torch.randint(0, 2, (len(ch),), generator=g).to(F64) * 2 - 1)
    c = torch.arange(C)
    for k, (i, j) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        x[:, :, i, j] = (1.0 - 2.0 * ((c >> k) & 1).to(F64)) * amp * (1 if k % 2 == 0 else -1)
    if zero_window and H >= 9 and W >= 9:
        x[:, :, 2:7, 2:7] = 0.0
    # adjacent slices differ: bump one interior (or only) element where a draw made two equal
    for d in (1, 2, 3):
        n = x.shape[d]
        for i in range(n - 1):
            if torch.equal(x.select(d, i), x.select(d, i + 1)):
                at = [0, 0, 0, 0]
                at[d] = i + 1
                x[tuple(at)] += 1.0 if float(x[tuple(at)]) < amp else -1.0
        for i in range(n - 1):
            assert not torch.equal(x.select(d, i), x.select(d, i + 1)), ("adjacent slices equal", d, i)
    assert float(x.abs().max()) <= max(amp, spikes)
    return x


def weights(shape, seed, amp=4, exp=-3, density=1.0):
    """Integer weights |w| <= amp times 2^exp (density < 1: that share of them kept, the rest zero); every (input channel, tap) pair has a non-zero weight for at least one
    output channel (asserted). shape: [co][ci][kh][kw] (Conv2d) or [ci][co][kh][kw] (ConvTranspose2d): the check covers
    both since it runs over both channel axes."""
    g = _gen(seed)
    w = _ints(g, shape, amp)
    if density < 1.0:
        w = w * (torch.rand(shape, generator=g) < density).to(F64)
    for ax in (0, 1):
        dead = (w != 0).sum(ax, keepdim=True) == 0
        if bool(dead.any()):
            idx = [slice(None)] * 4
            idx[ax] = slice(0, 1)
            w[tuple(idx)] = torch.where(dead, torch.ones_like(w[tuple(idx)]), w[tuple(idx)])
        assert bool(((w != 0).sum(ax) > 0).all())
    return w * 2.0 ** exp


def split_weights(shape, seed, amp=4, exp=-3):
    """fp32 weights a + b * 2^-9 (a a non-zero small integer, b in {-1, 0, 1}, times 2^exp): |b| * 2^-9 stays below
    half a bf16 ulp of a, so the bf16 hi half is a and the lo half b * 2^-9, both exact, the lo half non-zero somewhere
    (asserted through split_hi_lo)."""
    a = weights(shape, seed, amp, 0)
    a = torch.where(a == 0, torch.ones_like(a), a)
    b = weights(shape, seed + 1, 1, 0)
    w = (a + b * 2.0 ** -9) * 2.0 ** exp
    hi, lo = split_hi_lo(w)
    assert torch.equal(hi, a * 2.0 ** exp) and torch.equal(lo, b * 2.0 ** (exp - 9)) and bool((lo != 0).any())
    return w


def split_hi_lo(w):
    """hi = RNE_bf16(w), lo = RNE_bf16(w - hi); on split_weights() both are exact and hi + lo == w."""
    hi = rne_bf16(w)
    lo = rne_bf16(w - hi)
    assert torch.equal(hi + lo, w.double())
    return hi, lo


def bn_affine(C, seed, small=False):
    """BN source transform: scale in {+-0.5, +-1, +-2} with every third channel negative, shift a multiple of 0.5,
    |shift| <= 2. small (the lattices reduced for sums of squares over many pixels): scale +-1, shift in {-1, 0, 1}."""
    g = _gen(seed)
    scale = 2.0 ** torch.randint(-1, 2, (C,), generator=g).to(F64)
    shift = torch.randint(-4, 5, (C,), generator=g).to(F64) * 0.5
    if small:
        scale, shift = torch.ones(C, dtype=F64), torch.randint(-1, 2, (C,), generator=g).to(F64)
    scale[::3] *= -1
    return scale, shift


def bn_stats(C, seed):
    """mean (small integers), invstd (powers of two)."""
    g = _gen(seed)
    return torch.randint(-2, 3, (C,), generator=g).to(F64), 2.0 ** torch.randint(-1, 2, (C,), generator=g).to(F64)


def bn_coef(scale, seed):
    """The [C][3] BatchNorm-backward coefficients: coef0 = scale, coef1 a small integer, coef2 in {0, +-0.5, +-1}."""
    g = _gen(seed)
    C = scale.numel()
    c1 = torch.randint(-2, 3, (C,), generator=g).to(F64)
    c2 = torch.randint(-2, 3, (C,), generator=g).to(F64) * 0.5
    return torch.stack([scale, c1, c2], 1).contiguous()


def out_affine(C, seed):
    """Output affine of sd_conv3x3_ex: power-of-two scale (some negative), small integer shift."""
    g = _gen(seed)
    sc = 2.0 ** torch.randint(-2, 2, (C,), generator=g).to(F64)
    sc[::5] *= -1
    return sc, torch.randint(-3, 4, (C,), generator=g).to(F64)


def int_bias(C, seed, amp=8):
    return _ints(_gen(seed), (C,), amp)


# ------------------------------------------------------------------------------------------------ statements
def _v(t):
    return t.view(1, -1, 1, 1)


def bn_relu(y, scale, shift):
    """x = max(scale*y + shift, 0), the per-source transform (z > 0 is false at z == 0)."""
    z = y * _v(scale) + _v(shift)
    return torch.where(z > 0, z, torch.zeros_like(z))


def pool2(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).amax((3, 5))


def _pad1(x):
    B, C, H, W = x.shape
    p = torch.zeros(B, C, H + 2, W + 2, dtype=x.dtype)
    p[:, :, 1:-1, 1:-1] = x
    return p


def conv3x3(x, w):
    """Conv2d(k3, p1, no bias): out[b,o,h,w] = sum_{i,kh,kw} x[b,i,h+kh-1,w+kw-1] * w[o,i,kh,kw]; a tap-outer loop."""
    B, C, H, W = x.shape
    p = _pad1(x.to(F64))
    out = torch.zeros(B, w.shape[0], H, W, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            out += torch.einsum("bihw,oi->bohw", p[:, :, kh:kh + H, kw:kw + W], w[:, :, kh, kw].to(F64))
    return out


def conv3x3_dgrad(dy, w):
    """dx[b,i,h,w] = sum_{o,kh,kw} dy[b,o,h-kh+1,w-kw+1] * w[o,i,kh,kw]."""
    B, C, H, W = dy.shape
    p = _pad1(dy.to(F64))
    out = torch.zeros(B, w.shape[1], H, W, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            out += torch.einsum("bohw,oi->bihw", p[:, :, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W], w[:, :, kh, kw].to(F64))
    return out


def conv3x3_wgrad(x, dy):
    """dw[o,i,kh,kw] = sum_{b,h,w} dy[b,o,h,w] * x[b,i,h+kh-1,w+kw-1]."""
    B, C, H, W = x.shape
    p = _pad1(x.to(F64))
    dw = torch.zeros(dy.shape[1], C, 3, 3, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = torch.einsum("bohw,bihw->oi", dy.to(F64), p[:, :, kh:kh + H, kw:kw + W])
    return dw


def convT(x, w, bias=None):
    """ConvTranspose2d(k2, s2): out[b,o,2h+a,2w+c] = sum_i x[b,i,h,w] * w[i,o,a,c] + bias[o]."""
    B, C, H, W = x.shape
    out = torch.zeros(B, w.shape[1], 2 * H, 2 * W, dtype=F64)
    for a in range(2):
        for c in range(2):
            out[:, :, a::2, c::2] = torch.einsum("bihw,io->bohw", x.to(F64), w[:, :, a, c].to(F64))
    return out if bias is None else out + _v(bias.to(F64))


def convT_dgrad(dout, w):
    """dx[b,i,h,w] = sum_{o,a,c} dout[b,o,2h+a,2w+c] * w[i,o,a,c]."""
    B, C, H2, W2 = dout.shape
    dx = torch.zeros(B, w.shape[0], H2 // 2, W2 // 2, dtype=F64)
    for a in range(2):
        for c in range(2):
            dx += torch.einsum("bohw,io->bihw", dout[:, :, a::2, c::2].to(F64), w[:, :, a, c].to(F64))
    return dx


def convT_wgrad(x, dout):
    """dw[i,o,a,c] = sum_{b,h,w} x[b,i,h,w] * dout[b,o,2h+a,2w+c]; the bias gradient is chan_sums(dout)[0]."""
    dw = torch.zeros(x.shape[1], dout.shape[1], 2, 2, dtype=F64)
    for a in range(2):
        for c in range(2):
            dw[:, :, a, c] = torch.einsum("bihw,bohw->io", x.to(F64), dout[:, :, a::2, c::2].to(F64))
    return dw


def chan_sums(v):
    """Per-channel (sum, sum of squares) of the stored values v: [C][2] (STATS; column 0 is a bias gradient)."""
    v = v.to(F64)
    return torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))], 1)


def bn_bwd_dy(da, y, scale, shift, mean, invstd, coef):
    """BatchNorm-backward apply: dz = da where scale*y + shift > 0 else 0; xhat = (y - mean) * invstd;
    dy = coef0 * (dz - coef1 - xhat * coef2)."""
    z = y * _v(scale) + _v(shift)
    dz = torch.where(z > 0, da, torch.zeros_like(da))
    xhat = (y - _v(mean)) * _v(invstd)
    return _v(coef[:, 0]) * (dz - _v(coef[:, 1]) - xhat * _v(coef[:, 2]))


def bn_bwd_sums(dx, y, scale, shift, mean, invstd):
    """The BatchNorm-backward sums over (dx, y): [C][2] = (sum dz, sum dz * xhat), dz = dx where scale*y + shift > 0."""
    z = y * _v(scale) + _v(shift)
    dz = torch.where(z > 0, dx, torch.zeros_like(dx))
    xhat = (y - _v(mean)) * _v(invstd)
    return torch.stack([dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))], 1)


def require_bn_sums_exact(dx, y, scale, shift, mean, invstd, what):
    z = y * _v(scale) + _v(shift)
    dz = torch.where(z > 0, dx, torch.zeros_like(dx)).abs()
    xhat = ((y - _v(mean)) * _v(invstd)).abs()
    require_sum_exact(dz.sum((0, 2, 3)), step_of(dx), what + " sum dz")
    require_sum_exact((dz * xhat).sum((0, 2, 3)), step_of(dx) * step_of(xhat), what + " sum dz*xhat")
    require_sum_exact(z.abs().amax(), step_of(z), what + " z")


def require_stats_rounding(out, what, every_channel=True):
    """STATS are of the stored bf16 values: in every channel the sum or the sum of squares of the stored values differs
    from that of the exact (accumulator) values, so statistics taken from the fp32 accumulator fail in every channel
    (every_channel=False: in some channel, for the cases where no amplitude of the ladder reaches every channel)."""
    a, b = chan_sums(out), chan_sums(rne_bf16(out))
    same = (a[:, 0] == b[:, 0]) & (a[:, 1] == b[:, 1])
    if bool(same.any()) if every_channel else bool(same.all()):
        raise LatticeError(f"{what}: in {int(same.sum())} channels the stored values' sums equal the accumulator's")


def require_stats_exact(v, what):
    s = step_of(v)
    require_sum_exact(v.abs().sum((0, 2, 3)), s, what + " sum")
    require_sum_exact((v * v).sum((0, 2, 3)), s * s, what + " sum of squares")


# ------------------------------------------------------------------------------------------------ sources
class Source:
    """One or two NCHW tensors concatenated along channels, each raw or BN+ReLU, optionally 2x2 max-pooled after the
    transform: what sd_src describes. parts: list of (y, (scale, shift) or None)."""

    def __init__(self, parts, pool=False):
        self.parts, self.pool = parts, pool

    def x(self):
        """The operand the convolution multiplies (float64), each transformed part asserted bf16-exact and the
        transform's fp32 intermediates exact."""
        xs = []
        for y, bn in self.parts:
            v = y.to(F64)
            require_bf16(v, "source")
            if bn is not None:
                z = v * _v(bn[0]) + _v(bn[1])
                require_sum_exact(z.abs().amax(), step_of(z, v * _v(bn[0])), "source transform")
                v = bn_relu(v, *bn)
            if self.pool:
                v = pool2(v)
            require_bf16(v, "transformed source")
            xs.append(v)
        return torch.cat(xs, 1)

    def zeros_at_relu(self):
        """Number of pre-activation values exactly at 0 (where z > 0 must be false)."""
        return sum(int(((y * _v(bn[0]) + _v(bn[1])) == 0).sum()) for y, bn in self.parts if bn is not None)


def make_source(B, chans, H, W, seed, amp=8, bn=(), pool=False, spikes=0):
    """Source over len(chans) tensors; bn: per part True (BN+ReLU) / False (raw). H, W: the conv grid (a pooled
    source is stored at 2H x 2W)."""
    bn = tuple(bn) + (False,) * (len(chans) - len(bn))
    Hs, Ws = (2 * H, 2 * W) if pool else (H, W)
    parts = []
    for k, c in enumerate(chans):
        y = acts(B, c, Hs, Ws, seed + 10 * k, amp, spikes=spikes)
        parts.append((y, bn_affine(c, seed + 10 * k + 1, small=amp <= 4) if bn[k] else None))
    return Source(parts, pool)


def conv_case(src, w, what="conv3x3", rounding=False, stats=False, stats_round=None):
    """The exact forward result of conv3x3(src.x(), w) with its exactness conditions asserted; rounding / stats add the
    conditions for the bf16 store's rounding share and for the STATS sums of the stored bf16 values."""
    x = src.x()
    require_bf16(w, what + " weights")
    out = conv3x3(x, w)
    require_sum_exact(conv3x3(x.abs(), w.abs()), step_of(x) * step_of(w), what)
    if rounding:
        require_rounding(out, what)
    if stats:  # the bf16 path sums the stored values, the fp32 path the values themselves
        require_stats_exact(rne_bf16(out), what + " STATS")
        require_stats_exact(out, what + " STATS (fp32)")
    if stats_round is not None:
        require_stats_rounding(out, what + " STATS", stats_round)
    return x, out


def dgrad_case(dy, w, what="dgrad", rounding=False, stats=False, stats_round=None):
    """conv3x3_dgrad(dy, w) with its conditions; dy: the staged upstream gradient (bf16-exact)."""
    require_bf16(dy, what + " dy")
    require_bf16(w, what + " weights")
    dx = conv3x3_dgrad(dy, w)
    require_sum_exact(conv3x3_dgrad(dy.abs(), w.abs()), step_of(dy) * step_of(w), what)
    if rounding:
        require_rounding(dx, what)
    if stats:
        require_stats_exact(rne_bf16(dx), what + " STATS")
        require_stats_exact(dx, what + " STATS (fp32)")
    if stats_round is not None:
        require_stats_rounding(dx, what + " STATS", stats_round)
    return dx


def wgrad_case(x, dy, what="wgrad"):
    """conv3x3_wgrad(x, dy) with its conditions (x: the transformed operand of Source.x(), dy bf16-exact)."""
    require_bf16(dy, what + " dy")
    dw = conv3x3_wgrad(x, dy)
    require_sum_exact(conv3x3_wgrad(x.abs(), dy.abs()), step_of(x) * step_of(dy), what)
    return dw


class BnBwd:
    """The operands of a fused BatchNorm-backward apply over C channels: da, y (integers), the layer's forward
    coefficients and its [C][3] backward coefficients; dy = bn_bwd_dy(...) asserted bf16-exact with every intermediate
    on the lattice, and some pre-activations exactly 0 (the mask z > 0 is false there)."""

    def __init__(self, B, C, H, W, seed, amp=8):
        self.da = acts(B, C, H, W, seed, amp)
        self.y = acts(B, C, H, W, seed + 1, 8, zero_window=False)
        self.scale, self.shift = bn_affine(C, seed + 2)
        self.mean, self.invstd = bn_stats(C, seed + 3)
        self.coef = bn_coef(self.scale, seed + 4)
        self.dy = bn_bwd_dy(self.da, self.y, self.scale, self.shift, self.mean, self.invstd, self.coef)
        require_bf16(self.dy, "BatchNorm-backward dy")
        z = self.y * _v(self.scale) + _v(self.shift)
        xh = (self.y - _v(self.mean)) * _v(self.invstd)
        t = xh * _v(self.coef[:, 2])
        bound = self.da.abs() + _v(self.coef[:, 1]).abs() + t.abs() + z.abs() + xh.abs()
        require_sum_exact(bound.amax() * _v(self.scale).abs().amax(), step_of(self.dy, z, xh, t), "BatchNorm-backward apply")
        self.relu_zeros = int((z == 0).sum())
        assert self.relu_zeros > 0, "no pre-activation exactly at 0"

    def params(self):
        return (self.scale, self.shift, self.mean, self.invstd, self.coef)


def convT_case(x, w, bias, what="convT", rounding=False):
    require_bf16(x, what + " source")
    require_bf16(w, what + " weights")
    out = convT(x, w, bias)
    ab = convT(x.abs(), w.abs(), bias.abs())
    require_sum_exact(ab, min(step_of(x) * step_of(w), step_of(bias)), what)
    if rounding:
        require_rounding(out, what)
    return out


def convT_dgrad_case(dout, w, what="convT dgrad", rounding=False):
    require_bf16(dout, what + " dout")
    dx = convT_dgrad(dout, w)
    require_sum_exact(convT_dgrad(dout.abs(), w.abs()), step_of(dout) * step_of(w), what)
    if rounding:
        require_rounding(dx, what)
    return dx


def convT_wgrad_case(x, dout, what="convT wgrad"):
    dw = convT_wgrad(x, dout)
    require_sum_exact(convT_wgrad(x.abs(), dout.abs()), step_of(x) * step_of(dout), what)
    require_sum_exact(dout.abs().sum((0, 2, 3)), step_of(dout), what + " bias")
    return dw, dout.sum((0, 2, 3))


# ------------------------------------------------------------------------------------------------ packed layouts
def pack_conv3(w, ci_pad, dgrad, kpad):
    """sd_pack_conv3_w: fwd [co][kpad], k = tap*ci_pad + ci; dgrad [ci][kpad], k = tap*co + o of W[o][ci][8 - tap];
    zero elsewhere."""
    co, ci = w.shape[:2]
    wt = w.reshape(co, ci, 9)
    if not dgrad:
        out = torch.zeros(co, kpad, dtype=F64)
        v = torch.zeros(co, 9, ci_pad, dtype=F64)
        v[:, :, :ci] = wt.permute(0, 2, 1)
        out[:, :9 * ci_pad] = v.reshape(co, -1)
        return out
    out = torch.zeros(ci, kpad, dtype=F64)
    out[:, :9 * co] = wt.flip(2).permute(1, 2, 0).reshape(ci, -1)
    return out


def pack_convT(w, dgrad, kpad):
    """sd_pack_convT_w: fwd [(t, o)][kpad], k = i; dgrad [ci][kpad], k = t*co + o (t = 2a + c)."""
    ci, co = w.shape[:2]
    wt = w.reshape(ci, co, 4)
    if not dgrad:
        out = torch.zeros(4 * co, kpad, dtype=F64)
        out[:, :ci] = wt.permute(2, 1, 0).reshape(4 * co, ci)
        return out
    out = torch.zeros(ci, kpad, dtype=F64)
    out[:, :4 * co] = wt.permute(0, 2, 1).reshape(ci, -1)
    return out


def pack_conv3_split(w, ci_pad, kpad):
    """SD_PACK_CONV3_FWD_SPLIT: [co][kpad], k = tap*2*ci_pad + {ci: hi | ci_pad + ci: lo}."""
    co, ci = w.shape[:2]
    hi, lo = split_hi_lo(w)
    v = torch.zeros(co, 9, 2, ci_pad, dtype=F64)
    v[:, :, 0, :ci] = hi.reshape(co, ci, 9).permute(0, 2, 1)
    v[:, :, 1, :ci] = lo.reshape(co, ci, 9).permute(0, 2, 1)
    out = torch.zeros(co, kpad, dtype=F64)
    out[:, :18 * ci_pad] = v.reshape(co, -1)
    return out


def pack_convT_split(w, kpad):
    """SD_PACK_CONVT_FWD_SPLIT: [(t, o)][kpad], k = {i: hi | ci + i: lo}."""
    ci, co = w.shape[:2]
    hi, lo = split_hi_lo(w)
    out = torch.zeros(4 * co, kpad, dtype=F64)
    out[:, :ci] = hi.reshape(ci, co, 4).permute(2, 1, 0).reshape(4 * co, ci)
    out[:, ci:2 * ci] = lo.reshape(ci, co, 4).permute(2, 1, 0).reshape(4 * co, ci)
    return out
