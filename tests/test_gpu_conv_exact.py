"""The conv, ConvTranspose and weight-gradient kernels bit for bit against float64 (needs an MI355X).

Inputs come from the lattice of tests/conv_lattice_ref.py: every product, every partial sum in any order and every
value a kernel stages in bf16 is exactly representable (the conditions are asserted by the reference for each case
before anything is compared). A correct kernel then stores the float64 result itself in fp32 mode and its
round-to-nearest-even bf16 in bf16 mode, at every element: every comparison below is torch.equal on the expected bits,
over every element (shape and dtype included), with the output buffers pre-filled with NaN. Summation order, split-K
plans, MFMA shapes and block assignment do not matter; a product dropped, doubled, misplaced or taken from the wrong
neighbour is a wrong integer.

Amplitudes: each case takes the largest (activation, weight) amplitude pair of a fixed ladder for which the
reference's conditions hold. Where the bf16 store is checked the conditions include that truncation toward zero would
differ from RNE on more than a tenth of the elements; where sums of squares over many pixels must stay below 2^24
steps (STATS, the BatchNorm-backward sums) the ladder goes down to {-1, 0, 1} interiors. Those low lattices would leave
every output within 8 bits, and STATS taken from the fp32 accumulator instead of the stored value would pass; so the
STATS lattices plant six high pixels, and it is a condition of each STATS case that in every output channel the sum or
the sum of squares of the stored values differs from the accumulator's. One case cannot meet it in every channel: at
2 x 128 x 640 pixels 2^24 leaves about 100 steps^2 a pixel, which only the sparse {-1, 0, 1} weights meet, and with
8 input channels few of their outputs pass 256 steps; there the condition holds in some channels (the same instance is
held to it in every channel at 2 x 32 x 64). Grids below 16 pixels have no room for the pixels. With hi/lo split weights the
terms sit 2^-9 below the hi lattice and no amplitude keeps the sums of squares exact: there the STATS launch's stored
output is compared and the sums are pinned by the plain-weight launch of the same shape.

Each variant selected by a per-call switch (SD_HALO_CK, SD_HALO_N32, SD_HALO_RAW, SD_WG_X8, SD_WS_MF32, SD_WS_CO128,
SD_FWD_BM, SD_CONVT_KMAX) is compared with the float64 bits, not with its sibling. test_gpu_ops.py keeps the fp32
CPU-PyTorch parity and the variant-equals-variant checks on random data.
"""

import functools

import pytest
import torch

import conv_lattice_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
AMPS = ((32, 16), (16, 8), (8, 4))  # (activation, weight) amplitudes where the bf16 store must round visibly
# down to {-1, 0, 1} interiors, and last a quarter of the weights non-zero: sums of squares over many pixels
AMPS_SUM = AMPS + ((4, 2), (3, 1), (3, 0))


def _weights(shape, seed, amp, exp, split=False):
    if split:
        return R.split_weights(shape, seed, max(amp, 1), exp)
    return R.weights(shape, seed, amp, exp) if amp else R.weights(shape, seed, 1, exp, density=0.25)


COMPARED = [0, 0]  # comparisons made and elements compared by this module's tests (printed by the last test)


def _same(got, want):
    """torch.equal on the expected bits, over every element; counted."""
    COMPARED[0] += 1
    COMPARED[1] += want.numel()
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def _stats_ladder(npix=0):
    """(activation, weight, spike) amplitudes of the STATS lattices: each base pair with spikes of 60 (the largest
    whose BN transform 2*y + 2 stays within 8 bits of half steps; 250 on the {-1, 0, 1} lattices, whose transform is
    +-y + shift), then 30 and 15. The whole ladder first with the rounding condition on every output channel, then, for
    the cases where no rung reaches every channel, on some channel."""
    one = tuple((a, w, sp) for a, w in AMPS_SUM for sp in ((250, 120, 60) if a < 5 else (60, 30, 15)))
    if npix > 2 ** 16:  # 2^24 / npix leaves about 100 steps^2 a pixel: only the {-1, 0, 1} rungs can meet it
        one = tuple(r for r in one if r[0] == 3 and r[2] == 250)
    return tuple(r + (True,) for r in one) + tuple(r + (False,) for r in one)


def _tiny(H, W):
    """Grids of at most 4 pixels hold corner values only (multiples of the amplitude): their outputs are coarse and
    bf16-exact, so the rounding-share condition is not asked of them (they are there for the image edges)."""
    return H * W < 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def L():
    from stereo_depth_estimation_amd import _lib

    return _lib


def _adt(prec):
    return torch.float32 if prec == "fp32" else torch.bfloat16


def _sd(prec):
    return L().SD_F32 if prec == "fp32" else L().SD_BF16


def _rows(t):
    """NCHW float64 -> [B*H*W][C] (the kernels' NHWC rows)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _dev(t, prec):
    """A lattice tensor on the device in the path's dtype (exact: asserted by R.expected)."""
    return R.expected(_rows(t), prec).to(DEV)


def _want(t, prec):
    return R.expected(_rows(t), prec)


def _f32(t):
    return R.expected(t.contiguous(), "fp32").to(DEV)


def _nan(rows, cols, prec):
    return torch.full((rows, cols), NAN, dtype=_adt(prec), device=DEV)


def _src(S, H, W, prec, taps=9):
    """sd_src of a reference Source (one or two parts, raw or BN+ReLU, optionally pooled)."""
    lib = L()
    Hs, Ws = (2 * H, 2 * W) if S.pool else (H, W)
    t = [_dev(y, prec) for y, _ in S.parts]
    bn = [None if b is None else (_f32(b[0]), _f32(b[1])) for _, b in S.parts]
    ch = [y.shape[1] for y, _ in S.parts]
    if len(t) == 1:
        return lib.make_src(t[0], ch[0], Hs, Ws, taps=taps, pool=S.pool, bn0=bn[0])
    return lib.make_src(t[0], ch[0], Hs, Ws, taps=taps, pool=S.pool, bn0=bn[0], src1=t[1], c1=ch[1], bn1=bn[1])


def _kpad(k):
    return (k + 63) // 64 * 64


def _pack3(w, ci_pad, dgrad, prec):
    lib = L()
    co, ci = w.shape[:2]
    kpad = _kpad(9 * (co if dgrad else ci_pad))
    out = torch.full(((ci if dgrad else co) * kpad,), NAN, dtype=_adt(prec), device=DEV)
    wd = _f32(w)
    lib.call("sd_pack_conv3_w", _sd(prec), wd.data_ptr(), co, ci, ci_pad, int(dgrad), kpad, out.data_ptr(), lib.stream_handle())
    return out, kpad


def _packT(w, dgrad, prec):
    lib = L()
    ci, co = w.shape[:2]
    kpad = _kpad(4 * co if dgrad else ci)
    out = torch.full(((ci if dgrad else 4 * co) * kpad,), NAN, dtype=_adt(prec), device=DEV)
    wd = _f32(w)
    lib.call("sd_pack_convT_w", _sd(prec), wd.data_ptr(), ci, co, int(dgrad), kpad, out.data_ptr(), lib.stream_handle())
    return out, kpad


def _pack_job(w, kind, co, ci, ci_pad, kpad, rows):
    lib = L()
    out = torch.full((rows * kpad,), NAN, dtype=torch.bfloat16, device=DEV)
    wd = _f32(w)
    job = (lib.SdPackJob * 1)(lib.SdPackJob(wd.data_ptr(), kind, co, ci, ci_pad, kpad, 0))
    lib.call("sd_pack_weights", lib.SD_BF16, job, 1, out.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    return out


LAUNCHED = set()  # bf16 instance names, added where the launch is made
RAN = [0]  # tests of this module run so far


@pytest.fixture(autouse=True)
def _count_run():
    RAN[0] += 1


def _conv_gemm(prec, src, B, H, W, wp, N, kpad, epi, out0, out1=None, n_split=0, bias=None, stats=None):
    lib = L()
    if prec == "bf16":
        LAUNCHED.add(lib.kernel_name("sd_conv_gemm_kernel_name", lib.SD_BF16, src, B, H, W, N, epi))
    lib.call("sd_conv_gemm", _sd(prec), src, B, H, W, wp.data_ptr(), N, kpad, epi, out0.data_ptr(), lib.ptr(out1),
             n_split, lib.ptr(bias), lib.ptr(stats), lib.stream_handle())
    torch.cuda.synchronize()


def _stat_sums(stats):
    """[rows][C][2] fp32 partial rows -> [C][2] float64 (each row an exact fp32 value on the lattice)."""
    return stats.double().sum(0).cpu()


# ----------------------------------------------------------------------------------------------- forward cases
@functools.lru_cache(maxsize=4)
def _fwd_case(B, H, W, chans, co, bn, pool, kind, split=False, affine=None):
    """(Source, weights, exact output) on the first amplitude whose conditions hold; kind "round": the bf16 store's
    rounding share is a condition, "stats": the STATS sums' exactness is. split: fp32 weights a + b * 2^-9 (hi/lo
    pairs). affine (a seed): also the output affine and acc*scale + shift, which the store then rounds."""
    def build(amp):
        sp = amp[2] if kind == "stats" and not split else 0
        S = R.make_source(B, chans, H, W, 100 + H + W, amp[0], bn=bn, pool=pool, spikes=sp)
        w = _weights((co, sum(chans), 3, 3), 7 + co, amp[1], -3, split)
        if split:
            hi, lo = R.split_hi_lo(w)
            R.conv_case(S, hi, "hi half")
            R.conv_case(S, lo, "lo half")
            x = S.x()
            out = R.conv3x3(x, w)
            R.require_sum_exact(R.conv3x3(x.abs(), w.abs()), R.step_of(x) * R.step_of(w), "split conv")
            R.require_rounding(out, "split conv")
        else:
            _, out = R.conv_case(S, w, rounding=kind == "round" and not _tiny(H, W), stats=kind == "stats",
                                 stats_round=amp[3] if kind == "stats" and H * W > 15 else None)
        if affine is None:
            return S, w, out
        aff = R.out_affine(co, affine)
        z = out * aff[0].view(1, -1, 1, 1) + aff[1].view(1, -1, 1, 1)
        R.require_sum_exact(out.abs().amax() * aff[0].abs().amax() + aff[1].abs().amax(), R.step_of(z, out), "output affine")
        R.require_rounding(z, "output affine")
        return S, w, z, aff

    return R.fit(build, _stats_ladder(B * H * W) if kind == "stats" and not split else AMPS_SUM if split else AMPS)


# the shapes of test_gpu_ops.py::test_conv3x3_fwd_with_bn_pool_gather_and_stats (each reaches one tiling or instance,
# see the comments there), plus H or W of 1 and 2, and batch 3 with odd sizes
FWD = [(2, 12, 20, 16, 32, False, False), (2, 8, 16, 32, 64, True, True), (1, 16, 16, 64, 128, False, True),
       (3, 6, 10, 24, 8, False, False), (2, 15, 20, 40, 128, False, True), (1, 30, 40, 64, 192, False, False),
       (1, 26, 50, 16, 64, True, True), (1, 9, 300, 8, 64, False, False), (1, 32, 64, 32, 32, False, True),
       (2, 128, 640, 8, 32, False, True), (2, 32, 64, 8, 32, False, True), (2, 30, 50, 8, 32, False, True),
       (1, 1, 1, 8, 32, False, True), (2, 2, 2, 16, 64, False, False), (1, 1, 40, 32, 32, False, True),
       (1, 33, 1, 16, 64, False, True), (3, 7, 11, 24, 64, False, True), (3, 5, 9, 8, 16, False, True),
       # a whole-image tile of more than 256 pixels (RT 3) with three chunks: the weights staged per chunk (bottleneck)
       (1, 15, 20, 96, 64, False, True)]


def _run_fwd(prec, B, H, W, chans, co, bn, pool, stats_too=True):
    lib = L()
    ci = sum(chans)
    S, w, out = _fwd_case(B, H, W, chans, co, bn, pool, "round")
    wp, kpad = _pack3(w, ci, False, prec)
    src = _src(S, H, W, prec)
    got = _nan(B * H * W, co, prec)
    _conv_gemm(prec, src, B, H, W, wp, co, kpad, lib.SD_EPI_STORE, got)
    assert _same(got.cpu(), _want(out, prec))
    if not stats_too or (prec == "bf16" and pool):  # bf16 pooled gather = generic kernel, STORE only
        return
    S, w, out = _fwd_case(B, H, W, chans, co, bn, pool, "stats")
    wp, kpad = _pack3(w, ci, False, prec)
    src = _src(S, H, W, prec)
    got = _nan(B * H * W, co, prec)
    rows = lib.call("sd_conv_gemm_stat_rows", _sd(prec), B, H, W, co)
    st = torch.full((rows, co, 2), NAN, device=DEV)
    _conv_gemm(prec, src, B, H, W, wp, co, kpad, lib.SD_EPI_STATS, got, stats=st)
    assert _same(got.cpu(), _want(out, prec))
    stored = out if prec == "fp32" else R.rne_bf16(out)
    assert _same(_stat_sums(st), R.chan_sums(stored))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,ci,co,pool,bn", FWD)
def test_conv3x3_fwd_store_and_stats(prec, B, H, W, ci, co, pool, bn):
    """sd_conv_gemm STORE and STATS on raw, BN+ReLU and pooled sources: the output is the float64 convolution (fp32) or
    its RNE bf16, the STATS rows sum to the float64 sum and sum of squares of the stored values."""
    _run_fwd(prec, B, H, W, (ci,), co, (bn,), pool)


# per-call switches: every variant against the float64 bits (shapes of test_conv3x3_halo_tilings_store_and_stats and
# test_conv3x3_raw_source_dma_loaders_bit_identical, the smallest of each group)
FWD_ENV = [({"SD_HALO_CK": "16"}, 1, 32, 64, (48,), 64, (True,)), ({"SD_HALO_CK": "16"}, 1, 45, 60, (24,), 64, (True,)),
           ({"SD_HALO_CK": "16"}, 2, 20, 30, (200,), 64, (True,)), ({"SD_HALO_CK": "16"}, 1, 36, 64, (72,), 64, (False,)),
           ({"SD_HALO_CK": "32"}, 1, 36, 64, (72,), 64, (True,)), ({"SD_HALO_CK": "32"}, 2, 20, 30, (200,), 64, (True,)),
           ({"SD_HALO_N32": "8"}, 1, 32, 64, (32,), 32, (True,)), ({"SD_HALO_N32": "8"}, 2, 32, 64, (8,), 32, (False,)),
           ({"SD_HALO_RAW": "0"}, 2, 24, 64, (64,), 64, (False,)), ({"SD_HALO_RAW": "1"}, 2, 24, 64, (64,), 64, (False,)),
           ({"SD_HALO_RAW": "0"}, 2, 40, 48, (32, 32), 64, (False, False)),
           ({"SD_HALO_RAW": "1"}, 2, 40, 48, (32, 32), 64, (False, False)),
           ({"SD_HALO_RAW": "1"}, 1, 30, 40, (160,), 256, (False,)), ({"SD_HALO_RAW": "1"}, 1, 15, 20, (96, 64), 512, (False, False)),
           ({"SD_HALO_RAW": "0"}, 1, 48, 64, (96,), 32, (False,)), ({"SD_HALO_RAW": "1"}, 1, 48, 64, (96,), 32, (False,))]


@pytest.mark.parametrize("env,B,H,W,chans,co,bn", FWD_ENV)
def test_conv3x3_fwd_halo_variants(monkeypatch, env, B, H, W, chans, co, bn):
    """The bf16 halo conv at every tiling and loader a per-call switch selects (CK = 16 tiles, 8x32 tiles at N = 32,
    register-staged against LDS-DMA loaders), STORE and STATS, each against the float64 bits."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _run_fwd("bf16", B, H, W, chans, co, bn, False)


# ----------------------------------------------------------------------------------------------- dual source, dgrad
DUAL = [(2, 8, 12, 16, 16, 16), (2, 15, 20, 64, 64, 64), (1, 16, 32, 8, 24, 32), (1, 16, 64, 24, 40, 64),
        (3, 7, 11, 8, 8, 64)]


@functools.lru_cache(maxsize=4)
def _dgrad_case(B, H, W, co, ci, kind):
    def build(amp):
        dy = R.acts(B, co, H, W, 200 + H, amp[0], spikes=amp[2] if kind == "stats" else 0)
        w = _weights((co, ci, 3, 3), 9 + ci, amp[1], -3)
        return dy, w, R.dgrad_case(dy, w, rounding=kind == "round", stats=kind == "stats",
                                   stats_round=amp[3] if kind == "stats" and H * W > 15 else None)

    return R.fit(build, AMPS if kind == "round" else _stats_ladder())


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,c0,c1,co", DUAL)
def test_conv3x3_dual_source_and_dgrad_split(prec, B, H, W, c0, c1, co):
    """cat([up, relu(bn(skip))]) forward, and the dgrad with the SPLIT epilogue (n_split at 8-channel boundaries that
    are not 16-channel ones among them); bf16 halo shapes also SPLIT_STATS, whose rows give the ConvTranspose2d bias
    gradient through sd_stat_rows_sum and through an SD_W_ROWSUM job of sd_wgrad_reduce_batch."""
    lib = L()
    _run_fwd(prec, B, H, W, (c0, c1), co, (False, True), False, stats_too=False)
    N = c0 + c1
    for kind in ("round", "stats"):
        sstats = kind == "stats"
        if sstats and not (prec == "bf16" and (N == 32 or N % 64 == 0)):
            continue
        dy, w, dx = _dgrad_case(B, H, W, co, N, kind)
        wd, kpd = _pack3(w, N, True, prec)
        dsrc = lib.make_src(_dev(dy, prec), co, H, W, taps=9)
        du, ds = _nan(B * H * W, c0, prec), _nan(B * H * W, c1, prec)
        st = None
        if sstats:
            rows = lib.call("sd_conv_gemm_stat_rows", lib.SD_BF16, B, H, W, N)
            st = torch.full((rows, N, 2), NAN, device=DEV)
        _conv_gemm(prec, dsrc, B, H, W, wd, N, kpd, lib.SD_EPI_SPLIT_STATS if sstats else lib.SD_EPI_SPLIT, du, ds, c0,
                   stats=st)
        assert _same(du.cpu(), _want(dx[:, :c0], prec))
        assert _same(ds.cpu(), _want(dx[:, c0:], prec))
        if sstats:
            sums = R.chan_sums(R.rne_bf16(dx))
            assert _same(_stat_sums(st), sums)
            bias = torch.full((c0,), NAN, device=DEV)
            lib.call("sd_stat_rows_sum", st.data_ptr(), rows, N, c0, bias.data_ptr(), lib.stream_handle())
            bias2 = torch.full((c0,), NAN, device=DEV)
            jobs = (lib.SdWredJob * 1)(lib.SdWredJob(st.data_ptr(), rows, 1, N, lib.SD_W_ROWSUM, c0, bias2.data_ptr()))
            lib.call("sd_wgrad_reduce_batch", jobs, 1, lib.stream_handle())
            torch.cuda.synchronize()
            want = R.expected(sums[:c0, 0].contiguous(), "fp32")
            assert _same(bias.cpu(), want) and _same(bias2.cpu(), want)


# ----------------------------------------------------------------------------------------------- weight gradients
def _wgrad(prec, a, b, B, H, W, M, N, layout, ci_real, dw_shape, bnb=None, batch_reduce=False):
    """sd_wgrad_gemm (or _bnbwd with bnb = (da, y, params)) into NaN-filled slabs, then the reduce: dw fp32 on CPU."""
    lib = L()
    s = lib.stream_handle()
    sp = lib.call("sd_wgrad_splits", _sd(prec), B, H, W, M, N)
    slab = torch.full((sp * M * N,), NAN, device=DEV)
    if bnb is None:
        if prec == "bf16":
            LAUNCHED.add(lib.kernel_name("sd_wgrad_kernel_name", lib.SD_BF16, a, b, M, N))
        lib.call("sd_wgrad_gemm", _sd(prec), a, b, B, H, W, M, N, slab.data_ptr(), sp, s)
    else:
        LAUNCHED.add(lib.kernel_name("sd_wgrad_bnbwd_kernel_name", a, b, M, N))
        lib.call("sd_wgrad_gemm_bnbwd", lib.SD_BF16, a, b, B, H, W, M, N, *[t.data_ptr() for t in bnb], slab.data_ptr(),
                 sp, s)
    dw = torch.full(dw_shape, NAN, device=DEV)
    if batch_reduce:
        jobs = (lib.SdWredJob * 1)(lib.SdWredJob(slab.data_ptr(), sp, M, N, layout, ci_real, dw.data_ptr()))
        lib.call("sd_wgrad_reduce_batch", jobs, 1, s)
    else:
        lib.call("sd_wgrad_reduce", slab.data_ptr(), sp, M, N, layout, ci_real, dw.data_ptr(), s)
    torch.cuda.synchronize()
    return dw.cpu()


@functools.lru_cache(maxsize=4)
def _wgrad_case(B, H, W, chans, co, bn):
    def build(amp):
        S = R.make_source(B, chans, H, W, 300 + H + W, amp, bn=bn)
        dy = R.acts(B, co, H, W, 301 + H, amp)
        return S, dy, R.wgrad_case(S.x(), dy)

    return R.fit(build, (8, 4, 3))


# the shapes of test_gpu_ops.py::test_conv3x3_wgrad (halo, warp-specialised, M = 32 groups: the smallest of each, the
# ragged ones kept), plus H or W of 1 and 2 and batch 3 with odd sizes
WGRAD = [(2, 10, 14, 24, 32), (2, 15, 20, 64, 64), (1, 13, 50, 16, 192), (1, 9, 300, 8, 64), (1, 30, 40, 40, 128),
         (2, 30, 40, 128, 64), (1, 13, 50, 64, 128), (3, 17, 33, 64, 64), (2, 12, 40, 32, 32), (1, 24, 64, 64, 32),
         (2, 15, 20, 32, 64), (1, 1, 1, 8, 32), (2, 2, 2, 16, 64), (1, 1, 40, 32, 32), (3, 5, 9, 8, 16)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,ci,co", WGRAD)
def test_conv3x3_wgrad_exact(prec, B, H, W, ci, co):
    """sd_wgrad_gemm + sd_wgrad_reduce (and the same through sd_wgrad_reduce_batch) on a raw x: every dW element is the
    float64 sum over every pixel."""
    lib = L()
    S, dy, dw = _wgrad_case(B, H, W, (ci,), co, (False,))
    a = lib.make_src(_dev(dy, prec), co, H, W, taps=1)
    b = _src(S, H, W, prec)
    want = R.expected(dw, "fp32")
    for batch_reduce in (False, True):
        got = _wgrad(prec, a, b, B, H, W, co, 9 * ci, lib.SD_W_CONV3, ci, (co, ci, 3, 3), batch_reduce=batch_reduce)
        assert _same(got, want)


# BN+ReLU x (the training path), concatenated x spanning a block, 128-row dy blocks, and the per-call switches
WGRAD_BN = [({}, 2, 30, 40, (64,), 64), ({}, 1, 15, 20, (128,), 128), ({}, 2, 10, 14, (32,), 64), ({}, 1, 24, 64, (32,), 32),
            ({}, 1, 16, 64, (64,), 32), ({}, 2, 24, 64, (32, 32), 32), ({}, 1, 20, 30, (32, 32), 64),
            ({}, 2, 16, 40, (32, 96), 32), ({}, 2, 17, 33, (64,), 128), ({}, 2, 20, 30, (32, 96), 128),
            ({"SD_WS_CO128": "0"}, 2, 17, 33, (64,), 128), ({"SD_WS_CO128": "0"}, 2, 20, 30, (32, 96), 128),
            ({"SD_WS_CO128": "0", "SD_WS_MF32": "1"}, 3, 17, 33, (64,), 64),
            ({"SD_WS_CO128": "0", "SD_WS_MF32": "1"}, 1, 24, 64, (64,), 128),
            ({"SD_WS_MF32": "0"}, 3, 17, 33, (64,), 64)]


@pytest.mark.parametrize("env,B,H,W,chans,co", WGRAD_BN)
def test_conv3x3_wgrad_bn_relu_source_variants(monkeypatch, env, B, H, W, chans, co):
    """bf16 weight gradients whose x operand is relu(bn(y)) (one source or a concatenation) applied while the halo is
    staged, at the 64 x 64 and 128 x 32 blocks and on both MFMA shapes: dW is the float64 sum."""
    lib = L()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ci = sum(chans)
    S, dy, dw = _wgrad_case(B, H, W, chans, co, (True,) * len(chans))
    assert S.zeros_at_relu() > 0
    a = lib.make_src(_dev(dy, "bf16"), co, H, W, taps=1)
    got = _wgrad("bf16", a, _src(S, H, W, "bf16"), B, H, W, co, 9 * ci, lib.SD_W_CONV3, ci, (co, ci, 3, 3))
    assert _same(got, R.expected(dw, "fp32"))


@functools.lru_cache(maxsize=4)
def _bnbwd_case(B, H, W, chans, co):
    def build(amp):
        S = R.make_source(B, chans, H, W, 400 + H + W, amp, bn=(True,) * len(chans))
        bb = R.BnBwd(B, co, H, W, 401 + H, amp)
        return S, bb, R.wgrad_case(S.x(), bb.dy)

    return R.fit(build, (8, 4, 3))


# the shapes of test_conv3x3_wgrad_fused_bn_backward (the 8-channel x ones with SD_WG_X8 both ways), of the MFMA-shape
# test and of the dual-source one
BNBWD = [({}, 2, 30, 40, (128,), 64), ({}, 1, 15, 20, (128,), 128), ({}, 2, 10, 14, (32,), 64), ({}, 1, 24, 64, (32,), 32),
         ({}, 1, 16, 64, (64,), 32), ({}, 3, 17, 33, (64,), 64), ({}, 2, 15, 20, (256,), 64), ({}, 2, 32, 64, (8,), 32),
         ({}, 1, 30, 50, (8,), 32), ({"SD_WG_X8": "0"}, 2, 32, 64, (8,), 32), ({"SD_WG_X8": "0"}, 1, 30, 50, (8,), 32),
         ({}, 2, 24, 64, (32, 32), 32), ({}, 1, 20, 30, (32, 32), 64), ({}, 2, 16, 40, (32, 96), 32),
         ({"SD_WS_CO128": "0", "SD_WS_MF32": "1"}, 3, 17, 33, (64,), 64),
         ({"SD_WS_CO128": "0", "SD_WS_MF32": "1"}, 1, 24, 64, (64,), 128)]


@pytest.mark.parametrize("env,B,H,W,chans,co", BNBWD)
def test_conv3x3_wgrad_fused_bn_backward_exact(monkeypatch, env, B, H, W, chans, co):
    """sd_wgrad_gemm_bnbwd: dy = the BatchNorm-backward apply of (da, y) formed while staging, with pre-activations
    exactly at 0 (masked: z > 0 is false): the dy it writes for the dgrad is the float64 dy (bf16-exact on the
    lattice) at every element and dW the float64 weight gradient on it."""
    lib = L()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ci = sum(chans)
    S, bb, dw = _bnbwd_case(B, H, W, chans, co)
    write_dy = ci % 32 == 0
    dyd = _nan(B * H * W, co, "bf16")
    a = lib.make_src(dyd if write_dy else None, co, H, W, taps=1)
    b = _src(S, H, W, "bf16")
    assert lib.call("sd_wgrad_bnbwd_ok", lib.SD_BF16, a, b, co, 9 * ci) > 0
    keep = [_dev(bb.da, "bf16"), _dev(bb.y, "bf16")] + [_f32(t) for t in bb.params()]
    got = _wgrad("bf16", a, b, B, H, W, co, 9 * ci, lib.SD_W_CONV3, ci, (co, ci, 3, 3), bnb=keep)
    assert _same(got, R.expected(dw, "fp32"))
    if write_dy:
        assert _same(dyd.cpu(), _want(bb.dy, "bf16"))
    else:
        assert bool(torch.isnan(dyd).all())


# ----------------------------------------------------------------------------------------------- ConvTranspose2d
@functools.lru_cache(maxsize=4)
def _convT_case(B, h, w_, ci, co, bn, split=False):
    def build(amp):
        S = R.make_source(B, (ci,), h, w_, 500 + h, amp[0], bn=(bn,))
        wt = _weights((ci, co, 2, 2), 11 + ci, amp[1], -2, split)
        bias = R.int_bias(co, 12 + co)
        x = S.x()
        if split:
            out = R.convT(x, wt, bias)
            R.require_sum_exact(R.convT(x.abs(), wt.abs(), bias.abs()), R.step_of(x) * R.step_of(wt), "split convT")
            R.require_rounding(out, "split convT")
            return S, wt, bias, out
        out = R.convT_case(x, wt, bias, rounding=not _tiny(h, w_))
        dout = R.acts(B, co, 2 * h, 2 * w_, 501 + h, amp[0])
        dx = R.convT_dgrad_case(dout, wt, rounding=not _tiny(h, w_))
        return S, wt, bias, out, dout, dx

    return R.fit(build, AMPS_SUM if split else AMPS)


@functools.lru_cache(maxsize=4)
def _convT_wgrad_case(B, h, w_, ci, co):
    def build(amp):
        S = R.make_source(B, (ci,), h, w_, 510 + h, amp, bn=(True,))
        dout = R.acts(B, co, 2 * h, 2 * w_, 511 + h, amp)
        return (S, dout) + R.convT_wgrad_case(S.x(), dout)

    return R.fit(build, (8, 4, 3))


# the shapes of test_gpu_ops.py::test_convT_fwd_dgrad_wgrad_bias (k_convt with many ragged tiles, K = 256 / 512: the
# tiled GEMM), plus 1x1 and odd batch-3 grids
CONVT = [(2, 5, 7, 32, 16), (2, 12, 20, 64, 32), (1, 15, 20, 128, 64), (3, 30, 45, 64, 32), (2, 9, 13, 256, 128),
         (1, 6, 10, 512, 256), (1, 1, 1, 32, 16), (3, 3, 5, 64, 32)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,h,w_,ci,co", CONVT)
def test_convT_fwd_dgrad_wgrad_exact(prec, B, h, w_, ci, co):
    """ConvTranspose2d(k2, s2): the PIXSHUF forward with bias from a BN+ReLU source, the 4-tap sub-pixel data gradient,
    and the weight gradient through the SD_W_CONVT reduce; a transposed sub-pixel phase lands on the wrong pixel."""
    lib = L()
    S, wt, bias, out, dout, dx = _convT_case(B, h, w_, ci, co, True)
    wpf, kf = _packT(wt, False, prec)
    src = _src(S, h, w_, prec, taps=1)
    got = _nan(B * 4 * h * w_, co, prec)
    _conv_gemm(prec, src, B, h, w_, wpf, 4 * co, kf, lib.SD_EPI_PIXSHUF, got, bias=_f32(bias))
    assert _same(got.cpu(), _want(out, prec))
    wpd, kd = _packT(wt, True, prec)
    dsrc = lib.make_src(_dev(dout, prec), co, 2 * h, 2 * w_, taps=4)
    gdx = _nan(B * h * w_, ci, prec)
    _conv_gemm(prec, dsrc, B, h, w_, wpd, ci, kd, lib.SD_EPI_STORE, gdx)
    assert _same(gdx.cpu(), _want(dx, prec))
    S, dout, dw, _ = _convT_wgrad_case(B, h, w_, ci, co)
    a = _src(S, h, w_, prec, taps=1)
    b = lib.make_src(_dev(dout, prec), co, 2 * h, 2 * w_, taps=4)
    for batch_reduce in (False, True):
        got = _wgrad(prec, a, b, B, h, w_, ci, 4 * co, lib.SD_W_CONVT, ci, (ci, co, 2, 2), batch_reduce=batch_reduce)
        assert _same(got, R.expected(dw, "fp32"))


CONVT_ENV = [({"SD_CONVT_KMAX": "256"}, 16, 30, 40, 256, 32, True), ({"SD_CONVT_KMAX": "128"}, 16, 30, 40, 256, 32, True),
             ({}, 2, 7, 30, 64, 32, False), ({"SD_FWD_BM": "64"}, 64, 12, 16, 512, 32, False),
             ({"SD_FWD_BM": ""}, 64, 12, 16, 512, 32, False)]


@pytest.mark.parametrize("env,B,h,w_,ci,co,bn", CONVT_ENV)
def test_convT_fwd_routes_exact(monkeypatch, env, B, h, w_, ci, co, bn):
    """The bf16 ConvTranspose2d forward through k_convt (K = 256 at M >= 16384, the identity-source instance) and the
    tiled GEMM at 64 x 128 and 128 x 128 (M >= 12288), each against the float64 bits."""
    lib = L()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S, wt, bias, out = _convT_case(B, h, w_, ci, co, bn)[:4]
    wpf, kf = _packT(wt, False, "bf16")
    got = _nan(B * 4 * h * w_, co, "bf16")
    _conv_gemm("bf16", _src(S, h, w_, "bf16", taps=1), B, h, w_, wpf, 4 * co, kf, lib.SD_EPI_PIXSHUF, got, bias=_f32(bias))
    assert _same(got.cpu(), _want(out, "bf16"))


def test_convT_split_pack_doubled_k_exact():
    """up1's hi/lo forward: the source twice along K against SD_PACK_CONVT_FWD_SPLIT rows [hi | lo] is ConvTranspose2d
    with the fp32 weights a + b * 2^-9 exactly (a forward that ignores the lo half misses b * 2^-9 * x)."""
    lib = L()
    B, H, W, ci, co = 2, 12, 20, 64, 32
    S, wt, bias, out = _convT_case(B, H, W, ci, co, True, True)
    kpad = _kpad(2 * ci)
    wp = _pack_job(wt, lib.SD_PACK_CONVT_FWD_SPLIT, co, ci, ci, kpad, 4 * co)
    assert _same(wp.cpu().reshape(4 * co, kpad), R.expected(R.pack_convT_split(wt, kpad), "bf16"))
    y, bn = S.parts[0]
    yd, bnd = _dev(y, "bf16"), (_f32(bn[0]), _f32(bn[1]))
    src = lib.make_src(yd, ci, H, W, taps=1, bn0=bnd, src1=yd, c1=ci, bn1=bnd)
    got = _nan(B * 4 * H * W, co, "bf16")
    _conv_gemm("bf16", src, B, H, W, wp, 4 * co, kpad, lib.SD_EPI_PIXSHUF, got, bias=_f32(bias))
    assert _same(got.cpu(), _want(out, "bf16"))
    assert not _same(_want(R.convT(S.x(), R.split_hi_lo(wt)[0], bias), "bf16"), _want(out, "bf16"))


# ----------------------------------------------------------------------------------------------- bnsum launches
@functools.lru_cache(maxsize=4)
def _bnsum_case(B, H, W, ci, co, convt):
    """A dgrad-style launch whose stored output dx is da of a BatchNorm layer with raw output y: dx and the sums."""
    def build(amp):
        if convt:
            dout = R.acts(B, co, 2 * H, 2 * W, 600 + H, amp[0])
            w = _weights((ci, co, 2, 2), 13 + ci, amp[1], -2)
            dx = R.convT_dgrad_case(dout, w)
            n_out = ci
        else:
            dout = R.acts(B, ci, H, W, 600 + H, amp[0])
            w = _weights((co, ci, 3, 3), 13 + ci, amp[1], -3)
            R.require_bf16(dout, "bnsum source")
            dx = R.conv3x3(dout, w)
            R.require_sum_exact(R.conv3x3(dout.abs(), w.abs()), R.step_of(dout) * R.step_of(w), "bnsum conv")
            n_out = co
        y = R.acts(B, n_out, H, W, 601 + H, 8, zero_window=False)
        sc, sh = R.bn_affine(n_out, 602)
        mu, inv = R.bn_stats(n_out, 603)
        stored = R.rne_bf16(dx)
        R.require_bn_sums_exact(stored, y, sc, sh, mu, inv, "bnsum")
        return dout, w, dx, y, (sc, sh, mu, inv), R.bn_bwd_sums(stored, y, sc, sh, mu, inv)

    return R.fit(build, AMPS_SUM)


BNSUM = [(2, 32, 64, 32, 32, False), (1, 48, 64, 32, 32, False), (2, 30, 40, 64, 64, False), (1, 16, 64, 128, 64, False),
         (2, 24, 32, 64, 128, False), (1, 26, 50, 32, 64, False), (3, 7, 11, 32, 32, False),
         (2, 12, 20, 64, 32, True), (1, 15, 20, 128, 64, True), (3, 17, 23, 64, 32, True),
         # H or W of 1 and 2
         (1, 1, 1, 32, 32, False), (2, 2, 2, 32, 64, False), (1, 1, 1, 64, 32, True), (2, 2, 1, 64, 32, True)]


@pytest.mark.parametrize("B,H,W,ci,co,convt", BNSUM)
def test_conv_gemm_bnsum_exact(B, H, W, ci, co, convt):
    """sd_conv_gemm_bnsum (3x3 halo shapes and the ConvTranspose2d dgrad through k_convt): the stored output is the RNE
    bf16 of the float64 result and the partial rows sum to the float64 BatchNorm-backward sums over (stored dx, y)."""
    lib = L()
    dout, w, dx, y, prm, sums = _bnsum_case(B, H, W, ci, co, convt)
    if convt:
        wp, kpad = _packT(w, True, "bf16")
        src = lib.make_src(_dev(dout, "bf16"), co, 2 * H, 2 * W, taps=4)
        N = ci
    else:
        wp, kpad = _pack3(w, ci, False, "bf16")
        src = lib.make_src(_dev(dout, "bf16"), ci, H, W, taps=9)
        N = co
    assert lib.call("sd_conv_gemm_bnsum_ok", lib.SD_BF16, src, N) == 1
    rows = lib.call("sd_conv_gemm_bnsum_rows", src, B, H, W, N)
    part = torch.full((rows, N, 2), NAN, device=DEV)
    out = _nan(B * H * W, N, "bf16")
    keep = [_dev(y, "bf16")] + [_f32(t) for t in prm]
    LAUNCHED.add(lib.kernel_name("sd_conv_gemm_bnsum_kernel_name", src, H, W, N))
    lib.call("sd_conv_gemm_bnsum", lib.SD_BF16, src, B, H, W, wp.data_ptr(), N, kpad, out.data_ptr(),
             *[t.data_ptr() for t in keep], part.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    assert _same(out.cpu(), _want(dx, "bf16"))
    assert _same(_stat_sums(part), sums)


# ----------------------------------------------------------------------------------------------- sd_conv3x3_ex / _ws
EX = [(2, 32, 64, (8,), 32, (False,), "stats"), (2, 30, 50, (8,), 32, (False,), "affine"),
      (1, 32, 64, (32,), 32, (True,), "store"), (1, 32, 64, (32, 32), 32, (False, True), "stats"),
      (1, 32, 64, (32, 32), 32, (False, True), "affine"), (2, 15, 20, (64,), 64, (True,), "store"),
      (2, 15, 20, (64, 64), 128, (False, True), "affine"), (1, 30, 40, (128,), 128, (True,), "affine"),
      (1, 32, 64, (64, 64), 64, (False, True), "stats"), (1, 32, 48, (64,), 128, (True,), "store"),
      (3, 7, 11, (16,), 64, (True,), "affine"),
      # H or W of 1 and 2
      (1, 1, 1, (8,), 32, (True,), "store"), (2, 2, 2, (16,), 64, (False,), "stats"), (1, 1, 9, (32,), 32, (True,), "store"),
      # the eval forward's instances with the affine epilogue: enc1.0 at 16x32 tiles, and raw (pooled) sources through
      # the LDS-DMA loaders with the weights resident, staged per chunk, and on a whole-image tile of 300 pixels
      (2, 32, 64, (8,), 32, (False,), "affine"), (1, 16, 32, (32,), 64, (False,), "affine"),
      (1, 16, 32, (64,), 128, (False,), "affine"), (1, 15, 20, (64,), 64, (False,), "affine")]


@pytest.mark.parametrize("wsplit", [True, False])
@pytest.mark.parametrize("B,H,W,chans,co,bn,epi", EX)
def test_conv3x3_ex_split_weights_and_affine_exact(wsplit, B, H, W, chans, co, bn, epi):
    """sd_conv3x3_ex with plain bf16 weights and with SD_CONV_WSPLIT hi/lo pairs of fp32 weights a + b * 2^-9 (the lo
    half contributes b * 2^-9 * x to every output), STORE, STATS and the output affine bf16(acc*scale + shift)."""
    lib = L()
    ci = sum(chans)
    # split weights put the terms 2^-9 below the hi lattice: no amplitude keeps the sums of squares of the stored values
    # within 2^24 steps, so with them the STATS launch's stored output is compared and the sums are pinned by the
    # plain-weight launch of the same shape
    sums = epi == "stats" and not wsplit
    case = _fwd_case(B, H, W, chans, co, bn, False, "stats" if sums else "round", wsplit,
                     21 if epi == "affine" else None)
    S, w, out = case[:3]
    if wsplit:
        kpad = _kpad(18 * ci)
        wp = _pack_job(w, lib.SD_PACK_CONV3_FWD_SPLIT, co, ci, ci, kpad, co)
    else:
        wp, kpad = _pack3(w, ci, False, "bf16")
    src = _src(S, H, W, "bf16")
    assert lib.call("sd_conv3x3_ex_ok", src, co) == 1
    affd = (_f32(case[3][0]), _f32(case[3][1])) if epi == "affine" else (None, None)
    e = lib.SD_EPI_STATS if epi == "stats" else lib.SD_EPI_STORE
    rows = lib.call("sd_conv_gemm_stat_rows", lib.SD_BF16, B, H, W, co)
    st = torch.full((rows, co, 2), NAN, device=DEV)
    got = _nan(B * H * W, co, "bf16")
    LAUNCHED.add(lib.kernel_name("sd_conv3x3_ex_kernel_name", src, H, W, co, e, lib.SD_CONV_WSPLIT if wsplit else 0,
                                 int(epi == "affine")))
    lib.call("sd_conv3x3_ex", src, B, H, W, wp.data_ptr(), co, kpad, e, lib.SD_CONV_WSPLIT if wsplit else 0,
             lib.ptr(affd[0]), lib.ptr(affd[1]), got.data_ptr(), st.data_ptr() if epi == "stats" else None,
             lib.stream_handle())
    torch.cuda.synchronize()
    assert _same(got.cpu(), _want(out, "bf16"))
    if sums:
        assert _same(_stat_sums(st), R.chan_sums(R.rne_bf16(out)))


EX_WS = [(30, 40, (256,), 256, True, True), (15, 20, (256, 256), 512, True, True), (60, 80, (128,), 128, False, False),
         (15, 20, (512,), 512, False, True)]


@pytest.mark.parametrize("H,W,chans,co,wsplit,affine", EX_WS)
def test_conv3x3_ex_split_k_workspace_exact(H, W, chans, co, wsplit, affine):
    """sd_conv3x3_ex_ws at batch 1 (groups of blocks over slices of the chunks and of the hi/lo passes, partials added
    by a second launch, then the output affine): on the lattice the split-K sum is the float64 sum."""
    lib = L()
    ci = sum(chans)
    case = _fwd_case(1, H, W, chans, co, (True,) * len(chans), False, "round", wsplit, 22 if affine else None)
    S, w, out = case[:3]
    if wsplit:
        kpad = _kpad(18 * ci)
        wp = _pack_job(w, lib.SD_PACK_CONV3_FWD_SPLIT, co, ci, ci, kpad, co)
    else:
        wp, kpad = _pack3(w, ci, False, "bf16")
    src = _src(S, H, W, "bf16")
    flags = lib.SD_CONV_WSPLIT if wsplit else 0
    affd = (_f32(case[3][0]), _f32(case[3][1])) if affine else (None, None)
    nbytes = lib.call("sd_conv3x3_ex_ws_bytes", src, 1, H, W, co, lib.SD_EPI_STORE, flags)
    assert nbytes > 0, "the batch-1 deep shapes take the split-K path"
    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    got = _nan(H * W, co, "bf16")
    LAUNCHED.add(lib.kernel_name("sd_conv3x3_ex_kernel_name", src, H, W, co, lib.SD_EPI_STORE, flags, int(affine)))
    lib.call("sd_conv3x3_ex_ws", src, 1, H, W, wp.data_ptr(), co, kpad, lib.SD_EPI_STORE, flags, lib.ptr(affd[0]),
             lib.ptr(affd[1]), got.data_ptr(), None, ws.data_ptr(), 4 * ws.numel(), lib.stream_handle())
    torch.cuda.synchronize()
    assert _same(got.cpu(), _want(out, "bf16"))


# ----------------------------------------------------------------------------------------------- packs
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_weight_packs_bit_exact_in_documented_layout(prec):
    """sd_pack_conv3_w, sd_pack_convT_w and sd_pack_weights (every kind in one launch): lattice weights come back bit
    for bit at the positions include/stereo_hip.h documents, zero padding elsewhere, gaps untouched."""
    lib = L()
    s = lib.stream_handle()
    jobs, wants, keep, off = [], [], [], 0
    for co, ci, cp in ((32, 6, 8), (64, 32, 32), (16, 40, 40)):
        w = R.weights((co, ci, 3, 3), 31 + co, 4, -3)
        for dgrad in (0, 1):
            if dgrad and cp != ci:
                continue
            got, kpad = _pack3(w, cp, dgrad, prec)
            want = R.expected(R.pack_conv3(w, cp, dgrad, kpad), prec)
            torch.cuda.synchronize()
            assert _same(got.cpu().reshape(want.shape), want)
            keep.append(_f32(w))
            jobs.append(lib.SdPackJob(keep[-1].data_ptr(), lib.SD_PACK_CONV3_DGRAD if dgrad else lib.SD_PACK_CONV3_FWD,
                                      co, ci, cp, kpad, off))
            wants.append((off, want.reshape(-1)))
            off += want.numel() + 64
    for ci, co in ((64, 32), (24, 8)):
        w = R.weights((ci, co, 2, 2), 41 + co, 4, -2)
        for dgrad in (0, 1):
            got, kpad = _packT(w, dgrad, prec)
            want = R.expected(R.pack_convT(w, dgrad, kpad), prec)
            torch.cuda.synchronize()
            assert _same(got.cpu().reshape(want.shape), want)
            keep.append(_f32(w))
            jobs.append(lib.SdPackJob(keep[-1].data_ptr(), lib.SD_PACK_CONVT_DGRAD if dgrad else lib.SD_PACK_CONVT_FWD,
                                      co, ci, ci, kpad, off))
            wants.append((off, want.reshape(-1)))
            off += want.numel() + 64
    out = torch.full((off,), 7.0, dtype=_adt(prec), device=DEV)
    lib.call("sd_pack_weights", _sd(prec), (lib.SdPackJob * len(jobs))(*jobs), len(jobs), out.data_ptr(), s)
    torch.cuda.synchronize()
    full = torch.full((off,), 7.0, dtype=_adt(prec))
    for o, want in wants:
        full[o:o + want.numel()] = want
    assert _same(out.cpu(), full)


def test_pack_conv3_split_hi_lo_bit_exact():
    lib = L()
    for co, ci, cp in ((32, 24, 32), (16, 40, 40)):
        w = R.split_weights((co, ci, 3, 3), 51 + co, 4, -3)
        kpad = _kpad(18 * cp)
        got = _pack_job(w, lib.SD_PACK_CONV3_FWD_SPLIT, co, ci, cp, kpad, co)
        assert _same(got.cpu().reshape(co, kpad), R.expected(R.pack_conv3_split(w, cp, kpad), "bf16"))


# ----------------------------------------------------------------------------------------------- fused backwards
@functools.lru_cache(maxsize=2)
def _bwd_fused_case(B, H, W, dec):
    C = 32

    def build(amp):
        bb = R.BnBwd(B, C, H, W, 700 + H, amp[0])
        if dec:
            S = R.make_source(B, (C, C), H, W, 701 + H, amp[0], bn=(False, True))
        else:
            S = R.make_source(B, (C,), H, W, 701 + H, amp[0], bn=(True,))
        w = _weights((C, S.x().shape[1], 3, 3), 17, amp[1], -3)
        dw = R.wgrad_case(S.x(), bb.dy)
        dx = R.dgrad_case(bb.dy, w)
        stored = R.rne_bf16(dx)
        if dec:
            R.require_sum_exact(stored[:, :C].abs().sum((0, 2, 3)), R.step_of(stored), "d(up) column sums")
            sums = stored[:, :C].sum((0, 2, 3))
            prev = None
        else:
            yp, (psc, psh) = S.parts[0]
            pmu, pinv = R.bn_stats(C, 703)
            R.require_bn_sums_exact(stored, yp, psc, psh, pmu, pinv, "previous layer's sums")
            sums = R.bn_bwd_sums(stored, yp, psc, psh, pmu, pinv)
            prev = (pmu, pinv)
        return bb, S, w, dw, dx, sums, prev

    return R.fit(build, ((8, 4), (4, 2), (3, 1), (3, 0)))


@pytest.mark.parametrize("B,H,W", [(2, 16, 64), (1, 8, 32), (3, 24, 48)])
def test_conv3x3_bwd_fused_exact(B, H, W):
    """sd_conv3x3_bwd_fused (enc1.1 / dec1.1 backward in one pass): dW, the stored dx and the previous layer's
    BatchNorm-backward sums over (stored dx, y_prev), each the float64 value."""
    lib = L()
    C = 32
    bb, S, w, dw, dx, sums, (pmu, pinv) = _bwd_fused_case(B, H, W, False)
    yp, (psc, psh) = S.parts[0]
    assert lib.call("sd_conv3x3_bwd_fused_ok", C, C, H, W) == 1
    wp, kpad = _pack3(w, C, True, "bf16")
    sp = lib.call("sd_conv3x3_bwd_fused_splits", B, H, W)
    slab = torch.full((sp * C * 9 * C,), NAN, device=DEV)
    part = torch.full((sp, C, 2), NAN, device=DEV)
    gdx = _nan(B * H * W, C, "bf16")
    tens = [_dev(t, "bf16") for t in (bb.da, bb.y, yp)]
    prm = [_f32(t) for t in bb.params() + (psc, psh, pmu, pinv)]
    lib.call("sd_conv3x3_bwd_fused", tens[0].data_ptr(), tens[1].data_ptr(), *[t.data_ptr() for t in prm[:5]],
             tens[2].data_ptr(), *[t.data_ptr() for t in prm[5:]], wp.data_ptr(), kpad, B, H, W, gdx.data_ptr(),
             slab.data_ptr(), part.data_ptr(), lib.stream_handle())
    gdw = torch.full((C, C, 3, 3), NAN, device=DEV)
    lib.call("sd_wgrad_reduce", slab.data_ptr(), sp, C, 9 * C, lib.SD_W_CONV3, C, gdw.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    assert _same(gdw.cpu(), R.expected(dw, "fp32"))
    assert _same(gdx.cpu(), _want(dx, "bf16"))
    assert _same(_stat_sums(part), sums)


@pytest.mark.parametrize("B,H,W", [(2, 16, 64), (1, 8, 16), (3, 24, 48)])
def test_conv3x3_bwd_fused_dec_exact(B, H, W):
    """sd_conv3x3_bwd_fused_dec (dec1.0's backward in one pass): dW over cat(u, relu(bn(y_skip))), the stored
    d(u) | d(skip) and the column sums of the stored d(u) (the ConvTranspose2d bias gradient)."""
    lib = L()
    C = 32
    bb, S, w, dw, dx, sums, _ = _bwd_fused_case(B, H, W, True)
    (u, _), (ys, (ssc, ssh)) = S.parts
    assert lib.call("sd_conv3x3_bwd_fused_dec_ok", C, C, C, H, W) == 1
    wp, kpad = _pack3(w, 2 * C, True, "bf16")
    sp = lib.call("sd_conv3x3_bwd_fused_splits", B, H, W)
    slab = torch.full((sp * C * 9 * 2 * C,), NAN, device=DEV)
    part = torch.full((sp, C, 2), NAN, device=DEV)
    du, dsk = _nan(B * H * W, C, "bf16"), _nan(B * H * W, C, "bf16")
    tens = [_dev(t, "bf16") for t in (bb.da, bb.y, u, ys)]
    prm = [_f32(t) for t in bb.params() + (ssc, ssh)]
    lib.call("sd_conv3x3_bwd_fused_dec", tens[0].data_ptr(), tens[1].data_ptr(), *[t.data_ptr() for t in prm[:5]],
             tens[2].data_ptr(), tens[3].data_ptr(), prm[5].data_ptr(), prm[6].data_ptr(), wp.data_ptr(), kpad, B, H, W,
             du.data_ptr(), dsk.data_ptr(), slab.data_ptr(), part.data_ptr(), lib.stream_handle())
    gdw = torch.full((C, 2 * C, 3, 3), NAN, device=DEV)
    lib.call("sd_wgrad_reduce", slab.data_ptr(), sp, C, 9 * 2 * C, lib.SD_W_CONV3, 2 * C, gdw.data_ptr(),
             lib.stream_handle())
    bias = torch.full((C,), NAN, device=DEV)
    lib.call("sd_stat_rows_sum", part.data_ptr(), sp, C, C, bias.data_ptr(), lib.stream_handle())
    torch.cuda.synchronize()
    assert _same(gdw.cpu(), R.expected(dw, "fp32"))
    assert _same(du.cpu(), _want(dx[:, :C], "bf16"))
    assert _same(dsk.cpu(), _want(dx[:, C:], "bf16"))
    assert _same(bias.cpu(), R.expected(sums, "fp32"))


# ----------------------------------------------------------------------------------------------- refused shapes
def test_bad_shapes_are_errors_without_a_launch():
    """Shapes an entry point does not take are refused through the return code and sd_last_error, before any launch:
    the NaN-filled outputs stay untouched."""
    lib = L()
    raw = lib.load()
    B, H, W, ci, co = 1, 3, 5, 8, 32
    x = torch.zeros(B * H * W, ci, dtype=torch.bfloat16, device=DEV)
    wp = torch.zeros(co * 128, dtype=torch.bfloat16, device=DEV)
    out = _nan(B * H * W, co, "bf16")
    src = lib.make_src(x, ci, H, W, taps=9)
    s = lib.stream_handle()
    for args in ((0, H, W), (B, 0, W), (B, H, 0), (B, H + 1, W)):  # empty grids; a grid that is not the source's
        rc = raw.sd_conv_gemm(lib.SD_BF16, src, *args, wp.data_ptr(), co, 128, lib.SD_EPI_STORE, out.data_ptr(), None, 0,
                              None, None, s)
        assert rc != 0 and raw.sd_last_error().decode() != ""
    odd = lib.make_src(x, ci, 3, 5, taps=9, pool=True)  # pooled source dims must be even
    rc = raw.sd_conv_gemm(lib.SD_F32, odd, B, 1, 2, wp.data_ptr(), co, 128, lib.SD_EPI_STORE, out.data_ptr(), None, 0,
                          None, None, s)
    assert rc != 0 and "even" in raw.sd_last_error().decode()
    a = lib.make_src(out, co, H, W, taps=1)
    slab = torch.full((co * 9 * ci,), NAN, device=DEV)
    rc = raw.sd_wgrad_gemm(lib.SD_BF16, a, src, B, 0, W, co, 9 * ci, slab.data_ptr(), 1, s)
    assert rc != 0 and raw.sd_last_error().decode() != ""
    # the fused backwards take no grid with H or W of 1 or 2: _ok says so and the call refuses before any launch
    z16 = torch.zeros(64 * 640, dtype=torch.bfloat16, device=DEV)
    zf = torch.zeros(128, device=DEV)
    fsl = torch.full((32 * 9 * 64,), NAN, device=DEV)
    fpart = torch.full((32, 2), NAN, device=DEV)
    fdx, fds = _nan(64, 32, "bf16"), _nan(64, 32, "bf16")
    z, f = z16.data_ptr(), zf.data_ptr()
    for h, w_ in ((1, 1), (2, 2), (1, 40), (2, 32)):
        assert lib.call("sd_conv3x3_bwd_fused_ok", 32, 32, h, w_) == 0
        assert lib.call("sd_conv3x3_bwd_fused_dec_ok", 32, 32, 32, h, w_) == 0
        rc = raw.sd_conv3x3_bwd_fused(z, z, f, f, f, f, f, z, f, f, f, f, z, 320, 1, h, w_, fdx.data_ptr(), fsl.data_ptr(),
                                      fpart.data_ptr(), s)
        assert rc != 0 and "sd_conv3x3_bwd_fused" in raw.sd_last_error().decode()
        rc = raw.sd_conv3x3_bwd_fused_dec(z, z, f, f, f, f, f, z, z, f, f, z, 320, 1, h, w_, fdx.data_ptr(), fds.data_ptr(),
                                          fsl.data_ptr(), fpart.data_ptr(), s)
        assert rc != 0 and "sd_conv3x3_bwd_fused_dec" in raw.sd_last_error().decode()
    # sd_conv3x3_ex and sd_conv_gemm_bnsum take such grids (EX, BNSUM above); what they refuse: a pooled source, N = 48
    pooled = lib.make_src(x, ci, 2 * H, 2 * W, taps=9, pool=True)
    assert lib.call("sd_conv3x3_ex_ok", pooled, co) == 0 and lib.call("sd_conv3x3_ex_ok", src, 48) == 0
    assert lib.call("sd_conv_gemm_bnsum_ok", lib.SD_BF16, pooled, co) == 0
    rc = raw.sd_conv3x3_ex(src, B, H, W, wp.data_ptr(), 48, 128, lib.SD_EPI_STORE, 0, None, None, out.data_ptr(), None, s)
    assert rc != 0 and "sd_conv3x3_ex" in raw.sd_last_error().decode()
    rc = raw.sd_conv_gemm_bnsum(lib.SD_BF16, src, B, H, W, wp.data_ptr(), 48, 128, out.data_ptr(), z, f, f, f, f,
                                fsl.data_ptr(), s)
    assert rc != 0 and "sd_conv_gemm_bnsum" in raw.sd_last_error().decode()
    torch.cuda.synchronize()
    for t in (out, slab, fsl, fpart, fdx, fds):
        assert bool(torch.isnan(t).all())


# ----------------------------------------------------------------------------------------------- instance coverage
_P = 4096  # a stand-in pointer: the name functions launch nothing and read no memory


def _nsrc(chans, bn, H, W, taps=9, pool=False):
    lib = L()
    b = [(_P, _P) if f else None for f in bn]
    Hs, Ws = (2 * H, 2 * W) if pool else (H, W)
    if len(chans) == 1:
        return lib.make_src(_P, chans[0], Hs, Ws, taps=taps, pool=pool, bn0=b[0])
    return lib.make_src(_P, chans[0], Hs, Ws, taps=taps, pool=pool, bn0=b[0], src1=_P, c1=chans[1], bn1=b[1])


def _lattice_names(setenv):
    """The instance names the lattice cases above launch, from the same parameter lists and switches."""
    lib = L()
    bf = lib.SD_BF16
    names = set()

    def gemm(src, B, H, W, N, epi):
        names.add(lib.kernel_name("sd_conv_gemm_kernel_name", bf, src, B, H, W, N, epi))

    def fwd(B, H, W, chans, co, bn, pool, stats=True):
        src = _nsrc(chans, bn, H, W, pool=pool)
        gemm(src, B, H, W, co, lib.SD_EPI_STORE)
        if stats and not pool:
            gemm(src, B, H, W, co, lib.SD_EPI_STATS)

    def env(e):
        for k in ("SD_HALO_CK", "SD_HALO_N32", "SD_HALO_RAW", "SD_WG_X8", "SD_WS_MF32", "SD_WS_CO128", "SD_FWD_BM",
                  "SD_CONVT_KMAX"):
            setenv(k, e.get(k))

    env({})
    for B, H, W, ci, co, pool, bn in FWD:
        fwd(B, H, W, (ci,), co, (bn,), pool)
    for e, B, H, W, chans, co, bn in FWD_ENV:
        env(e)
        fwd(B, H, W, chans, co, bn, False)
    env({})
    for B, H, W, c0, c1, co in DUAL:
        fwd(B, H, W, (c0, c1), co, (False, True), False, stats=False)
        d = _nsrc((co,), (False,), H, W)
        gemm(d, B, H, W, c0 + c1, lib.SD_EPI_SPLIT)
        if c0 + c1 == 32 or (c0 + c1) % 64 == 0:
            gemm(d, B, H, W, c0 + c1, lib.SD_EPI_SPLIT_STATS)
    for lst, bnf in ((WGRAD, False), (WGRAD_BN, True)):
        for c in lst:
            e, (B, H, W, chans, co) = ({}, c[:3] + ((c[3],), c[4])) if lst is WGRAD else (c[0], c[1:])
            env(e)
            names.add(lib.kernel_name("sd_wgrad_kernel_name", bf, _nsrc((co,), (False,), H, W, taps=1),
                                      _nsrc(chans, (bnf,) * len(chans), H, W), co, 9 * sum(chans)))
    for e, B, H, W, chans, co in BNBWD:
        env(e)
        a = _nsrc((co,), (False,), H, W, taps=1)
        if sum(chans) % 32:
            a.ptr[0] = None
        names.add(lib.kernel_name("sd_wgrad_bnbwd_kernel_name", a, _nsrc(chans, (True,) * len(chans), H, W), co,
                                  9 * sum(chans)))
    env({})
    for B, h, w_, ci, co in CONVT:
        s = _nsrc((ci,), (True,), h, w_, taps=1)
        d = _nsrc((co,), (False,), 2 * h, 2 * w_, taps=4)
        gemm(s, B, h, w_, 4 * co, lib.SD_EPI_PIXSHUF)
        gemm(d, B, h, w_, ci, lib.SD_EPI_STORE)
        names.add(lib.kernel_name("sd_wgrad_kernel_name", bf, s, d, ci, 4 * co))
    for e, B, h, w_, ci, co, bn in CONVT_ENV:
        env(e)
        gemm(_nsrc((ci,), (bn,), h, w_, taps=1), B, h, w_, 4 * co, lib.SD_EPI_PIXSHUF)
    env({})
    gemm(_nsrc((64, 64), (True, True), 12, 20, taps=1), 2, 12, 20, 128, lib.SD_EPI_PIXSHUF)
    for B, H, W, ci, co, convt in BNSUM:
        src = _nsrc((co,), (False,), 2 * H, 2 * W, taps=4) if convt else _nsrc((ci,), (False,), H, W)
        names.add(lib.kernel_name("sd_conv_gemm_bnsum_kernel_name", src, H, W, ci if convt else co))
    for B, H, W, chans, co, bn, epi in EX:
        for wsplit in (lib.SD_CONV_WSPLIT, 0):
            names.add(lib.kernel_name("sd_conv3x3_ex_kernel_name", _nsrc(chans, bn, H, W), H, W, co,
                                      lib.SD_EPI_STATS if epi == "stats" else lib.SD_EPI_STORE, wsplit, int(epi == "affine")))
    for H, W, chans, co, wsplit, affine in EX_WS:
        names.add(lib.kernel_name("sd_conv3x3_ex_kernel_name", _nsrc(chans, (True,) * len(chans), H, W), H, W, co,
                                  lib.SD_EPI_STORE, lib.SD_CONV_WSPLIT if wsplit else 0, int(affine)))
    return names


def _model_names(eng, B, H, W, train):
    """The instance names a bf16 StereoUNet step (training forward, weight gradients, data gradients) or eval forward
    launches at B x H x W. The layers, their channels and levels, the fusion switches and the fused-backward decision
    come from the engine's own layer table (eng.convs, eng.ups, eng._bwd_fused, eng._use_wsplit); the sources are built
    as engine.py's _src_fwd / _conv_bwd / _up_bwd build them."""
    from stereo_depth_estimation_amd.engine import PREV_ENC, SKIP_OF_DEC, UP_OF_DEC, UP_SRC

    lib = L()
    bf = lib.SD_BF16
    out = set()
    for cl in eng.convs.values():
        Hl, Wl = H >> cl.level, W >> cl.level
        first = cl.name == "enc1.0"
        if first or (cl.idx == 0 and cl.blk in PREV_ENC):  # the packed input; the pool materialised by sd_bnrelu_pool
            src = _nsrc((cl.cin_pad,), (False,), Hl, Wl)
        elif cl.idx == 1:
            src = _nsrc((cl.cin,), (True,), Hl, Wl)
        else:  # cat([up, skip])
            uc, sc = eng.ups[UP_OF_DEC[cl.blk]].cout, eng.convs[SKIP_OF_DEC[cl.blk] + ".1"].cout
            src = _nsrc((uc, sc), (False, True), Hl, Wl)
        if not train:  # hi/lo split weights, the eval BatchNorm in the epilogue
            assert eng._use_wsplit(cl, False) and eng.zstore and lib.call("sd_conv3x3_ex_ok", src, cl.cout) == 1
            out.add(lib.kernel_name("sd_conv3x3_ex_kernel_name", src, Hl, Wl, cl.cout, lib.SD_EPI_STORE,
                                    lib.SD_CONV_WSPLIT, 1))
            continue
        assert not eng._use_wsplit(cl, True)
        out.add(lib.kernel_name("sd_conv_gemm_kernel_name", bf, src, B, Hl, Wl, cl.cout, lib.SD_EPI_STATS))
        if not first and eng._bwd_fused(cl, H, W):
            continue  # sd_conv3x3_bwd_fused / _dec: one instance each, run by their own tests above
        M, N = cl.cout, 9 * cl.cin_pad
        a = _nsrc((cl.cout,), (False,), Hl, Wl, taps=1)
        if first:
            a.ptr[0] = None
            if not (eng.bn_fuse and lib.call("sd_wgrad_bnbwd_ok", bf, a, src, M, N) == 1):
                a = _nsrc((cl.cout,), (False,), Hl, Wl, taps=1)
        nblk = lib.call("sd_wgrad_bnbwd_ok", bf, a, src, M, N) if eng.bn_fuse else 0
        if nblk == 1 or (nblk == 2 and cl.level == 0):
            out.add(lib.kernel_name("sd_wgrad_bnbwd_kernel_name", a, src, M, N))
        else:
            out.add(lib.kernel_name("sd_wgrad_kernel_name", bf, a, src, M, N))
        if first:
            continue
        d = _nsrc((cl.cout,), (False,), Hl, Wl)
        if cl.idx == 1:
            if eng.bnsum_fuse and cl.cin < 65 and lib.call("sd_conv_gemm_bnsum_ok", bf, d, cl.cin) == 1:
                out.add(lib.kernel_name("sd_conv_gemm_bnsum_kernel_name", d, Hl, Wl, cl.cin))
                continue
            epi = lib.SD_EPI_STORE
        elif cl.blk in PREV_ENC:
            epi = lib.SD_EPI_STORE
        else:
            sums = eng.bias_fuse and (cl.cin == 32 or cl.cin % 64 == 0)
            epi = lib.SD_EPI_SPLIT_STATS if sums else lib.SD_EPI_SPLIT
        out.add(lib.kernel_name("sd_conv_gemm_kernel_name", bf, d, B, Hl, Wl, cl.cin, epi))
    for u in eng.ups.values():
        Hl, Wl = H >> u.level, W >> u.level
        sc = eng.convs[UP_SRC[u.name] + ".1"].cout
        split = eng._use_wsplit(u, train)
        s = _nsrc((sc, sc), (True, True), Hl, Wl, taps=1) if split else _nsrc((sc,), (True,), Hl, Wl, taps=1)
        out.add(lib.kernel_name("sd_conv_gemm_kernel_name", bf, s, B, Hl, Wl, 4 * u.cout, lib.SD_EPI_PIXSHUF))
        if train:
            d = _nsrc((u.cout,), (False,), 2 * Hl, 2 * Wl, taps=4)
            out.add(lib.kernel_name("sd_wgrad_kernel_name", bf, s, d, u.cin, 4 * u.cout))
            if eng.bnsum_fuse and lib.call("sd_conv_gemm_bnsum_ok", bf, d, u.cin) == 1:
                out.add(lib.kernel_name("sd_conv_gemm_bnsum_kernel_name", d, Hl, Wl, u.cin))
            else:
                out.add(lib.kernel_name("sd_conv_gemm_kernel_name", bf, d, B, Hl, Wl, u.cin, lib.SD_EPI_STORE))
    return out


EXEMPT = {}


def test_lattice_cases_reach_every_instance_of_the_model(monkeypatch, request):
    """Every kernel instance that a bf16 StereoUNet launches at 240x320 and 480x640 (training forward, weight and data
    gradients at the benchmark's batch of 64 and at batch 2, eval forward at batch 1), as the name functions report
    them without a launch, is among the instances the lattice cases of this file run (the names are also recorded at
    each launch and compared with the ones foreseen here). Exemptions: 0."""
    def setenv(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)

    reached = _lattice_names(setenv)
    for k in ("SD_HALO_CK", "SD_HALO_N32", "SD_HALO_RAW", "SD_WG_X8", "SD_WS_MF32", "SD_WS_CO128", "SD_FWD_BM",
              "SD_CONVT_KMAX"):
        monkeypatch.delenv(k, raising=False)
    from stereo_depth_estimation_amd.engine import UNetEngine

    eng = UNetEngine(base_channels=32, precision="bf16")
    model = set()
    for H, W in ((240, 320), (480, 640)):
        for B in (64, 2):
            model |= _model_names(eng, B, H, W, True)
        model |= _model_names(eng, 1, H, W, False)
    # the names recorded where the launches were made: each was foreseen from the parameter lists, and when every test
    # of this module ran before this one, the two sets are the same
    assert LAUNCHED.issubset(reached), sorted(LAUNCHED - reached)
    if RAN[0] == sum(1 for it in request.session.items if it.module is request.module):
        assert reached == LAUNCHED, sorted(reached - LAUNCHED)
    assert "" not in model and "" not in reached
    missing = sorted(model - reached - set(EXEMPT))
    assert missing == [], missing
    print(f"\nlattice comparisons: {COMPARED[0]} over {COMPARED[1]} elements; instances reached: {len(reached)}, "
          f"of the model: {len(model)}, exempt: {len(EXEMPT)}")
    print("\n".join(sorted(reached)))
