"""Proxy-label adaptation on the device (csrc/proxy.hip: sd_proxy_gray, sd_proxy_loss; stereo_depth_estimation_amd/proxy.py,
selfsup.adapt_step(proxy=) and the adapt tool; needs an MI355X).

The reference is the NumPy restatement tests/proxy_ref.py. sd_proxy_gray is integer arithmetic after one float32
product and one rounding to an integer, so it is held bit for bit. sd_proxy_loss without logvar involves no ``exp``: the
gradient maps, the count and the integer columns of ``rows`` equal the float32 restatement bit for bit. With logvar a
gradient value is within a relative 8 * 2^-24 per term of the float64 restatement (the 4 ulp INTEGRATION.md states for
the device ``exp`` plus the roundings after it), that is 8 * 2^-24 times the sum of the magnitudes of the terms it is made
of (proxy_ref's ``gdisp_mag`` / ``glogvar_mag``: |base| + |g| in accumulate mode, (w / Np)(1 + a v) for g_lv); the float
columns of ``rows`` are within the same factor times the sum of their terms' magnitudes. On an MI355X the worst ratio of
an error to that bound over every case of this file was 0.47 for the gradients and 0.20 for the sums.

Shapes are test_gpu_selfsup.py's (the same row walk): widths around a thread's four pixels, a wave-quarter, one and two
steps of the walk, with one, two and five rows, one and three samples, buffers 0, 1 and 3 elements into their
allocation (so the scalar path runs where W % 4 == 0 too), 0xFF guards around every output.
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import proxy_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import proxy as P
from stereo_depth_estimation_amd import selfsup as S
from test_gpu_selfsup import WIDTHS, guards_untouched, placed, ramp_scene, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFFSETS = (0, 1, 3)
REL = 8 * 2.0 ** -24
W_PROXY = 0.7
LEARN_LR = 3e-2
PRIOR = 5  # what the count holds before an accumulating run


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------------- sd_proxy_gray
def gray_inputs(n, H, W, seed):
    """Values around [0, 1] with exact codes, ties ((k + 0.5) / 255 where the product is exact), out-of-range values,
    NaN and infinities."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.1, 1.1, (n, 6, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    k = rng.integers(0, 256, flat.size)
    pick = rng.random(flat.size)
    flat[pick < 0.2] = (k[pick < 0.2] / 255.0).astype(np.float32)
    half = ((k + 0.5).astype(np.float32) / np.float32(255)).astype(np.float32)
    flat[(pick >= 0.2) & (pick < 0.3)] = half[(pick >= 0.2) & (pick < 0.3)]
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, 0.0], dtype=np.float32)
    sp = (pick >= 0.3) & (pick < 0.33)
    flat[sp] = special[rng.integers(0, len(special), int(sp.sum()))]
    return x


@pytest.mark.parametrize("W", [1, 2, 3, 63, 64, 65, 1025])
def test_gray_is_bit_equal(W):
    s = L.stream_handle(torch.device(DEV))
    i = 0
    for H in (1, 2, 5):
        for n in (1, 3):
            x = gray_inputs(n, H, W, seed=100 * W + 10 * H + n)
            want = R.gray(x)
            for off in (OFFSETS if (H, n) == (5, 3) else (OFFSETS[i % 3],)):
                xin = placed(x, off)
                outs = [placed(np.zeros((n, H, W), np.uint8), off) for _ in range(2)]
                L.call("sd_proxy_gray", n, xin[1].data_ptr(), H, W, outs[0][1].data_ptr(), outs[1][1].data_ptr(), s)
                torch.cuda.synchronize()
                for (raw, view), w in zip(outs, want):
                    assert np.array_equal(view.cpu().numpy(), w), (H, n, off)
                    assert guards_untouched(raw, view)
                assert np.array_equal(xin[1].cpu().numpy().view(np.uint32), x.view(np.uint32))
            i += 1


# ---------------------------------------------------------------------- sd_proxy_loss
_cases = {}


def case(n, H, W):
    """The generator's inputs of one shape and the maps to accumulate onto: made once, read-only."""
    key = (n, H, W)
    if key not in _cases:
        disp, logvar, q4 = R.random_case(n, H, W, seed=1000 * W + 10 * H + n)
        lab = (q4 > 0) & np.isfinite(disp)
        arrs = (disp, logvar, q4) + R.base_maps(n, H, W, lab, seed=W + H + n)
        for a in arrs:
            a.setflags(write=False)
        _cases[key] = arrs
    return _cases[key]


def run_device(n, H, W, disp, logvar, q4, accumulate=0, base=(None, None), off=0, prior=-7, w=W_PROXY):
    """sd_proxy_loss on buffers ``off`` elements into their allocations. Returns numpy outputs and whether every guard
    survived."""
    s = L.stream_handle(torch.device(DEV))
    zero = np.zeros((n, H, W), np.float32)
    bufs = {"disp": placed(disp, off), "q4": placed(q4, off), "gdisp": placed(base[0] if accumulate else zero, off)}
    if not accumulate:
        bufs["gdisp"][1].view(torch.uint8).fill_(0xAB)  # overwrite mode: nobody has to clear the maps
    if logvar is not None:
        bufs["logvar"] = placed(logvar, off)
        bufs["glogvar"] = placed(base[1] if accumulate else zero, off)
        if not accumulate:
            bufs["glogvar"][1].view(torch.uint8).fill_(0xAB)
    rows = torch.full((n, 8), -1.0, dtype=torch.float64, device=DEV)
    count = torch.full((1,), prior, dtype=torch.int32, device=DEV)
    work = torch.full((L.call("sd_proxy_ws_bytes", n, H, W) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    ptr = lambda k: bufs[k][1].data_ptr() if k in bufs else None  # noqa: E731
    L.call("sd_proxy_loss", n, ptr("disp"), ptr("logvar"), ptr("q4"), H, W, w, accumulate, ptr("gdisp"), ptr("glogvar"),
           rows.data_ptr(), count.data_ptr(), work.data_ptr(), s)
    torch.cuda.synchronize()
    out = {k: bufs[k][1].cpu().numpy() for k in ("gdisp", "glogvar") if k in bufs}
    out.update(rows=rows.cpu().numpy(), count=int(count.item()), guards=all(guards_untouched(*bufs[k]) for k in bufs),
               inputs_kept=all(np.array_equal(bufs[k][1].cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))
                               for k, a in (("disp", disp), ("q4", q4))))
    return out


worst = {"grad": 0.0, "sum": 0.0}


def assert_case(got, r64, r32, with_lv, accumulate, base):
    lab = r64["labelled"]
    assert got["guards"] and got["inputs_kept"]
    assert got["count"] == r64["count"] == r32["count"]
    assert np.array_equal(got["rows"][:, [0, 5]], r32["rows"][:, [0, 5]])
    assert (got["rows"][:, 6:] == 0).all()
    names = ("gdisp", "glogvar") if with_lv else ("gdisp",)
    if not with_lv:
        assert "glogvar" not in got
        assert got["gdisp"].tobytes() == r32["gdisp"].tobytes()  # no exp: bit-equal to the float32 restatement
    for bi, k in enumerate(names):
        if accumulate:  # NaN payloads and -0 at the unlabelled pixels: the bytes are the base's
            assert got[k].view(np.uint32)[~lab].tobytes() == base[bi].view(np.uint32)[~lab].tobytes(), k
        else:
            assert (got[k].view(np.uint32)[~lab] == 0).all(), k
        err = np.abs(got[k].astype(np.float64) - r64[k])[lab]
        bound = REL * r64[f"{k}_mag"][lab]
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        print(f"{k}: worst error / bound {ratio:.3f}")
        worst["grad"] = max(worst["grad"], ratio)
        assert (err <= bound).all(), (k, ratio)
    for col in (1, 2, 3, 4):
        err = np.abs(got["rows"][:, col] - r64["rows"][:, col])
        bound = REL * r64["rows_mag"][:, col]
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"rows[:, {col}]: worst error / bound {ratio:.3f}")
        worst["sum"] = max(worst["sum"], ratio)
        assert (err <= bound).all(), (col, err, bound)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 5])
@pytest.mark.parametrize("W", WIDTHS)
def test_loss_is_held_to_the_restatement(W, H, n):
    disp, logvar, q4, base_d, base_l = case(n, H, W)
    i = 0
    for with_lv in (True, False):
        for accumulate in (0, 1):
            lv = logvar if with_lv else None
            kw = dict(w_proxy=W_PROXY, accumulate=accumulate, gdisp=base_d, glogvar=base_l, count=PRIOR)
            r64, r32 = R.loss(disp, lv, q4, **kw), R.loss(disp, lv, q4, dtype=np.float32, **kw)
            got = run_device(n, H, W, disp, lv, q4, accumulate, (base_d, base_l), OFFSETS[i % 3], prior=PRIOR)
            assert_case(got, r64, r32, with_lv, accumulate, (base_d, base_l))
            i += 1
    print("worst ratio so far:", worst)


@pytest.mark.parametrize("W", [64, WIDTHS[-2]])
def test_two_runs_and_both_paths_give_equal_bytes(W):
    """Two runs give equal bytes, and the vector path (offset 0, W % 4 == 0) the scalar path's (offset 1)."""
    n, H = 3, 5
    disp, logvar, q4, base_d, base_l = case(n, H, W)
    for accumulate in (0, 1):
        a = run_device(n, H, W, disp, logvar, q4, accumulate, (base_d, base_l), 0)
        for off in (0, 1):
            b = run_device(n, H, W, disp, logvar, q4, accumulate, (base_d, base_l), off)
            for k in ("gdisp", "glogvar", "rows"):
                assert a[k].tobytes() == b[k].tobytes(), (k, off, accumulate)
            assert a["count"] == b["count"] and b["guards"]


@pytest.mark.parametrize("W", [65, WIDTHS[-3]])
def test_a_stream_depends_on_its_neighbours_only_through_the_normaliser(W):
    """Sample i's bytes in a batch of three equal its bytes at another place of a batch whose other two samples have
    other disparities, log-variances and label values but the same number of labelled pixels (so the same Np)."""
    n, H = 3, 5
    disp, logvar, q4, base_d, base_l = case(n, H, W)
    full = run_device(n, H, W, disp, logvar, q4, 1, (base_d, base_l), 0)
    rng = np.random.default_rng(W)
    lab = (q4 > 0) & np.isfinite(disp)
    other = (np.where(np.isfinite(disp), disp + rng.uniform(0.5, 3.0, disp.shape), disp).astype(np.float32),
             (logvar * np.float32(0.5)).astype(np.float32), np.where(q4 > 0, np.minimum(q4 // 2 + 1, 1024), q4).astype(np.int16))
    assert np.array_equal((other[2] > 0) & np.isfinite(other[0]), lab)
    for i in range(n):
        order = [(i + 1) % n, i, (i + 2) % n]  # sample i moves to place 1, between changed neighbours
        mix = [np.stack([src[j] if j == i else alt[j] for j in order])
               for src, alt in ((disp, other[0]), (logvar, other[1]), (q4, other[2]))]
        bases = tuple(np.stack([b[j] for j in order]) for b in (base_d, base_l))
        got = run_device(n, H, W, *mix, 1, bases, 0)
        assert got["count"] == full["count"]
        for k in ("gdisp", "glogvar", "rows"):
            assert got[k][1].tobytes() == full[k][i].tobytes(), (k, i)


def test_count_overwrite_add_and_saturation():
    n, H, W = 3, 5, 65
    disp, logvar, q4, base_d, base_l = case(n, H, W)
    found = int(((q4 > 0) & np.isfinite(disp)).sum())
    assert found > 2
    imax = 2 ** 31 - 1
    assert run_device(n, H, W, disp, logvar, q4, 0, prior=123456)["count"] == found
    assert run_device(n, H, W, disp, logvar, q4, 1, (base_d, base_l), prior=0)["count"] == found
    assert run_device(n, H, W, disp, logvar, q4, 1, (base_d, base_l), prior=1000)["count"] == found + 1000
    assert run_device(n, H, W, disp, logvar, q4, 1, (base_d, base_l), prior=imax - found)["count"] == imax
    assert run_device(n, H, W, disp, logvar, q4, 1, (base_d, base_l), prior=imax - 1)["count"] == imax
    assert run_device(n, H, W, disp, logvar, q4, 1, (base_d, base_l), prior=imax)["count"] == imax
    none = np.where(q4 > 0, -16, q4).astype(np.int16)
    got = run_device(n, H, W, disp, logvar, none, 0, prior=99)
    assert got["count"] == 0 and (got["gdisp"] == 0).all() and (got["glogvar"] == 0).all() and (got["rows"] == 0).all()
    got = run_device(n, H, W, disp, logvar, none, 1, (base_d, base_l), prior=99)
    assert got["count"] == 99 and got["gdisp"].tobytes() == base_d.tobytes() and got["glogvar"].tobytes() == base_l.tobytes()


# ---------------------------------------------------------------------- ProxyLoss
@pytest.mark.parametrize("scene", ["ramp", "band"])
def test_labels_equal_the_matchers_restatement(scene):
    """ProxyLoss.labels against sgm_ref.compute on the restated grays, bit for bit, at 2 x 32 x 64 with D = 16: the
    ramp scene, and the same with a textureless band at the top, where the restatement keeps no label (the winner is
    disparity 0, which is no label) while it labels the rows below."""
    x = ramp_scene(seed=0)
    D = 16
    if scene == "band":
        x = R.band_scene(x)
    want = R.labels(x, num_disparities=D, block_size=5)
    right = want[:, :, D:] > 0
    assert right.any()
    if scene == "band":
        assert (~right).any() and not right[:, 2:8].any() and right[:, 20:].all()
    px = P.ProxyLoss(2, num_disparities=D, block_size=5)
    xs = torch.as_tensor(x).to(DEV)
    got = px.labels(xs)
    assert got.dtype == torch.int16 and tuple(got.shape) == (2, 32, 64)
    assert np.array_equal(got.cpu().numpy(), want)
    assert got.data_ptr() == px.labels(xs).data_ptr()  # the object's own buffer, overwritten by the next call
    # run on those labels: the class route gives sd_proxy_loss's numbers, its summary and its totals
    disp = torch.as_tensor(np.broadcast_to(np.linspace(2.0, 6.0, 64, dtype=np.float32), (2, 32, 64)).copy()).to(DEV)
    lv = torch.zeros_like(disp)
    res = px.run(disp, lv, xs)
    ref = R.loss(disp.cpu().numpy(), lv.cpu().numpy(), want)
    assert int(res.count.item()) == ref["count"] and torch.equal(res.labels, got)
    s = res.summary()
    want_s = P.summary_from_rows(ref["rows"], 2 * 32 * 64, 1.0)
    assert set(s) == set(P.SUMMARY_KEYS)
    for k in P.SUMMARY_KEYS:
        assert s[k] == pytest.approx(want_s[k], rel=1e-5), k
    assert s["proxy_loss"] == pytest.approx(ref["total"], rel=1e-5)
    px.run(disp[:, None], lv[:, None], xs)
    m = px.means()
    assert m["steps"] == 2 and m["proxy_mae"] == pytest.approx(want_s["proxy_mae"], rel=1e-5)
    assert m["proxy_fraction"] == pytest.approx(ref["count"] / (2 * 32 * 64), rel=1e-12)
    plain = P.ProxyLoss(2, uncertainty=False, num_disparities=D).run(disp, None, xs)
    assert plain.glogvar is None and int(plain.count.item()) == ref["count"]
    with pytest.raises(ValueError, match="needs the logvar"):
        px.run(disp, None, xs)
    with pytest.raises(ValueError, match="inputs must be"):
        px.run(disp, lv, xs[:, :5])
    with pytest.raises(ValueError, match="width 64 is not above"):
        P.ProxyLoss(2).labels(xs)
    with pytest.raises(ValueError, match="1..2 samples"):
        px.labels(torch.cat([xs, xs]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_adapt_step_with_a_proxy_equals_the_autograd_bridge(precision):
    """adapt_step(proxy=)'s flat gradient buffer against the gradients through the autograd bridge fed with the summed
    maps of SelfSupLoss.run and ProxyLoss.run(into=) on the same outputs, bit for bit; the labels-only step against the
    bridge fed with the proxy's own maps; proxy=None against today's adapt_step; a mismatch of uncertainty raises."""
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x = torch.as_tensor(ramp_scene(seed=3)).to(DEV)
    kw = dict(num_disparities=16, block_size=5)

    def fresh(state=None):
        m = small_model(precision, seed=1)
        if state is not None:
            m.load_state_dict(state)
        return m.to(DEV).train()

    m = fresh()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    disp, logvar = m(x, return_uncertainty=True)
    res = S.SelfSupLoss(2).run(disp.detach(), logvar.detach(), x)
    photo_only = res.gdisp.clone()
    pres = P.ProxyLoss(2, **kw).run(disp.detach(), logvar.detach(), x, into=res)
    assert pres.gdisp.data_ptr() == res.gdisp.data_ptr() and not torch.equal(res.gdisp, photo_only)
    gd, gl = res.gdisp.clone()[:, None], res.glogvar.clone()[:, None]
    both = int(res.count.item())
    torch.autograd.backward((disp, logvar), (gd, gl))
    want = m.flat_buffers()[1].clone()
    assert float(want.abs().sum()) > 0

    m2 = fresh(state)
    proxy = P.ProxyLoss(2, **kw)
    res2 = S.adapt_step(m2, FusedAdamW(m2.parameters(), lr=0.0, weight_decay=0.0), x, S.SelfSupLoss(2), proxy=proxy)
    assert torch.equal(res2.gdisp, gd[:, 0]) and torch.equal(res2.glogvar, gl[:, 0])
    labelled = int(proxy.last.rows[:, 0].sum().item())
    assert int(res2.count.item()) == both and 0 < labelled < both
    assert torch.equal(m2.flat_buffers()[1], want)

    # labels only
    m3 = fresh(state)
    disp3, logvar3 = m3(x, return_uncertainty=True)
    only = P.ProxyLoss(2, **kw).run(disp3.detach(), logvar3.detach(), x)
    gd3, gl3 = only.gdisp.clone()[:, None], only.glogvar.clone()[:, None]
    torch.autograd.backward((disp3, logvar3), (gd3, gl3))
    want3 = m3.flat_buffers()[1].clone()
    m4 = fresh(state)
    res4 = S.adapt_step(m4, FusedAdamW(m4.parameters(), lr=0.0, weight_decay=0.0), x, None, proxy=P.ProxyLoss(2, **kw))
    assert isinstance(res4, P.ProxyResult) and int(res4.count.item()) == labelled
    assert torch.equal(res4.gdisp, gd3[:, 0]) and torch.equal(res4.glogvar, gl3[:, 0])
    assert torch.equal(m4.flat_buffers()[1], want3) and not torch.equal(want3, want)

    # proxy=None is today's step
    grads = []
    for extra in ({}, {"proxy": None}):
        m5 = fresh(state)
        r5 = S.adapt_step(m5, FusedAdamW(m5.parameters(), lr=0.0, weight_decay=0.0), x, S.SelfSupLoss(2), **extra)
        assert torch.equal(r5.gdisp, photo_only)
        grads.append(m5.flat_buffers()[1].clone())
    assert torch.equal(grads[0], grads[1]) and not torch.equal(grads[0], want)

    with pytest.raises(ValueError, match="agree on uncertainty"):
        S.adapt_step(m5, None, x, S.SelfSupLoss(2), proxy=P.ProxyLoss(2, uncertainty=False, **kw))
    with pytest.raises(ValueError, match="width 64 is not above"):
        S.adapt_step(m5, None, x, S.SelfSupLoss(2), proxy=P.ProxyLoss(2))


def test_the_gate_opens_when_either_stage_found_pixels():
    """The AdamW gate: a labels-only batch whose label map holds only the invalid value (handed in through ``labels``)
    leaves the weights bit for bit; the matcher's labels alone move them; and with a loss that counts nothing (a
    disparity past the row everywhere) the proxy's labels still open the gate."""
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x = torch.as_tensor(ramp_scene(seed=4)).to(DEV)
    kw = dict(num_disparities=16, block_size=5)
    m = small_model(seed=2)
    opt = FusedAdamW(m.parameters(), lr=1e-2, weight_decay=1e-2)
    m.engine(DEV)
    proxy = P.ProxyLoss(2, **kw)
    invalid = torch.full((2, 32, 64), proxy.matcher.invalid_value, dtype=torch.int16, device=DEV)
    real_labels = proxy.labels
    proxy.labels = lambda inputs: invalid
    before = m.flat_buffers()[0].clone()
    res = S.adapt_step(m, opt, x, None, proxy=proxy)
    assert int(res.count.item()) == 0 and float(res.gdisp.abs().sum()) == 0
    assert torch.equal(m.flat_buffers()[0], before)
    proxy.labels = real_labels
    res = S.adapt_step(m, opt, x, None, proxy=proxy)
    assert int(res.count.item()) > 0 and not torch.equal(m.flat_buffers()[0], before)
    with torch.no_grad():
        m.disparity_head.bias.fill_(200.0)  # every pixel looks left of the right image: the loss counts nothing
    m.engine(DEV)
    before = m.flat_buffers()[0].clone()
    loss = S.SelfSupLoss(2)
    res = S.adapt_step(m, opt, x, loss, proxy=proxy)
    assert bool((res.cls == 2).all()) and int(res.count.item()) == int(proxy.last.rows[:, 0].sum().item()) > 0
    assert not torch.equal(m.flat_buffers()[0], before)


def test_it_learns_from_labels_alone():
    """20 labels-only adapt_steps on the ramp scene with a fixed seed (D = 16, block 5): the mean proxy_mae of the last
    5 steps is below that of the first 5. The learning rate was chosen on an MI355X among 1e-3, 3e-3, 1e-2 and 3e-2
     as the one with the largest fall; the observed means (first 5 -> last 5 steps, px) with this seed and
    with the next one:
        1e-3   3.706 -> 3.612    3.834 -> 3.827
        3e-3   3.687 -> 3.438    3.831 -> 3.810
        1e-2   3.637 -> 2.920    3.805 -> 3.389
        3e-2   3.492 -> 0.597    3.731 -> 2.195"""
    from stereo_depth_estimation_amd.optim import FusedAdamW

    x = torch.as_tensor(ramp_scene(seed=0)).to(DEV)
    m = small_model(seed=0)
    opt = FusedAdamW(m.parameters(), lr=LEARN_LR, weight_decay=0.0)
    proxy = P.ProxyLoss(2, num_disparities=16, block_size=5)
    mae = []
    for _ in range(20):
        mae.append(S.adapt_step(m, opt, x, None, proxy=proxy).summary()["proxy_mae"])
    assert all(v is not None for v in mae)
    first, last = float(np.mean(mae[:5])), float(np.mean(mae[-5:]))
    print(f"lr {LEARN_LR}: proxy_mae first 5 {first:.5f}, last 5 {last:.5f}")
    assert last < first, (first, last)
    assert proxy.means()["steps"] == 20


# ---------------------------------------------------------------------- the tool
def _png_pairs(tmp_path, count=4):
    from PIL import Image

    frames = (ramp_scene(count, 32, 64, seed=9) * 255).round().astype(np.uint8)
    for side, sl in (("left", slice(0, 3)), ("right", slice(3, 6))):
        (tmp_path / side).mkdir()
        for i in range(count):
            Image.fromarray(np.ascontiguousarray(frames[i, sl].transpose(1, 2, 0))).save(tmp_path / side / f"{i:03d}.png")


@pytest.mark.parametrize("only", [False, True])
def test_adapt_tool_with_a_proxy(tmp_path, only):
    """The tool on 4 synthetic PNG pairs at 32 x 64 with --proxy-weight 1 --proxy-num-disparities 16, with and without
    --proxy-only: adapted.pt loads, and adapt_meta.json holds the proxy arguments and figures."""
    from stereo_depth_estimation_amd import adapt as A
    from stereo_depth_estimation_amd import cli
    from stereo_depth_estimation_amd.model import StereoUNet
    from stereo_depth_estimation_amd.optim import FusedAdamW

    _png_pairs(tmp_path)
    src = small_model(seed=5)
    cfg = cli.parse_args(["--height", "32", "--width", "64", "--output-dir", str(tmp_path)])
    cli.save_checkpoint(tmp_path / "src.pt", 3, src, FusedAdamW(src.parameters()), cfg, {"val_mae": 1.0})
    meta = A.main(["--checkpoint", str(tmp_path / "src.pt"), "--left-dir", str(tmp_path / "left"), "--right-dir",
                   str(tmp_path / "right"), "--output-dir", str(tmp_path / "out"), "--base-channels", "8",
                   "--batch-size", "2", "--lr", "1e-4", "--proxy-weight", "1", "--proxy-num-disparities", "16"]
                  + (["--proxy-only"] if only else []))
    assert json.loads((tmp_path / "out" / "adapt_meta.json").read_text()) == json.loads(json.dumps(meta))
    assert (meta["proxy_weight"], meta["proxy_only"], meta["proxy_num_disparities"], meta["proxy_block_size"],
            meta["proxy_mode"]) == (1.0, only, 16, 5, "3way")
    row = meta["epochs_run"][0]
    want = {"proxy_loss", "proxy_mae", "proxy_fraction"} | (set() if only else {"loss", "photo", "smooth", "visible_fraction"})
    assert len(meta["epochs_run"]) == 1 and set(row) == want
    assert meta["proxy_mae_first"] == meta["proxy_mae_last"] == row["proxy_mae"] > 0
    assert 0 < row["proxy_fraction"] <= 0.75  # no column left of the range carries a label
    assert (meta["photo_first"] is None) == only and meta["epe_before"] is None
    back = StereoUNet(base_channels=8)
    ck = cli.load_checkpoint(tmp_path / "out" / "adapted.pt", back, None, DEV)
    assert ck["epoch"] == 3 and ck["args"]["height"] == 32
    moved = [k for k, v in src.state_dict().items() if not torch.equal(v.cpu(), back.state_dict()[k].cpu())]
    assert any(k.endswith("weight") for k in moved)


def test_adapt_tool_with_a_proxy_and_labels_measures_epe(tmp_path):
    """--dataset-root with a proxy: epe_before and epe_after are written as well; and without the proxy weight the
    meta's key set has no proxy key."""
    from conftest import write_stereo_tree

    from stereo_depth_estimation_amd import adapt as A

    write_stereo_tree(tmp_path / "data", scenes=2, frames=2, hw=(45, 61), seed=3)
    m = small_model(seed=6)
    meta = A.adapt(None, model=m, dataset_root=tmp_path / "data", output_dir=tmp_path / "out", height=32, width=64,
                   batch_size=3, epochs=2, lr=1e-3, proxy_weight=1.0, proxy_num_disparities=16)
    assert meta["epe_before"] is not None and meta["epe_after"] is not None and meta["epe_after"] != meta["epe_before"]
    assert (meta["num_samples"], meta["num_batches"], len(meta["epochs_run"])) == (4, 2, 2)
    assert meta["proxy_mae_first"] == meta["epochs_run"][0]["proxy_mae"]
    assert meta["proxy_mae_last"] == meta["epochs_run"][1]["proxy_mae"]
    assert (tmp_path / "out" / "adapted.pt").exists()
    plain = A.adapt(None, model=small_model(seed=6), dataset_root=tmp_path / "data", output_dir=tmp_path / "out2",
                    height=32, width=64, batch_size=3, lr=1e-3)
    assert not any("proxy" in k for k in plain) and not any("proxy" in k for k in plain["epochs_run"][0])
    assert set(meta) - set(plain) == {"proxy_weight", "proxy_only", "proxy_num_disparities", "proxy_block_size",
                                      "proxy_mode", "proxy_mae_first", "proxy_mae_last"}
