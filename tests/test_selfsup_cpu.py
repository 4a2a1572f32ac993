"""The label-free adaptation loss without a GPU: the NumPy restatement tests/selfsup_ref.py against torch CPU float64
autograd of the same loss written independently in torch ops and against central finite differences, the host side of
csrc/selfsup.hip (sd_selfsup_ws_bytes' limits and every argument rule of sd_selfsup_loss rejected before a launch), the
adapt tool's option errors and the refusal of fp8."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import selfsup_ref as R
from stereo_depth_estimation_amd import _lib as L
from stereo_depth_estimation_amd import adapt as A
from stereo_depth_estimation_amd import selfsup as S

INF, NAN = float("inf"), float("nan")


def _torch_loss(disp, logvar, inputs, cls, N, w_photo, w_smooth, eps, eps_s, gamma):
    """The loss of INTEGRATION.md "sd_selfsup_loss" in torch ops, float64, differentiable in disp and logvar. The warp's
    xr is the float32 subtraction (the normative text): its value enters as a constant, its derivative -1 through d."""
    n, H, W = disp.shape
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    w_photo, w_smooth, eps, eps_s, gamma = (f32(v) for v in (w_photo, w_smooth, eps, eps_s, gamma))
    d32 = disp.detach().float()
    counted = torch.as_tensor(cls == 0)
    x = torch.arange(W, dtype=torch.float32).expand(n, H, W)
    xr32 = x - torch.where(counted & torch.isfinite(d32), d32, torch.zeros_like(d32))
    x0 = xr32.floor().long().clamp(0, W - 1)
    x1 = (x0 + 1).clamp(max=W - 1)
    dsafe = torch.where(torch.isfinite(disp), disp, torch.zeros_like(disp))
    f = (xr32 - x0.float()).double() - (dsafe - dsafe.detach())
    left, right = inputs[:, :3].double(), inputs[:, 3:].double()
    a = torch.gather(right, 3, x0[:, None].expand(n, 3, H, W))
    b = torch.gather(right, 3, x1[:, None].expand(n, 3, H, W))
    t = left - (a + f[:, None] * (b - a))
    e = torch.sqrt(t * t + eps * eps).sum(dim=1) / 3
    ell = e if logvar is None else e * torch.exp(-logvar) + logvar
    photo = torch.where(counted, ell, torch.zeros_like(ell)).sum()
    smooth = torch.zeros((), dtype=torch.float64)
    for ax in (2, 1):
        if disp.shape[ax] < 2:
            continue
        k = disp.shape[ax] - 1
        dp, dq = dsafe.narrow(ax, 0, k), dsafe.narrow(ax, 1, k)
        ok = torch.isfinite(disp.narrow(ax, 0, k)) & torch.isfinite(disp.narrow(ax, 1, k))
        g = (left.narrow(ax + 1, 1, k) - left.narrow(ax + 1, 0, k)).abs().sum(dim=1) / 3
        term = torch.exp(-gamma * g) * torch.sqrt((dq - dp) ** 2 + eps_s * eps_s)
        smooth = smooth + torch.where(ok, term, torch.zeros_like(term)).sum()
    return w_photo * photo / N + w_smooth * smooth / (n * H * W), photo, smooth


@pytest.mark.parametrize("with_lv", (True, False))
@pytest.mark.parametrize("shape", ((2, 5, 37), (1, 1, 9), (3, 4, 1), (1, 2, 2)))
def test_restatement_matches_torch_autograd(shape, with_lv):
    """Loss and both gradients of the float64 restatement against torch CPU float64 autograd. Both evaluate the same
    real function on the same float32 xr, so they differ by float64 rounding only: 1e-12 of the largest gradient term
    (the gradients are sums of at most seven terms of that size), 1e-12 relative for the sums."""
    disp, logvar, inputs = R.random_case(*shape, seed=11)
    if not with_lv:
        logvar = None
    cls, crows = R.classes(disp)
    params = dict(w_photo=1.3, w_smooth=0.2, eps=0.01, eps_s=0.02, gamma=7.0)
    ref = R.loss(disp, logvar, inputs, cls, crows, **params)
    d = torch.tensor(disp, dtype=torch.float64, requires_grad=True)
    lv = torch.tensor(logvar, dtype=torch.float64, requires_grad=True) if with_lv else None
    total, photo, smooth = _torch_loss(d, lv, torch.tensor(inputs), cls, ref["N"], **params)
    total.backward()
    gd = torch.where(torch.isfinite(d), d.grad, torch.zeros_like(d.grad)).numpy()
    tol = 1e-12 * max(ref["gterm"], 1e-30)
    assert np.abs(gd - ref["gdisp"]).max() <= tol
    if with_lv:
        assert np.abs(lv.grad.numpy() - ref["glogvar"]).max() <= tol
    else:
        assert ref["glogvar"] is None
    assert ref["rows"][:, 1].sum() == pytest.approx(float(photo.detach()), rel=1e-12, abs=1e-300)
    assert ref["rows"][:, 3].sum() == pytest.approx(float(smooth.detach()), rel=1e-12, abs=1e-300)
    assert ref["total"] == pytest.approx(float(total.detach()), rel=1e-12)
    assert ref["count"] == int((cls == 0).sum()) == int(ref["rows"][:, 0].sum())


def test_central_finite_differences():
    """d total / d disp and d total / d logvar of the restatement against central differences of its own total at a
    handful of pixels whose xr is not within 1e-3 of an integer (the warp has a kink there). Disparities and
    log-variances are multiples of 2^-14 below 64, so x - d and the steps of 2^-14 are exact in float32; the truncation
    error of the difference is (h / eps)^2 / 6 ~ 1e-5 relative, the bound 1e-3 of the largest gradient."""
    n, H, W, h = 2, 5, 37, 2.0 ** -14
    disp, logvar, inputs = R.random_case(n, H, W, seed=5)
    disp = np.where(np.isfinite(disp), np.round(np.minimum(disp, 60) / h) * h, disp).astype(np.float32)
    logvar = (np.round(logvar / h) * h).astype(np.float32)
    cls, crows = R.classes(disp)
    ref = R.loss(disp, logvar, inputs, cls, crows)
    xr = np.arange(W, dtype=np.float32) - np.where(np.isfinite(disp), disp, 0.5)
    ok = np.isfinite(disp) & (np.abs(xr - np.round(xr)) > 1e-3)
    picks = [p for p in np.argwhere(ok & (cls == 0))[::17][:6]] + [p for p in np.argwhere(ok & (cls != 0))[::5][:3]]
    assert len(picks) >= 6
    scale = max(np.abs(ref["gdisp"]).max(), np.abs(ref["glogvar"]).max())
    for i, y, x in picks:
        for name, arr in (("gdisp", disp), ("glogvar", logvar)):
            vals = []
            for sgn in (1.0, -1.0):
                moved = arr.copy()
                moved[i, y, x] = np.float32(arr[i, y, x] + sgn * h)
                assert float(moved[i, y, x]) == float(arr[i, y, x]) + sgn * h
                args = (moved, logvar) if name == "gdisp" else (disp, moved)
                vals.append(R.loss(*args, inputs, cls, crows)["total"])
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - ref[name][i, y, x]) <= 1e-3 * scale, (name, i, y, x, fd, ref[name][i, y, x])


def test_float32_restatement_is_close_and_exact_in_counts():
    """The dtype switch: the float32 evaluation takes the same index and class decisions (equal counts) and differs from
    float64 by float32 rounding."""
    disp, logvar, inputs = R.random_case(2, 5, 70, seed=3)
    cls, crows = R.classes(disp)
    r64 = R.loss(disp, logvar, inputs, cls, crows)
    r32 = R.loss(disp, logvar, inputs, cls, crows, dtype=np.float32)
    assert r32["gdisp"].dtype == np.float32 and r32["glogvar"].dtype == np.float32
    assert np.array_equal(r32["rows"][:, [0, 4]], r64["rows"][:, [0, 4]]) and r32["count"] == r64["count"]
    assert np.abs(r32["gdisp"] - r64["gdisp"]).max() <= 1e-3 * r64["gterm"]
    assert np.abs(r32["glogvar"] - r64["glogvar"]).max() <= 1e-3 * r64["gterm"]
    assert np.allclose(r32["rows"], r64["rows"], rtol=1e-4)
    assert (r64["gdisp"][~np.isfinite(disp)] == 0).all()
    assert (r64["glogvar"][cls != 0] == 0).all()


def test_nothing_counted():
    disp = np.full((1, 3, 8), np.nan, dtype=np.float32)
    _, logvar, inputs = R.random_case(1, 3, 8, seed=1)
    cls, crows = R.classes(disp)
    ref = R.loss(disp, logvar, inputs, cls, crows)
    assert ref["count"] == 0 and ref["N"] == 1.0 and (ref["gdisp"] == 0).all() and (ref["glogvar"] == 0).all()
    assert ref["rows"][0, [0, 1, 2, 3, 4, 5]].tolist() == [0, 0, 0, 0, 0, 0]
    s = S.summary_from_rows(ref["rows"], 24, 1.0, 0.1)
    assert s == {"loss": 0.0, "photo": None, "smooth": 0.0, "visible_fraction": 0.0, "grad_l1": 0.0}


def test_ws_bytes_limits():
    ws = lambda *a: L.call("sd_selfsup_ws_bytes", *a)  # noqa: E731
    assert ws(1, 1, 1) == 128  # the header and one partial row of 8 doubles
    assert ws(3, 480, 640) - 64 == 3 * (ws(1, 480, 640) - 64) and ws(1, 480, 640) == 64 + 480 * 64
    assert ws(1, 480, 64) == 64 + 30 * 64      # sixteen rows per block when W is small
    assert 0 < ws(1, 100000, 16) <= 64 + 1024 * 64  # a bounded number of partial rows however tall the image
    for bad in ((0, 4, 4), (65536, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (1, 4, -4), (1, 65536, 32768),
                (1, 46341, 46341)):
        assert ws(*bad) == -1, bad
    assert ws(65535, 4, 4) > 0 and ws(1, 65536, 32767) > 0
    assert S.STEP_PIXELS == 1024 and S.MAX_SAMPLES == 65535 and S.ROW == 8


def test_loss_rejects_bad_args_without_launch():
    p = 256  # a non-null, aligned address that is never dereferenced
    ok = dict(n=1, disp=p, logvar=p, input=p, cls=p, check_rows=p, H=4, W=4, w_photo=1.0, w_smooth=0.1, eps=0.01,
              eps_s=0.01, gamma=10.0, gdisp=p, glogvar=p, rows=p, count=p, work=p)

    def call(**kw):
        a = {**ok, **kw}
        L.call("sd_selfsup_loss", *[a[k] for k in ok], None)

    cases = [(dict(n=0), "n = 0"), (dict(n=65536), "n = 65536"), (dict(disp=None), "null disp"),
             (dict(input=None), "null input"), (dict(cls=None), "null cls"), (dict(check_rows=None), "null check_rows"),
             (dict(H=0), "bad sizes"), (dict(W=-3), "bad sizes"), (dict(H=65536, W=32768), "bad sizes"),
             (dict(gdisp=None), "null gdisp"), (dict(logvar=None), "glogvar needs logvar"),
             (dict(rows=None), "null rows or count"), (dict(count=None), "null rows or count"),
             (dict(work=None), "8-B aligned"), (dict(work=p + 4), "8-B aligned"), (dict(rows=p + 4), "8-B aligned"),
             (dict(check_rows=p + 4), "8-B aligned"), (dict(disp=p + 2), "4-B aligned"), (dict(gdisp=p + 1), "4-B aligned"),
             (dict(count=p + 2), "4-B aligned")]
    for name, strict in (("w_photo", False), ("w_smooth", False), ("eps", True), ("eps_s", True), ("gamma", False)):
        cases += [({name: -0.5}, f"{name} -0.5"), ({name: NAN}, f"{name} nan"), ({name: INF}, f"{name} inf")]
        if strict:
            cases.append(({name: 0.0}, f"{name} 0"))
    for kw, msg in cases:
        with pytest.raises(L.StereoHipError, match=msg):
            call(**kw)


def test_python_parameter_rules():
    assert S.selfsup_params() == tuple(float(np.float32(v)) for v in (1.0, 0.1, 0.01, 0.01, 10.0))
    assert S.selfsup_params(0, 0, 1e-3, 1e-3, 0)[:2] == (0.0, 0.0)
    for kw in (dict(w_photo=-1), dict(w_smooth=NAN), dict(eps=0), dict(eps_s=-1), dict(gamma=INF), dict(eps=INF)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            S.selfsup_params(**kw)
    with pytest.raises(ValueError, match="streams"):
        S.SelfSupLoss(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.SelfSupLoss(1, device="cpu")
    with pytest.raises(ValueError, match="occ_tol"):
        S.SelfSupLoss(1, occ_tol=-1)


def test_adapt_option_errors(tmp_path):
    good = dict(left_dir=tmp_path, right_dir=tmp_path, output_dir=tmp_path / "out")
    o = A.adapt_options(**good)
    assert (o["epochs"], o["batch_size"], o["lr"], o["weight_decay"], o["precision"], o["uncertainty"]) == \
        (1, 16, 1e-5, 0.0, "fp32", True)
    assert (o["w_smooth"], o["edge_gamma"], o["occ_tol"]) == (float(np.float32(0.1)), 10.0, 0.5)
    for kw, msg in ((dict(dataset_root=tmp_path), "either --dataset-root or both"), (dict(right_dir=None), "either --dataset-root"),
                    (dict(left_dir=None, right_dir=None), "either --dataset-root"), (dict(output_dir=None), "--output-dir"),
                    (dict(precision="fp8"), "fp8 is the inference-only"), (dict(epochs=0), "--epochs"),
                    (dict(batch_size=0), "--batch-size"), (dict(lr=0.0), "--lr"), (dict(lr=NAN), "--lr"),
                    (dict(weight_decay=-1.0), "--weight-decay"), (dict(max_samples=-1), "--max-samples"),
                    (dict(height=32), "both or neither"), (dict(height=30, width=64), "multiples of 16"),
                    (dict(w_smooth=-1.0), "w_smooth"), (dict(edge_gamma=NAN), "gamma"), (dict(occ_tol=-0.1), "occ_tol")):
        with pytest.raises(ValueError, match=msg):
            A.adapt_options(**{**good, **kw})
    # the entry point raises the same way, before it looks for a model or a device
    with pytest.raises(ValueError, match="--epochs"):
        A.adapt("ck.pt", **{**good, "epochs": 0})
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.adapt("ck.pt", device="cpu", **good)
    assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit):
        A.main(["--checkpoint", "c", "--output-dir", str(tmp_path / "out"), "--left-dir", str(tmp_path)])
    a = A.build_parser().parse_args(["--checkpoint", "c", "--dataset-root", "d", "--output-dir", "o"])
    assert (a.epochs, a.batch_size, a.lr, a.weight_decay, a.precision, a.w_smooth, a.edge_gamma, a.occ_tol,
            a.no_uncertainty, a.max_samples, a.seed, a.device) == (1, 16, 1e-5, 0.0, "fp32", 0.1, 10.0, 0.5, False, 0, 42, "cuda")
    with pytest.raises(SystemExit):
        A.build_parser().parse_args(["--checkpoint", "c", "--dataset-root", "d", "--output-dir", "o", "--precision", "fp8"])


def test_fp8_raises():
    class Fp8Model:
        precision = "fp8"
        training = True

    with pytest.raises(RuntimeError, match="fp8"):
        S.adapt_step(Fp8Model(), None, torch.zeros(1, 6, 16, 16), None)
