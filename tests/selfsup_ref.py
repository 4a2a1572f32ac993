"""NumPy restatement of sd_selfsup_loss (INTEGRATION.md "sd_selfsup_loss"; kernels in csrc/selfsup.hip): the photometric
and smoothness terms of the label-free adaptation loss and their gradient with respect to disparity and log-variance.
Evaluated in float64 (the reference of the device tests) or, with ``dtype=np.float32``, with every operation rounded on
its own as the kernel does; the distance between the two is what float32 arithmetic costs, and the device tests take
their bound from it. In both, xr, x0 and f come from the float32 subtraction, so every index and every class decision
is the device's."""

from __future__ import annotations

import numpy as np

import check_ref

F = np.float32
DEFAULTS = dict(w_photo=1.0, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10.0)


def classes(disp, occ_tol=0.5):
    """(cls uint8 [n, H, W], check_rows float64 [n, 8]) of the geometry-only check, per sample."""
    out = [check_ref.check(d, occ_tol=occ_tol) for d in disp]
    return np.stack([o["cls"] for o in out]), np.stack([o["row"] for o in out])


def normaliser(check_rows) -> tuple[int, float]:
    """(count, N): the counted pixels of the batch from the check stage's rows, and max(1, count)."""
    r = np.asarray(check_rows, dtype=np.float64).reshape(-1, 8)
    total = float((r[:, 0] - r[:, 1] - r[:, 2] - r[:, 6]).sum())
    return int(total), max(1.0, total)


def _pairs(d, left, axis, gamma, eps_s2, T):
    """term and s of the pairs (p, p + 1 along axis) of d [n, H, W], left [n, 3, H, W]; ok where both are finite."""
    def sl(a, lo, ax):
        idx = [slice(None)] * a.ndim
        idx[ax] = slice(1, None) if lo else slice(0, -1)
        return a[tuple(idx)]

    dp, dq = sl(d, 0, axis), sl(d, 1, axis)
    ok = np.isfinite(dp) & np.isfinite(dq)
    dp, dq = np.where(ok, dp, 0).astype(T), np.where(ok, dq, 0).astype(T)
    lp, lq = sl(left, 0, axis + 1), sl(left, 1, axis + 1)
    ad = np.abs((lq - lp).astype(T))
    g = (((ad[:, 0] + ad[:, 1]).astype(T) + ad[:, 2]).astype(T) / T(3)).astype(T)
    w = np.exp(-(gamma * g).astype(T)).astype(T)
    t = (dq - dp).astype(T)
    r = np.sqrt(((t * t).astype(T) + eps_s2).astype(T)).astype(T)
    term = np.where(ok, (w * r).astype(T), 0).astype(T)
    s = np.where(ok, ((w * t).astype(T) / r).astype(T), 0).astype(T)
    return term, s, ok


def loss(disp, logvar, inputs, cls, check_rows, w_photo=1.0, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10.0,
         dtype=np.float64) -> dict:
    """disp float32 [n, H, W]; logvar float32 [n, H, W] or None; inputs float32 [n, 6, H, W]; cls uint8 [n, H, W] and
    check_rows float64 [n, 8] of the check stage on this disp. Returns gdisp, glogvar (None without logvar) in ``dtype``,
    rows float64 [n, 8], count, N, ``total`` (the loss the gradients belong to, fp64) and what the bound of the device
    tests is made of: ``gterm``, the largest single term of a gradient, and ``l``, ``e``, ``terms`` [n, k], the values
    that rows[1], rows[2] and rows[3] add up."""
    T = dtype
    disp = np.asarray(disp, dtype=F)
    n, H, W = disp.shape
    inputs = np.asarray(inputs, dtype=F)
    cls = np.asarray(cls)
    count, N = normaliser(check_rows)
    # the parameters are float32 values; their products are formed in the evaluation's dtype
    wp, wsm, gam = T(F(w_photo)), T(F(w_smooth)), T(F(gamma))
    eps2, eps_s2 = (T(F(eps)) * T(F(eps))).astype(T), (T(F(eps_s)) * T(F(eps_s))).astype(T)
    if T is F:
        sp = F(F(w_photo) / F(N))
        ssm = F(F(w_smooth) / F(n * H * W))
    else:
        sp, ssm = wp / T(N), wsm / T(n * H * W)
    counted = cls == 0
    with np.errstate(all="ignore"):
        # warp: the float32 subtraction in both dtypes
        x = np.broadcast_to(np.arange(W).astype(F), (n, H, W))
        ds = np.where(counted & np.isfinite(disp), disp, F(0)).astype(F)
        xr = (x - ds).astype(F)
        x0 = np.clip(np.floor(xr).astype(np.int64), 0, W - 1)
        f = (xr - x0.astype(F)).astype(F).astype(T)
        x1 = np.minimum(x0 + 1, W - 1)
        ii = np.arange(n)[:, None, None, None]
        cc = np.arange(3)[None, :, None, None]
        yy = np.arange(H)[None, None, :, None]
        left = inputs[:, :3].astype(T)
        right = inputs[:, 3:]
        a = right[ii, cc, yy, x0[:, None]].astype(T)
        b = right[ii, cc, yy, x1[:, None]].astype(T)
        dba = (b - a).astype(T)
        r = (a + (f[:, None] * dba).astype(T)).astype(T)
        t = (left - r).astype(T)
        phi = np.sqrt(((t * t).astype(T) + eps2).astype(T)).astype(T)
        q = ((t / phi).astype(T) * dba).astype(T)
        e = (((phi[:, 0] + phi[:, 1]).astype(T) + phi[:, 2]).astype(T) / T(3)).astype(T)
        de = (((q[:, 0] + q[:, 1]).astype(T) + q[:, 2]).astype(T) / T(3)).astype(T)
        glv = None
        if logvar is None:
            l, dl = e, de
        else:
            lv = np.asarray(logvar, dtype=F).astype(T)
            v = np.exp(-lv).astype(T)
            ev = (e * v).astype(T)
            l = (ev + lv).astype(T)
            dl = (v * de).astype(T)
            glv = np.where(counted, (sp * (T(1) - ev).astype(T)).astype(T), 0).astype(T)
        gp = np.where(counted, (sp * dl).astype(T), 0).astype(T)
        # smoothness
        d = disp.astype(T)
        sx = np.zeros((n, H, W + 1), dtype=T)  # sx[..., j] = s of the pair (j - 1, j); 0 at both ends
        sy = np.zeros((n, H + 1, W), dtype=T)
        rows = np.zeros((n, 8), dtype=np.float64)
        termx = termy = None
        if W > 1:
            termx, s, okx = _pairs(d, left, 2, gam, eps_s2, T)
            sx[:, :, 1:W] = s
            rows[:, 3] += termx.astype(np.float64).sum(axis=(1, 2))
            rows[:, 4] += okx.sum(axis=(1, 2))
        if H > 1:
            termy, s, oky = _pairs(d, left, 1, gam, eps_s2, T)
            sy[:, 1:H] = s
            rows[:, 3] += termy.astype(np.float64).sum(axis=(1, 2))
            rows[:, 4] += oky.sum(axis=(1, 2))
        gs = ((sx[:, :, :W] - sx[:, :, 1:]).astype(T) + (sy[:, :H] - sy[:, 1:]).astype(T)).astype(T)
        gsm = (ssm * gs).astype(T)
        gdisp = np.where(np.isfinite(disp), (gp + gsm).astype(T), 0).astype(T)
        rows[:, 0] = counted.sum(axis=(1, 2))
        rows[:, 1] = np.where(counted, l, 0).astype(np.float64).sum(axis=(1, 2))
        rows[:, 2] = np.where(counted, e, 0).astype(np.float64).sum(axis=(1, 2))
        rows[:, 5] = np.abs(gdisp).astype(np.float64).sum(axis=(1, 2))
        # the largest single term a gradient value is made of (the floor of the device tests' bound)
        gterm = max(float(np.abs(gp).max()), float(np.abs(gsm).max()),
                    float(ssm * max(np.abs(sx).max(), np.abs(sy).max())),
                    0.0 if glv is None else float(np.abs(glv).max()))
        terms = np.concatenate([a.reshape(n, -1) for a in (termx, termy) if a is not None] or [np.zeros((n, 0), dtype=T)],
                               axis=1)
    return {"gdisp": gdisp, "glogvar": glv, "rows": rows, "count": count, "N": N, "gterm": gterm,
            # what rows[1], rows[2] and rows[3] add up, per sample: l and e of the counted pixels (0 elsewhere), the terms
            "l": np.where(counted, l, 0).astype(T).reshape(n, -1), "e": np.where(counted, e, 0).astype(T).reshape(n, -1),
            "terms": terms,
            "total": float(F(w_photo)) * rows[:, 1].sum() / N + float(F(w_smooth)) * rows[:, 3].sum() / (n * H * W)}


def random_case(n: int, H: int, W: int, seed: int):
    """The generator of the tests: per row, runs of 3..12 pixels of one disparity, log-uniform from 0.05 to 1.5 W (past
    the row), plus +-0.2 jitter; 5 % of the pixels from NaN, 0, -3.5, +inf, -inf, -0; the frames a smooth ramp pattern
    in the even samples' rows and white noise in the odd rows, in [0, 1]; logvar uniform in [-6, 3].
    Returns (disp [n, H, W], logvar [n, H, W], inputs [n, 6, H, W]) float32."""
    rng = np.random.default_rng(seed)
    disp = np.empty((n, H, W), dtype=F)
    for i in range(n):
        for y in range(H):
            x = 0
            while x < W:
                run = int(rng.integers(3, 13))
                disp[i, y, x:x + run] = np.exp(rng.uniform(np.log(0.05), np.log(1.5 * W + 1.0)))
                x += run
    disp = (disp + rng.uniform(-0.2, 0.2, disp.shape)).astype(F)
    special = np.array([np.nan, 0.0, -3.5, np.inf, -np.inf, -0.0], dtype=F)
    hole = rng.random(disp.shape) < 0.05
    disp[hole] = special[rng.integers(0, len(special), int(hole.sum()))]
    xs = np.arange(W)[None, None, None, :] / 7.0
    ys = np.arange(H)[None, None, :, None] / 3.0
    ph = rng.uniform(0, 6.28, (n, 6, 1, 1))
    smooth = 0.5 + 0.4 * np.sin(xs + ys + ph)
    noise = rng.random((n, 6, H, W))
    noisy_row = (np.arange(H) % 2 == 1)[None, None, :, None]
    inputs = np.where(noisy_row, noise, smooth).astype(F)
    logvar = rng.uniform(-6.0, 3.0, (n, H, W)).astype(F)
    return disp, logvar, inputs
