"""NumPy restatement of sd_selfsup_loss_ssim (INTEGRATION.md "sd_selfsup_loss_ssim"; kernel in csrc/selfsup_ssim.hip):
the label-free adaptation loss whose photometric error is e' = (1 - alpha) e + alpha s, s the structural dissimilarity
of a 3 x 3 window of counted pixels, and its gradient with respect to disparity and log-variance. Evaluated in float64
(the reference of the device tests) or, with ``dtype=np.float32``, with every operation rounded on its own in the stated
order, as the kernel does.

Classes, normaliser, smoothness and the Charbonnier error are ``selfsup_ref``'s, through its ``loss``: the smoothness
gradient and sums are those of a call with ``w_photo = 0``; e and its slope de/dd are those of a call without log-variance,
``w_smooth = 0`` and a normaliser of 1, whose ``gdisp`` is then the slope itself. Only the warp is written again here,
because the window needs r_c and b_c - a_c per channel, which that module does not return."""

from __future__ import annotations

import numpy as np

import selfsup_ref as R

F = np.float32
OFFSETS = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))  # ascending (y, x)


def constants(T):
    """C1 = 0.01 * 0.01 and C2 = 0.03 * 0.03 from the float32 values, the products formed in the evaluation's dtype."""
    return (T(F(0.01)) * T(F(0.01))).astype(T), (T(F(0.03)) * T(F(0.03))).astype(T)


def warp(disp, inputs, counted, T):
    """(left, r, dba) [n, 3, H, W] in T: the warp of selfsup_ref.loss, xr, x0 and f from the float32 subtraction."""
    n, H, W = disp.shape
    x = np.broadcast_to(np.arange(W).astype(F), (n, H, W))
    ds = np.where(counted & np.isfinite(disp), disp, F(0)).astype(F)
    xr = (x - ds).astype(F)
    x0 = np.clip(np.floor(xr).astype(np.int64), 0, W - 1)
    f = (xr - x0.astype(F)).astype(F).astype(T)
    x1 = np.minimum(x0 + 1, W - 1)
    ii = np.arange(n)[:, None, None, None]
    cc = np.arange(3)[None, :, None, None]
    yy = np.arange(H)[None, None, :, None]
    right = inputs[:, 3:]
    a = right[ii, cc, yy, x0[:, None]].astype(T)
    b = right[ii, cc, yy, x1[:, None]].astype(T)
    dba = (b - a).astype(T)
    r = (a + (f[:, None] * dba).astype(T)).astype(T)
    return inputs[:, :3].astype(T), r, dba


def shifted(a, dy, dx, fill=0):
    """b[..., y, x] = a[..., y + dy, x + dx], ``fill`` outside the image."""
    H, W = a.shape[-2:]
    pad = [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)]
    p = np.pad(a, pad, constant_values=fill)
    return p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def window_sum(val, mem, T):
    """The sum of val over win(p), started at 0, its members added in ascending (y, x) order, each addition rounded."""
    acc = np.zeros(val.shape, dtype=T)
    for dy, dx in OFFSETS:
        m = shifted(mem, dy, dx, False)
        acc = (acc + np.where(m, shifted(val, dy, dx), T(0)).astype(T)).astype(T)
    return acc


def window_stats(left, r, mem, T):
    """Per channel and pixel (valid where mem): k, muL, mur and S, P, 2 Qv, T of the stated formulas. left, r
    [n, 3, H, W]; mem [n, H, W]."""
    C1, C2 = constants(T)
    m4 = np.broadcast_to(mem[:, None], left.shape)
    k = window_sum(mem.astype(T), mem, T)
    kk = np.where(mem, k, T(1)).astype(T)[:, None]  # k >= 1 where it is used
    muL = (window_sum(left, m4, T) / kk).astype(T)
    mur = (window_sum(r, m4, T) / kk).astype(T)

    def central(a, mua, b, mub):
        """(sum over q in win(p) of (a(q) - mua(p)) (b(q) - mub(p))) / k"""
        acc = np.zeros(a.shape, dtype=T)
        for dy, dx in OFFSETS:
            m = shifted(m4, dy, dx, False)
            da = (shifted(a, dy, dx) - mua).astype(T)
            db = (shifted(b, dy, dx) - mub).astype(T)
            acc = (acc + np.where(m, (da * db).astype(T), T(0)).astype(T)).astype(T)
        return (acc / kk).astype(T)

    sL, sr, sLr = central(left, muL, left, muL), central(r, mur, r, mur), central(left, muL, r, mur)
    two = T(2)
    A1 = ((two * (muL * mur).astype(T)).astype(T) + C1).astype(T)
    A2 = ((two * sLr).astype(T) + C2).astype(T)
    B1 = (((muL * muL).astype(T) + (mur * mur).astype(T)).astype(T) + C1).astype(T)
    B2 = ((sL + sr).astype(T) + C2).astype(T)
    B12 = (B1 * B2).astype(T)
    S = ((A1 * A2).astype(T) / B12).astype(T)
    P = (two * (((muL * A2).astype(T) / B12).astype(T) - ((S * mur).astype(T) / B1).astype(T)).astype(T)).astype(T)
    Q2 = (two * (-(S / B2).astype(T))).astype(T)
    Tc = ((two * A1).astype(T) / B12).astype(T)
    return {"k": kk, "muL": muL, "mur": mur, "S": S, "P": P, "Q2": Q2, "T": Tc}


def loss(disp, logvar, inputs, cls, check_rows, alpha, w_photo=1.0, w_smooth=0.1, eps=0.01, eps_s=0.01, gamma=10.0,
         dtype=np.float64) -> dict:
    """The arguments of ``selfsup_ref.loss`` and ``alpha``. Returns gdisp, glogvar (None without logvar) in ``dtype``,
    rows float64 [n, 8], count, N, ``total`` (the loss the gradients belong to, fp64) and what the bound of the device
    tests is made of: ``gterm``, the largest single term of a gradient, and ``l``, ``e``, ``s``, ``terms`` [n, k], the
    values that rows[1], rows[2], rows[6] and rows[3] add up; ``ep`` is e' per pixel and ``S`` [n, 3, H, W] the SSIM."""
    T = dtype
    disp = np.asarray(disp, dtype=F)
    n, H, W = disp.shape
    inputs = np.asarray(inputs, dtype=F)
    cls = np.asarray(cls)
    mem = cls == 0
    count, N = R.normaliser(check_rows)
    al = T(F(alpha))
    oma = T(T(1) - al)
    sp = F(F(w_photo) / F(N)) if T is F else T(F(w_photo)) / T(N)
    # selfsup_ref's own statements: smoothness (gradient, terms, pairs), and e with its slope
    sm = R.loss(disp, None, inputs, cls, check_rows, w_photo=0.0, w_smooth=w_smooth, eps=eps, eps_s=eps_s, gamma=gamma,
                dtype=T)
    ch = R.loss(disp, None, inputs, cls, np.zeros((n, 8)), w_photo=1.0, w_smooth=0.0, eps=eps, eps_s=eps_s, gamma=gamma,
                dtype=T)
    gsm = sm["gdisp"]                       # (w_smooth / float32(M)) g_s, 0 where disp is not finite
    e = ch["e"].reshape(n, H, W)            # 0 where not counted
    de = np.where(mem, ch["gdisp"], T(0)).astype(T)  # normaliser 1, weight 1, no smoothness: the slope itself
    with np.errstate(all="ignore"):
        left, r, dba = warp(disp, inputs, mem, T)
        st = window_stats(left, r, mem, T)
        one = (T(1) - st["S"]).astype(T)
        s = (((one[:, 0] + one[:, 1]).astype(T) + one[:, 2]).astype(T) / T(6)).astype(T)
        s = np.where(mem, s, T(0)).astype(T)
        if logvar is None:
            lv, u = None, np.ones((n, H, W), dtype=T)
        else:
            lv = np.asarray(logvar, dtype=F).astype(T)
            u = np.exp(-lv).astype(T)
        # the gather: over p in win(q), ascending
        m4 = np.broadcast_to(mem[:, None], left.shape)
        acc = np.zeros(left.shape, dtype=T)
        hterm = 0.0
        for dy, dx in OFFSETS:
            mp = shifted(m4, dy, dx, False) & m4
            c = {k: shifted(st[k], dy, dx, 1) for k in ("P", "Q2", "T", "muL", "mur", "k")}
            up = shifted(u, dy, dx, 1)[:, None]
            h = ((c["P"] + (c["Q2"] * (r - c["mur"]).astype(T)).astype(T)).astype(T)
                 + (c["T"] * (left - c["muL"]).astype(T)).astype(T)).astype(T)
            h = (h / c["k"]).astype(T)
            term = np.where(mp, (up * h).astype(T), T(0)).astype(T)
            acc = (acc + term).astype(T)
            if mp.any():
                hterm = max(hterm, float(np.abs(np.where(mp, term * dba, 0)).max()))
        g3 = (dba * acc).astype(T)
        gss = (((g3[:, 0] + g3[:, 1]).astype(T) + g3[:, 2]).astype(T) / T(6)).astype(T)
        ep = ((oma * e).astype(T) + (al * s).astype(T)).astype(T)
        glv = None
        if lv is None:
            l = ep
        else:
            ev = (ep * u).astype(T)
            l = (ev + lv).astype(T)
            glv = np.where(mem, (sp * (T(1) - ev).astype(T)).astype(T), T(0)).astype(T)
        pe = (oma * (u * de).astype(T)).astype(T)
        ps = (al * gss).astype(T)
        gp = np.where(mem, (sp * (pe + ps).astype(T)).astype(T), T(0)).astype(T)
        gdisp = np.where(np.isfinite(disp), (gp + gsm).astype(T), T(0)).astype(T)
        l = np.where(mem, l, T(0)).astype(T)
        ep = np.where(mem, ep, T(0)).astype(T)
        rows = np.zeros((n, 8), dtype=np.float64)
        rows[:, 0] = mem.sum(axis=(1, 2))
        rows[:, 1] = l.astype(np.float64).sum(axis=(1, 2))
        rows[:, 2] = e.astype(np.float64).sum(axis=(1, 2))
        rows[:, 3:5] = sm["rows"][:, 3:5]
        rows[:, 5] = np.abs(gdisp).astype(np.float64).sum(axis=(1, 2))
        rows[:, 6] = s.astype(np.float64).sum(axis=(1, 2))
        # the largest single term a gradient value is made of (the floor of the device tests' bound)
        gterm = max(sm["gterm"], float(np.abs(gp).max()), float(np.abs(np.where(mem, sp * pe, 0)).max()),
                    float(np.abs(np.where(mem, sp * ps, 0)).max()), float(abs(sp * al) * hterm / 6.0),
                    0.0 if glv is None else float(np.abs(glv).max()))
    return {"gdisp": gdisp, "glogvar": glv, "rows": rows, "count": count, "N": N, "gterm": gterm,
            "l": l.reshape(n, -1), "e": e.reshape(n, -1), "s": s.reshape(n, -1), "ep": ep.reshape(n, -1),
            "terms": sm["terms"], "S": np.where(m4, st["S"], T(0)).astype(T),
            "total": float(F(w_photo)) * rows[:, 1].sum() / N + float(F(w_smooth)) * rows[:, 3].sum() / (n * H * W)}
