"""NumPy restatement of sd_proxy_gray and sd_proxy_loss (INTEGRATION.md "sd_proxy_gray", "sd_proxy_loss"; kernels in
csrc/proxy.hip), written from the text and not from the kernels. The loss is evaluated in float64 (the reference of the
device tests) or, with ``dtype=np.float32``, with every operation rounded on its own in the stated order, which the
device equals bit for bit wherever no ``exp`` is involved. The labels themselves are sgm_ref's: the matcher's
restatement on the restated gray images."""

from __future__ import annotations

import numpy as np

import sgm_ref

F = np.float32
INT32_MAX = 2 ** 31 - 1


def to_bytes(x) -> np.ndarray:
    """b = (int) rint(min(max(x * 255, 0), 255)) in float32, ties to even; a NaN gives 0."""
    with np.errstate(invalid="ignore"):
        v = (np.asarray(x, dtype=F) * F(255)).astype(F)
        v = np.where(v > 0, v, F(0))  # NaN fails the comparison
        v = np.where(v < 255, v, F(255))
    return np.rint(v).astype(np.int32)


def gray(inputs):
    """inputs float32 [n, 6, H, W] (left RGB / 255, then right) -> (gray_l, gray_r) uint8 [n, H, W]: INTEGRATION step 1
    on the bytes with channel 0 as R."""
    b = to_bytes(inputs)

    def one(c):
        return ((4899 * c[:, 0] + 9617 * c[:, 1] + 1868 * c[:, 2] + 8192) >> 14).astype(np.uint8)

    return one(b[:, :3]), one(b[:, 3:])


def labels(inputs, num_disparities=64, block_size=5, **kw) -> np.ndarray:
    """int16 [n, H, W]: sgm_ref.compute on every sample's restated gray pair."""
    p = sgm_ref.Params(num_disparities=num_disparities, block_size=block_size, **kw)
    gl, gr = gray(inputs)
    return np.stack([sgm_ref.compute(a, b, p) for a, b in zip(gl, gr)]).astype(np.int16)


def loss(disp, logvar, q4, w_proxy=1.0, accumulate=0, gdisp=None, glogvar=None, count=0, dtype=np.float64) -> dict:
    """disp float32 [n, H, W]; logvar float32 [n, H, W] or None; q4 int16 [n, H, W]. accumulate = 1: gdisp (and glogvar
    with logvar) float32 [n, H, W] are the maps added onto, count the prior value of the count. Returns gdisp, glogvar
    (None without logvar) in ``dtype``, rows float64 [n, 8], count, Np, labelled (the mask), ``total`` (the loss the
    gradients belong to, fp64) and, for the device tests' bounds, the sums of the magnitudes of the terms each output is
    made of: ``gdisp_mag``, ``glogvar_mag`` [n, H, W] and ``rows_mag`` [n, 8]."""
    T = dtype
    disp = np.asarray(disp, dtype=F)
    q4 = np.asarray(q4, dtype=np.int16)
    n = disp.shape[0]
    labelled = (q4 > 0) & np.isfinite(disp)
    bad = (q4 > 0) & ~np.isfinite(disp)
    found = int(labelled.sum())
    Np = max(1, found)
    w = F(w_proxy)
    sp = F(w / F(Np)) if T is F else T(w) / T(Np)
    with np.errstate(all="ignore"):
        t = (q4.astype(T) / T(16)).astype(T)  # exact
        d = np.where(labelled, disp, F(0)).astype(T)
        diff = (d - t).astype(T)
        a = np.abs(diff)
        sgn = np.sign(diff).astype(T)
        if logvar is None:
            l, dl, glv, av = a, sgn, None, None
        else:
            lv = np.asarray(logvar, dtype=F).astype(T)
            v = np.exp(-lv).astype(T)
            av = (a * v).astype(T)
            l = (av + lv).astype(T)
            dl = (sgn * v).astype(T)
            glv = np.where(labelled, (sp * (T(1) - av).astype(T)).astype(T), T(0)).astype(T)
        gd = np.where(labelled, (sp * dl).astype(T), T(0)).astype(T)
        l = np.where(labelled, l, T(0)).astype(T)
        a = np.where(labelled, a, T(0)).astype(T)
        gd_mag = np.abs(gd).astype(np.float64)
        gl_mag = None
        if glv is not None:
            gl_mag = np.where(labelled, np.abs(np.float64(sp)) * (1.0 + np.abs(av.astype(np.float64))), 0.0)
        rows = np.zeros((n, 8), dtype=np.float64)
        rows[:, 0] = labelled.sum(axis=(1, 2))
        rows[:, 1] = l.astype(np.float64).sum(axis=(1, 2))
        rows[:, 2] = a.astype(np.float64).sum(axis=(1, 2))
        rows[:, 3] = (a.astype(np.float64) ** 2).sum(axis=(1, 2))
        rows[:, 4] = np.abs(gd).astype(np.float64).sum(axis=(1, 2))
        rows[:, 5] = bad.sum(axis=(1, 2))
        rows_mag = np.zeros((n, 8), dtype=np.float64)
        lmag = a.astype(np.float64) if logvar is None else \
            np.where(labelled, np.abs(av.astype(np.float64)) + np.abs(np.asarray(logvar, dtype=np.float64)), 0.0)
        rows_mag[:, 1] = lmag.sum(axis=(1, 2))
        rows_mag[:, 2:5] = rows[:, 2:5]
        if accumulate:
            base_d = np.asarray(gdisp, dtype=F)
            out_d = np.where(labelled, (base_d.astype(T) + gd).astype(T), base_d.astype(T)).astype(T)
            gd_mag = np.where(labelled, np.abs(base_d.astype(np.float64)) + gd_mag, 0.0)
            out_l = None
            if glv is not None:
                base_l = np.asarray(glogvar, dtype=F)
                out_l = np.where(labelled, (base_l.astype(T) + glv).astype(T), base_l.astype(T)).astype(T)
                gl_mag = np.where(labelled, np.abs(base_l.astype(np.float64)) + gl_mag, 0.0)
            total_count = min(INT32_MAX, found + int(count))
        else:
            out_d, out_l, total_count = gd, glv, min(INT32_MAX, found)
    return {"gdisp": out_d, "glogvar": out_l, "rows": rows, "count": total_count, "Np": Np, "labelled": labelled,
            "g_d": gd, "g_lv": glv, "gdisp_mag": gd_mag, "glogvar_mag": gl_mag, "rows_mag": rows_mag,
            "total": float(w) * rows[:, 1].sum() / Np}


def random_case(n: int, H: int, W: int, seed: int):
    """The generator of the tests. By the pixel's flat index k: k % 5 == 0 and every k not named below a valid label
    within +-2 px of the disparity; 1 no label (the matcher's invalid value -16, -1 or -32768 in turn); 2 a valid label
    on a non-finite disparity (NaN, +inf, -inf in turn); 3 the label 0; 4 a valid label equal to the disparity
    (sgn = 0). Disparities uniform in [0.5, 60), labels in [1, 16 * 64]; logvar uniform in [-6, 3].
    Returns (disp float32, logvar float32, q4 int16), each [n, H, W]."""
    rng = np.random.default_rng(seed)
    shape = (n, H, W)
    k = np.arange(n * H * W).reshape(shape)
    disp = rng.uniform(0.5, 60.0, shape).astype(F)
    q4 = np.clip(np.rint(disp.astype(np.float64) * 16 + rng.uniform(-32, 32, shape)), 1, 16 * 64).astype(np.int16)
    kind = k % 5
    q4[kind == 1] = np.array([-16, -1, -32768], dtype=np.int16)[(k[kind == 1] // 5) % 3]
    disp[kind == 2] = np.array([np.nan, np.inf, -np.inf], dtype=F)[(k[kind == 2] // 5) % 3]
    q4[kind == 3] = 0
    disp[kind == 4] = (q4[kind == 4].astype(np.float64) / 16).astype(F)
    logvar = rng.uniform(-6.0, 3.0, shape).astype(F)
    return disp, logvar, q4


def base_maps(n: int, H: int, W: int, labelled, seed: int):
    """Maps to accumulate onto: normal values at the labelled pixels and NaN (with a payload) and -0 at the others, whose
    bytes the stage must leave alone. Returns (gdisp, glogvar) float32 [n, H, W]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        m = rng.uniform(-1e-3, 1e-3, (n, H, W)).astype(F)
        odd = np.zeros((n, H, W), dtype=np.uint32)
        odd[...] = np.where(np.arange(n * H * W).reshape(n, H, W) % 2 == 0, 0x7FC12345, 0x80000000)
        bits = m.view(np.uint32).copy()
        bits[~labelled] = odd[~labelled]
        out.append(bits.view(F))
    return out[0], out[1]


def band_scene(inputs, y0=0, y1=12, value=0.5):
    """``inputs`` [n, 6, H, W] with the rows y0 .. y1 - 1 of both views set to one value: a textureless band. At the top
    of the frame no path of the 3-way matcher brings evidence into it, every cost ties, the winner is disparity 0, and
    a disparity of 0 is no label; a band further down inherits the rows above it through the downward path and is
    labelled throughout."""
    out = np.array(inputs, dtype=F)
    out[:, :, y0:y1, :] = F(value)
    return out
