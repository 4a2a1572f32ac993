"""Plain numpy statements (float64 unless said otherwise) of the live frame path's definitions, for the tests:
fixed-point remap with a constant border, bilinear resize on half-pixel centres over the REMAPPED image, the front
end's model input, the rectified view, rectify_maps, the colour compose and the nearest-resized contour mask, and the
post stage in numpy float32 exactly as the reference's live app writes it."""

import numpy as np


def remap(frame: np.ndarray, map1: np.ndarray | None, map2: np.ndarray | None) -> np.ndarray:
    """frame uint8 [Hc, Wc, 3]; map1 int16 [Hc, Wc, 2] = integer x, y; map2 uint16, low 10 bits = fy5 << 5 | fx5.
    Bilinear with weights fx5/32, fy5/32; a tap outside the frame contributes 0. float64 [Hc, Wc, 3]."""
    img = frame.astype(np.float64)
    if map1 is None:
        return img
    Hc, Wc, _ = frame.shape
    ix, iy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    f = map2.astype(np.int64) & 1023
    fx, fy = (f & 31) / 32.0, (f >> 5) / 32.0
    out = np.zeros((Hc, Wc, 3), dtype=np.float64)
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            yy, xx = iy + dy, ix + dx
            inside = (yy >= 0) & (yy < Hc) & (xx >= 0) & (xx < Wc)
            tap = np.where(inside[..., None], img[np.clip(yy, 0, Hc - 1), np.clip(xx, 0, Wc - 1)], 0.0)
            out += (wy * wx)[..., None] * tap
    return out


def _src(out_size: int, in_size: int):
    s = (in_size / out_size) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5
    s = np.maximum(s, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    return i0, i1, np.clip(s - i0, 0.0, 1.0)


def resize_bilinear(img: np.ndarray, H: int, W: int) -> np.ndarray:
    """[Hs, Ws, C] float64 -> [H, W, C]: bilinear on half-pixel centres, edge replicate."""
    y0, y1, ly = _src(H, img.shape[0])
    x0, x1, lx = _src(W, img.shape[1])
    lx, ly = lx[None, :, None], ly[:, None, None]
    top = img[y0][:, x0] * (1.0 - lx) + img[y0][:, x1] * lx
    bot = img[y1][:, x0] * (1.0 - lx) + img[y1][:, x1] * lx
    return top * (1.0 - ly) + bot * ly


def front_end(left, right, maps_l, maps_r, H: int, W: int) -> np.ndarray:
    """The reference's model_input [6, H, W] (float64): per side remap -> BGR to RGB -> resize -> / 255."""
    planes = []
    for frame, maps in ((left, maps_l), (right, maps_r)):
        m1, m2 = maps if maps is not None else (None, None)
        small = resize_bilinear(remap(frame, m1, m2), H, W) / 255.0
        planes.append(small[..., ::-1].transpose(2, 0, 1))
    return np.concatenate(planes, axis=0)


def view_u8(frame, map1, map2) -> np.ndarray:
    """The rectified view as displayed: round half to even, saturated."""
    return np.clip(np.rint(remap(frame, map1, map2)), 0, 255).astype(np.uint8)


def random_maps(rng, Hc: int, Wc: int, outside=0.1):
    """Random fixed-point maps near the identity; about `outside` of the coordinates point outside the frame, -1 and
    Wc / Hc among them."""
    x = np.arange(Wc)[None, :] + rng.integers(-3, 4, (Hc, Wc))
    y = np.arange(Hc)[:, None] + rng.integers(-3, 4, (Hc, Wc))
    x, y = np.clip(x, 0, Wc - 2), np.clip(y, 0, Hc - 2)
    far = rng.random((Hc, Wc)) < outside
    kind = rng.integers(0, 6, (Hc, Wc))
    x = np.where(far & (kind == 0), -1, x)
    x = np.where(far & (kind == 1), Wc, x)
    x = np.where(far & (kind == 2), Wc - 1, x)  # the right tap is outside
    y = np.where(far & (kind == 3), -1, y)
    y = np.where(far & (kind == 4), Hc, y)
    x = np.where(far & (kind == 5), -7, x)
    map1 = np.stack([x, y], axis=-1).astype(np.int16)
    map2 = rng.integers(0, 1024, (Hc, Wc)).astype(np.uint16)
    return map1, map2


def rectify_maps(mtx, dist, R, P, image_size):
    """Pixel by pixel: (P[:, :3] R)^-1 (u, v, 1), normalise, radial k1..k6 and tangential p1, p2 distortion, project
    through mtx, quantise round_half_even(32 * coord) -> (map1 int16 [h, w, 2], map2 uint16 [h, w])."""
    w, h = image_size
    d = list(np.asarray(dist, dtype=np.float64).reshape(-1)) if dist is not None else []
    k1, k2, p1, p2, k3, k4, k5, k6 = (d + [0.0] * 8)[:8]
    inv = np.linalg.inv(np.asarray(P, dtype=np.float64)[:3, :3] @ (np.eye(3) if R is None else np.asarray(R, np.float64)))
    map1 = np.zeros((h, w, 2), dtype=np.int16)
    map2 = np.zeros((h, w), dtype=np.uint16)
    for v in range(h):
        for u in range(w):
            X = inv[0, 0] * u + inv[0, 1] * v + inv[0, 2]
            Y = inv[1, 0] * u + inv[1, 1] * v + inv[1, 2]
            Z = inv[2, 0] * u + inv[2, 1] * v + inv[2, 2]
            x, y = X / Z, Y / Z
            r2 = x * x + y * y
            radial = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
            xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            qx = int(np.rint(32.0 * (mtx[0][0] * xd + mtx[0][2])))
            qy = int(np.rint(32.0 * (mtx[1][1] * yd + mtx[1][2])))
            map1[v, u] = (qx >> 5, qy >> 5)
            map2[v, u] = ((qy & 31) << 5) | (qx & 31)
    return map1, map2


def compose(code: np.ndarray, lut: np.ndarray, Hc: int, Wc: int) -> np.ndarray:
    """cv2.resize(applyColorMap(code), (Wc, Hc), INTER_LINEAR) as defined here: float64 bilinear of lut[code], round
    half to even."""
    return np.clip(np.rint(resize_bilinear(lut[code].astype(np.float64), Hc, Wc)), 0, 255).astype(np.uint8)


def nearest_mask(mask: np.ndarray, Hc: int, Wc: int) -> np.ndarray:
    H, W = mask.shape
    sy = np.minimum(np.arange(Hc) * H // Hc, H - 1)
    sx = np.minimum(np.arange(Wc) * W // Wc, W - 1)
    return mask[sy][:, sx]


def codes(values: np.ndarray, lo: float, hi: float) -> np.ndarray:
    """colorize_scalar_map's uint8 codes for a given range (numpy float32 arithmetic, Python-float scalars)."""
    valid = np.isfinite(values) & (values > 0.0)
    scale = max(float(hi) - float(lo), 1e-6)
    with np.errstate(all="ignore"):
        out = (np.clip((values - float(lo)) / scale, 0.0, 1.0) * 255.0).astype(np.uint8)
    out[~valid] = 0
    return out


# ---------------------------------------------------------------------- the host post stage (numpy float32)
def depth_from_disparity(disp: np.ndarray, focal_px: float, baseline_m: float) -> np.ndarray:
    ok = np.isfinite(disp) & (disp > 1e-6)
    out = np.full(disp.shape, np.nan, dtype=np.float32)
    out[ok] = (focal_px * baseline_m) / disp[ok]
    return out


def contour_mask(depth: np.ndarray, step: float, lo: float, hi: float) -> np.ndarray:
    ok = np.isfinite(depth) & (depth > lo) & (depth <= hi)
    with np.errstate(all="ignore"):
        bins = np.where(ok, np.floor((np.clip(depth, lo, hi) - lo) / step), -1.0).astype(np.int32)
    edge = np.zeros(depth.shape, dtype=bool)
    edge[:-1] |= ok[:-1] & ok[1:] & (bins[:-1] != bins[1:])
    edge[:, :-1] |= ok[:, :-1] & ok[:, 1:] & (bins[:, :-1] != bins[:, 1:])
    return edge.astype(np.uint8) * 255


def center_median(m: np.ndarray, window: int) -> float:
    h, w = m.shape
    half = max(1, window // 2)
    p = m[max(0, h // 2 - half):min(h, h // 2 + half + 1), max(0, w // 2 - half):min(w, w // 2 + half + 1)]
    p = p[np.isfinite(p) & (p > 0.0)]
    return float(np.median(p)) if p.size else float("nan")


def host_post(disp, logvar, view, lut_a, lut_b, focal_px, baseline_m, window=15):
    """Everything the host loop does after the forward, for one frame with depth on: depth, confidence, contour
    overlay, the two colour images at the view size and the three centre medians."""
    Hc, Wc = view.shape[:2]
    depth = depth_from_disparity(disp, focal_px, baseline_m)
    with np.errstate(all="ignore"):
        conf = np.exp(-0.5 * logvar)
    mask = nearest_mask(contour_mask(depth, 0.5, 0.0, 10.0), Hc, Wc)
    left = view.copy()
    left[mask > 0] = (0, 255, 0)
    depth_vis = compose(codes(depth, 0.0, 10.0), lut_a, Hc, Wc)
    conf_vis = compose(codes(conf, 0.0, 5.0), lut_b, Hc, Wc)
    return depth_vis, conf_vis, left, (center_median(disp, window), center_median(depth, window),
                                       center_median(conf, window))
