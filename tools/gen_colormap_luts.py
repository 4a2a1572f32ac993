#!/usr/bin/env python3
"""Generate stereo_depth_estimation_amd/colormaps.json: the [4][256][3] uint8 BGR tables of the live display's
colormaps (turbo, inferno, magma, viridis; the order of live.COLORMAP_NAMES), round_half_even(255 * c) of
matplotlib's listed colormaps. OpenCV's COLORMAP_* tables come from the same published data; their bytes are not
compared here (no cv2)."""

import json
from pathlib import Path

import numpy as np
from matplotlib import colormaps

NAMES = ("turbo", "inferno", "magma", "viridis")
OUT = Path(__file__).resolve().parents[1] / "stereo_depth_estimation_amd" / "colormaps.json"


def main() -> None:
    luts = []
    for name in NAMES:
        rgb = np.asarray(colormaps[name].colors, dtype=np.float64)
        assert rgb.shape == (256, 3), (name, rgb.shape)
        luts.append(np.rint(255.0 * rgb).astype(np.uint8)[:, ::-1])
    rows = ",\n".join(json.dumps(lut.tolist(), separators=(",", ":")) for lut in luts)
    OUT.write_text('{"names": %s,\n"bgr": [\n%s\n]}\n' % (json.dumps(list(NAMES)), rows))
    print(OUT, np.asarray(json.loads(OUT.read_text())["bgr"], dtype=np.uint8).shape)


if __name__ == "__main__":
    main()
