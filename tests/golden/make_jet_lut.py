"""Rebuilds tests/golden/jet_lut.json, the 256-entry cv::COLORMAP_JET palette, from recorded reference output.

Run from the repo root:  python tests/golden/make_jet_lut.py [REFERENCE_DIR]      (default /root/reference, as DESIGN.md cites it)

The reference's images/iter_{0..9}.png are cv::imwrite output of toColorImage (main_sl_OFFICIAL.cpp:1159-1162): a depth plane
through cv::normalize(NORM_MINMAX, [0, 1]) -> convertTo(CV_8U, 255) -> cv::applyColorMap(COLORMAP_JET).  Every pixel is one
palette entry.  Each of the 256 distinct colours of an image lies within L1 distance 1 of exactly one entry of the closed-form jet
255 * clip(1.5 - |4 x - c|, 0, 1), x = i / 255, c = 3, 2, 1 for R, G, B, which gives its index; all ten images must give the same
256 colours.  The closed form itself is not the table: its ramp values are exact .5 ties that OpenCV's float arithmetic rounds one
way or the other, so the recorded colours are the fixture.  PNGs store RGB; the fixture stores BGR (OpenCV's channel order, and
what dcmt_colormap_jet returns).

Without the reference checkout this does nothing.  Not a test; never run on the GPU machine.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jet_lut.json")


def closed_form_rgb() -> np.ndarray:
    x = np.arange(256, dtype=np.float64)[:, None] / 255.0
    return 255.0 * np.clip(1.5 - np.abs(4.0 * x - np.array([3.0, 2.0, 1.0])[None, :]), 0.0, 1.0)


def palette_from_png(path: str) -> np.ndarray:
    from PIL import Image
    rgb = np.asarray(Image.open(path).convert("RGB")).reshape(-1, 3)
    cols = np.unique(rgb, axis=0)
    d = np.abs(cols[:, None, :].astype(np.float64) - closed_form_rgb()[None]).sum(-1)
    near = d <= 1.0 + 1e-9
    if not (near.sum(1) == 1).all():
        raise SystemExit(f"{path}: a colour is not within L1 distance 1 of exactly one closed-form entry")
    idx = near.argmax(1)
    if sorted(idx.tolist()) != list(range(256)):
        raise SystemExit(f"{path}: {len(cols)} colours do not cover the 256 indices one to one")
    lut = np.zeros((256, 3), np.uint8)
    lut[idx] = cols
    return lut


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    imgs = [os.path.join(ref, "images", f"iter_{k}.png") for k in range(10)]
    if not all(os.path.exists(p) for p in imgs):
        print(f"no reference images under {ref}: nothing to do")
        return
    luts = [palette_from_png(p) for p in imgs]
    for p, l in zip(imgs[1:], luts[1:]):
        if not np.array_equal(l, luts[0]):
            raise SystemExit(f"{p}: palette differs from iter_0.png")
    bgr = luts[0][:, ::-1]
    doc = {
        "header": "cv::COLORMAP_JET, 256 entries in index order, each [B, G, R] (OpenCV channel order; the source PNGs are RGB). "
                  "Recovered from the reference's recorded toColorImage output images/iter_{0..9}.png by tests/golden/make_jet_lut.py.",
        "bgr": bgr.tolist(),
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {OUT}: entry 0 BGR {bgr[0].tolist()}, entry 255 BGR {bgr[255].tolist()}")


if __name__ == "__main__":
    main()
