"""Writes the JPEG fixtures of this directory: the encoded files and decoded.npz, Pillow's (libjpeg's) decode of each as
uint8 [H,W,3].  Needs Pillow; the tests do not (they read what this wrote).  Run once:  python tests/golden/jpeg/gen_fixtures.py"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (width, height, content, save options).  Pillow's subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
CASES = {
    "c1x1": (1, 1, "mix", dict(quality=75)),
    "c8x8": (8, 8, "mix", dict(quality=75)),
    "c4x3_420": (4, 3, "mix", dict(quality=90, subsampling=2)),          # chroma plane two samples wide: replication
    "c3x5_422": (3, 5, "mix", dict(quality=90, subsampling=1)),
    "c17x9_420": (17, 9, "mix", dict(quality=50, subsampling=2)),
    "c31x16_422": (31, 16, "mix", dict(quality=80, subsampling=1)),
    "c33x20_grey": (33, 20, "grey", dict(quality=70)),
    "c83x61_444": (83, 61, "mix", dict(quality=90, subsampling=0)),
    "c83x61_422": (83, 61, "mix", dict(quality=60, subsampling=1)),
    "c83x61_420_rst": (83, 61, "mix", dict(quality=85, subsampling=2, optimize=True, restart_marker_blocks=5)),
    "c300x2": (300, 2, "mix", dict(quality=75, subsampling=2)),
    "c24x40_q1": (24, 40, "stripes", dict(quality=1)),
    "c24x40_q100": (24, 40, "stripes", dict(quality=100)),
    "progressive": (40, 24, "mix", dict(quality=75, progressive=True)),
}
UNSUPPORTED = ("progressive",)


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "stripes":
        img = np.zeros((h, w, 3), np.uint8)
        img[:, (xx[0] // 3) % 2 == 0] = (255, 0, 0)
        img[:, (xx[0] // 3) % 2 == 1] = (0, 255, 255)
        img[(yy[:, 0] // 5) % 3 == 0] = 255 - img[(yy[:, 0] // 5) % 3 == 0]
        return img
    grad = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1)
    noise = rng.integers(0, 256, (h, w, 3))
    img = np.where((xx[..., None] + 2 * yy[..., None]) % 7 < 3, noise, grad)
    img[(yy // 4) % 5 == 0] = np.where(xx[(yy // 4) % 5 == 0][:, None] % 2 == 0, 255, 0)      # saturated stripes
    img = img.astype(np.uint8)
    return img[..., 0] if kind == "grey" else img


def main():
    decoded = {}
    for seed, (name, (w, h, kind, opts)) in enumerate(CASES.items()):
        buf = io.BytesIO()
        Image.fromarray(content(kind, w, h, seed)).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(data)
        decoded[name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), np.uint8)
        print("%-16s %5d bytes" % (name, len(data)))
    np.savez_compressed(os.path.join(HERE, "decoded.npz"), **decoded)


if __name__ == "__main__":
    main()
