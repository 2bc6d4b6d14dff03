"""The JPEG fixtures of tests/golden/jpeg (written by gen_fixtures.py there), their oracle decode, their corrupted variants, and
a small COCO-shaped directory built from them.  Plain Python: importable without a GPU and without Pillow."""
import functools
import json
import os

import numpy as np

from tests import jpeg_oracle as J

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
SUPPORTED = ("c1x1", "c8x8", "c4x3_420", "c3x5_422", "c17x9_420", "c31x16_422", "c33x20_grey", "c83x61_444", "c83x61_422",
             "c83x61_420_rst", "c300x2", "c24x40_q1", "c24x40_q100")
UNSUPPORTED = ("progressive",)
KIND = {"c1x1": J.K420, "c8x8": J.K420, "c4x3_420": J.K420, "c3x5_422": J.K422, "c17x9_420": J.K420, "c31x16_422": J.K422,
        "c33x20_grey": J.GREY, "c83x61_444": J.K444, "c83x61_422": J.K422, "c83x61_420_rst": J.K420, "c300x2": J.K420,
        "c24x40_q1": J.K420, "c24x40_q100": J.K420}


@functools.lru_cache(None)
def data(name):
    with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(None)
def _decoded():
    with np.load(os.path.join(DIR, "decoded.npz")) as z:
        return {k: z[k] for k in z.files}


def decoded(name):
    """Pillow's decode of the fixture, uint8 [H,W,3] (committed; treat as read-only)"""
    return _decoded()[name]


@functools.lru_cache(None)
def oracle(name):
    """(coef int16 [ncoef], header) of the numpy oracle (cached; treat as read-only)"""
    return J.entropy_decode(data(name))


def scan_start(d):
    """offset of the first entropy-coded byte: behind the SOS segment"""
    p = 2
    while True:
        assert d[p] == 0xFF
        m, length = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        p += 2 + length
        if m == 0xDA:
            return p


def dht_offsets(d):
    p, out = 2, []
    while True:
        m, length = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        if m == 0xC4:
            out.append(p)
        if m == 0xDA:
            return out
        p += 2 + length


def corrupted(name):
    """[(label, bytes)] that must all be refused as corrupt (SSD_ERR_VALUE): the stream cut inside the headers, inside a
    segment, inside the entropy data and in front of the EOI; a Huffman table's count byte inverted (over-subscribed code);
    the first restart marker renumbered, and removed."""
    d = data(name)
    s = scan_start(d)
    out = [("cut at %d" % n, d[:n]) for n in sorted({0, 1, 3, 30, s - 5, s, s + (len(d) - s) // 2, len(d) - 2})]
    dht = dht_offsets(d)[0]
    flipped = bytearray(d)
    flipped[dht + 5] ^= 0xFF                                # the count of 1-bit codes: 255 codes of length 1
    out.append(("huffman count byte inverted", bytes(flipped)))
    rst = [i for i in range(s, len(d) - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]
    if rst:
        wrong = bytearray(d)
        wrong[rst[0] + 1] = 0xD0 + ((d[rst[0] + 1] - 0xD0 + 1) & 7)
        out.append(("restart marker renumbered", bytes(wrong)))
        out.append(("restart marker removed", d[:rst[0]] + d[rst[0] + 2:]))
    return out


# ---- images past one stride of the reconstruction kernels' loops -------------------------------------------------------------------
# k_jpeg_idct walks the 8x8 blocks of an image (all components) 64 x 256 = 16 384 at a time, k_jpeg_rgb its pixels 128 x 256 =
# 32 768 at a time (IDCT_GRID_X, RGB_GRID_X in csrc/jpeg.hip); the largest fixture has 264 blocks and 5 063 pixels.  No larger
# file is committed: the kernels take coefficients, so a large image is a fixture's block grid repeated.
IDCT_STRIDE, RGB_STRIDE = 64 * 256, 128 * 256
# name: (fixture, copies across, copies down, width, height).  4:4:4: 3 x 77 x 72 = 16 632 blocks (the last 248 of the Cr plane
# on a second trip), 348 881 pixels (eleven trips), neither extent a multiple of 8; 4:2:0: the fancy upsampling across block
# borders, 96 393 pixels (three trips)
LARGE = {"444": ("c83x61_444", 7, 9, 611, 571), "420": ("c83x61_420_rst", 4, 4, 381, 253)}


def tiled(name, tx, ty, width, height):
    """(coef int16 [ncoef], header) of an image whose every component plane is the fixture's grid of blocks repeated tx x ty
    times and cropped to width x height; the luma DC of copy (i, j) is raised by 3 ((7 j + i) % 5), so copies differ.  Its
    decode is jpeg_oracle.reconstruct of these coefficients (the oracle is Pillow's decode bit for bit on every fixture)."""
    coef, h = oracle(name)
    parts, bws, bhs, offs, off = [], [], [], [], 0
    for c in range(h["ncomp"]):
        bw, bh = h["blocks_w"][c], h["blocks_h"][c]
        blk = np.asarray(coef[h["coef_off"][c]:][:64 * bw * bh]).reshape(bh, bw, 64)
        big = np.tile(blk, (ty, tx, 1))
        if c == 0:
            step = 3 * ((7 * np.arange(ty)[:, None] + np.arange(tx)[None, :]) % 5)
            big[..., 0] += np.repeat(np.repeat(step, bh, 0), bw, 1).astype(np.int16)
        parts.append(big.reshape(-1))
        bws.append(bw * tx)
        bhs.append(bh * ty)
        offs.append(off)
        off += big.size
        need_w, need_h = (width, height) if c == 0 or h["kind"] == J.K444 else \
            ((width + 1) // 2, (height + 1) // 2 if h["kind"] == J.K420 else height)
        assert 0 < need_w <= 8 * bws[-1] and 0 < need_h <= 8 * bhs[-1], (c, need_w, need_h)      # the planes cover the image
    return np.concatenate(parts).astype(np.int16), dict(h, width=width, height=height, blocks_w=bws, blocks_h=bhs, coef_off=offs,
                                                        ncoef=off, restart=0)


# ---- a COCO-shaped directory ------------------------------------------------------------------------------------------------------
CATEGORIES = [(90, "zebra crossing"), (1, "person"), (3, "car")]            # non-contiguous ids, not sorted in the file
# eighty categories with gaps in their ids, for the model-level tests (the networks' heads are built for 80 classes)
CATEGORIES_80 = [(i, "kind %d" % i) for i in range(90, 0, -1) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]
TRAIN_IMAGES = ("c83x61_444", "c24x40_q100", "c83x61_420_rst", "c31x16_422", "c8x8", "c33x20_grey", "c83x61_422", "c17x9_420")
TRAIN_EMPTY = ("c8x8",)                                                     # no annotations: skipped
VAL_IMAGES = ("c83x61_422", "c300x2", "c24x40_q1", "c17x9_420", "c83x61_444")
VAL_EMPTY = ("c300x2",)


def _boxes(name, seed, categories):
    h, w = decoded(name).shape[:2]
    rng = np.random.default_rng(seed)
    n = 1 + seed % 3
    out = []
    for k in range(n):
        bw, bh = rng.uniform(0.3, 0.9) * w, rng.uniform(0.3, 0.9) * h
        x, y = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
        out.append(dict(bbox=[round(float(x), 2), round(float(y), 2), round(float(bw), 2), round(float(bh), 2)],
                        category_id=categories[(7 * seed + 3 * k) % len(categories)][0], iscrowd=1 if (seed + k) % 4 == 3 else 0, area=float(bw * bh)))
    return out


def build_coco(root, val_categories=None, missing=(), categories=CATEGORIES):
    """writes annotations/instances_{train,val}2017.json and {train,val}2017/<name>.jpg under root; returns
    {split: [(name, [annotation dicts])]} in file order, images without annotations included"""
    root = str(root)
    layout = {}
    ann_id = 1
    for split, names, empty in (("train", TRAIN_IMAGES, TRAIN_EMPTY), ("val", VAL_IMAGES, VAL_EMPTY)):
        os.makedirs(os.path.join(root, split + "2017"), exist_ok=True)
        os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
        images, annotations, layout[split] = [], [], []
        for i, name in enumerate(names):
            h, w = decoded(name).shape[:2]
            image_id = 1000 * (1 + (split == "val")) + 7 * i
            images.append(dict(id=image_id, file_name=name + ".jpg", height=int(h), width=int(w),
                               coco_url="http://invalid.invalid/" + name + ".jpg"))
            if name not in missing:
                with open(os.path.join(root, split + "2017", name + ".jpg"), "wb") as f:
                    f.write(data(name))
            anns = [] if name in empty else _boxes(name, i + (10 if split == "val" else 0), categories)
            for a in anns:
                a.update(image_id=image_id, id=ann_id)
                ann_id += 1
            annotations.extend(anns)
            layout[split].append((name, anns))
        cats = categories if split == "train" or val_categories is None else val_categories
        doc = dict(images=images, annotations=annotations[::-1],               # annotations in any order in the file
                   categories=[dict(id=i, name=n, supercategory="x") for i, n in cats])
        with open(os.path.join(root, "annotations", "instances_%s2017.json" % split), "w") as f:
            json.dump(doc, f)
    return layout


class DecodedReader:
    """The reader contract (data_loaders/ssd/make_dataset.py) over the same directory layout, yielding the committed decoded
    arrays: what a user's own reader with a host JPEG decoder would have produced."""

    def __init__(self, layout, categories=CATEGORIES):
        self.layout, self.categories = layout, sorted(categories)

    def _split(self, split):
        class_of = {cid: i for i, (cid, _) in enumerate(self.categories)}
        out = []
        for name, anns in self.layout[split]:
            if not anns:
                continue
            anns = sorted(anns, key=lambda a: -a["id"])                         # the file's order (build_coco reverses them)
            box = np.array([a["bbox"] for a in anns], np.float32).reshape(-1, 4)
            box[:, :2] += box[:, 2:] / np.float32(2.0)
            out.append((decoded(name), np.array([class_of[a["category_id"]] for a in anns], np.float32), box,
                        np.array([a["iscrowd"] for a in anns], np.uint8)))
        return out

    def get_dataset(self):
        return self._split("train"), self._split("val")

    def get_names_and_colors(self):
        return [n for _, n in self.categories], [[128, 128, 128]] * len(self.categories)
