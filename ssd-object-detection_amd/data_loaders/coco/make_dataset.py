"""COCODataLoader with the reference reader's contract (data_loaders/coco/make_dataset.py:32-36, 100-134, 160 of the
reference), read with `json` alone: no pycocotools, no scikit-image.

    COCODataLoader(dataset_root, prefetch=1, shuffle=True, mini_batch=0, decode="device")
    .get_dataset()            -> (train, val) splits: iterables of (image, cls f32[n], box f32[n,4], crowd u8[n]); boxes are
                                 (cx, cy, w, h) in PIXELS of the image (reference :132), crowd is the annotations' `iscrowd`
    .get_names_and_colors()   -> (names, colors)

Files: <root>/annotations/instances_{train,val}2017.json and <root>/{train,val}2017/<file_name> (reference :46-49).
Classes: the index of a category is the rank of its id among the file's categories sorted by id (COCO's 80 ids run to 90 with
gaps); the names are the file's own.  The two files must list the same categories (the reference asserts it, :92).
Images without annotations are skipped (reference :126-128).  mini_batch > 0 keeps the first mini_batch image records of each
file, before shuffling (reference :108-113).  Shuffling is seeded: pass k of a split uses the same order in every process.

decode="device": `image` is an ops.EncodedImage -- the file's bytes with (H, W, 3) as its .shape, from the JPEG frame header
    where the decoder reads it, else from the annotation file; SSDObjectDetectionModel decodes whole batches with
    ops.image_arena (Huffman on host threads, the rest on the device).  Nothing on this path needs Pillow unless a file is a
    stream the decoder refuses (progressive, CMYK, ...), which the Pillow fallback of ops.decode_jpeg_batch then decodes.
decode="host":   `image` is the decoded uint8 array [H,W,3]; needs Pillow.

A split's lazy() yields zero-argument callables, one per kept sample, in iteration order: no file is opened until one is
called, so a data-parallel rank reads only its own images.  A missing image file raises FileNotFoundError: unlike the
reference (:118-120) this loader never fetches `coco_url`, or anything else, from a network."""
import json
import os

import numpy as np

from ... import ops

EncodedImage = ops.EncodedImage                    # what decode="device" yields as a sample's image


def _load_annotations(path):
    if not os.path.exists(path):
        raise ValueError("COCO annotation file does not exist: %s" % path)         # the reference's check(), :52-55
    with open(path) as f:
        doc = json.load(f)
    cats = sorted(((int(c["id"]), str(c["name"])) for c in doc["categories"]))
    by_image = {}
    for a in doc["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    return doc["images"], by_image, cats


class _CocoSplit:
    def __init__(self, images, by_image, class_of, image_root, shuffle, mini_batch, decode, seed):
        if mini_batch:
            images = images[:int(mini_batch)]
        # the records that have annotations, in file order
        self._records = [(im, by_image[im["id"]]) for im in images if by_image.get(im["id"])]
        self._class_of, self._root, self._shuffle, self._decode, self._seed = class_of, image_root, shuffle, decode, seed
        self._epoch = 0

    def __len__(self):
        return len(self._records)

    def _sample(self, i):
        im, anns = self._records[i]
        path = os.path.join(self._root, im["file_name"])
        if not os.path.isfile(path):
            raise FileNotFoundError("COCO image file does not exist: %s (this loader does not download images)" % path)
        with open(path, "rb") as f:
            data = f.read()
        if self._decode == "host":
            image = ops._pil_decode(data)
        else:
            try:
                h = ops.jpeg_info(data)
                image = ops.EncodedImage(data, h["height"], h["width"])
            except NotImplementedError:                              # the fallback's business; the size is in the annotations
                image = ops.EncodedImage(data, im["height"], im["width"])
            except ValueError as e:
                raise ValueError("%s: %s" % (path, e)) from None
        box = np.array([a["bbox"] for a in anns], np.float32).reshape(-1, 4)
        box[:, :2] += box[:, 2:] / np.float32(2.0)                   # top-left -> centre, in pixels (reference :132)
        cls = np.array([self._class_of[a["category_id"]] for a in anns], np.float32)
        crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in anns], np.uint8)
        return image, cls, box, crowd

    def lazy(self):
        order = np.arange(len(self._records))
        if self._shuffle:
            np.random.default_rng(self._seed + self._epoch).shuffle(order)
        self._epoch += 1
        for i in order:
            yield lambda i=int(i): self._sample(i)

    def __iter__(self):
        for thunk in self.lazy():
            yield thunk()


class COCODataLoader:
    def __init__(self, dataset_root, prefetch=1, shuffle=True, mini_batch=0, decode="device"):
        """prefetch: accepted for the reference's signature; batches are assembled by SSDObjectDetectionModel.get_train_set"""
        if decode not in ("device", "host"):
            raise ValueError("decode must be 'device' or 'host', not %r" % (decode,))
        if decode == "host":
            try:
                import PIL  # noqa: F401
            except ImportError as e:
                raise ImportError("decode='host' needs Pillow; decode='device' does not") from e
        ann = os.path.join(dataset_root, "annotations")
        train_images, train_by_image, train_cats = _load_annotations(os.path.join(ann, "instances_train2017.json"))
        val_images, val_by_image, val_cats = _load_annotations(os.path.join(ann, "instances_val2017.json"))
        if train_cats != val_cats:
            raise ValueError("the train and val annotation files list different categories: %s"
                             % sorted(set(train_cats) ^ set(val_cats))[:8])
        self._names = [name for _, name in train_cats]
        class_of = {cid: i for i, (cid, _) in enumerate(train_cats)}
        rng = np.random.default_rng(0)
        self._colors = [rng.integers(80, 240, 3).tolist() for _ in self._names]
        self._train_set = _CocoSplit(train_images, train_by_image, class_of, os.path.join(dataset_root, "train2017"), shuffle,
                                     mini_batch, decode, 977)
        self._val_set = _CocoSplit(val_images, val_by_image, class_of, os.path.join(dataset_root, "val2017"), shuffle,
                                   mini_batch, decode, 1977)

    def get_dataset(self):
        return self._train_set, self._val_set

    def get_names_and_colors(self):
        return self._names, self._colors
