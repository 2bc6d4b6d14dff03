"""VOCDataLoader: PASCAL VOC from a VOCdevkit tree, with the reader contract of data_loaders/coco (no reference counterpart:
the reference names "voc" only to refuse it).  Read with `xml.etree.ElementTree` from the standard library alone.

    VOCDataLoader(dataset_root, train=(("2007", "trainval"), ("2012", "trainval")), val=(("2007", "test"),), shuffle=True,
                  mini_batch=0, decode="device", use_difficult=True)
    .get_dataset()            -> (train, val) splits: iterables of (image, cls f32[n], box f32[n,4], difficult u8[n]); boxes are
                                 (cx, cy, w, h) in PIXELS of the image
    .get_names_and_colors()   -> (names, colors)

Files: per (year, set) pair <root>/VOC<year>/ImageSets/Main/<set>.txt lists the image ids, <root>/VOC<year>/Annotations/<id>.xml
holds an image's objects and <root>/VOC<year>/JPEGImages/<id>.jpg the image.  A split is its pairs' lists one after the other.
A pair whose list file is absent raises ValueError naming the path -- the defaults are the SSD paper's VOC07+12 trainval and
VOC2007 test; give other pairs for a tree that holds less.
Classes: the twenty VOC names in the devkit's alphabetical order are the indices 0..19 (VOC_CLASSES); any other name raises
ValueError naming the file.
Boxes: VOC's corners are 1-based and inclusive, so the covered continuous box is x = xmin - 1, w = xmax - xmin + 1 (y and h
likewise) and its centre x + w / 2.
use_difficult=False drops the `difficult` objects from the TRAIN splits only (evaluation needs them: a detection on a difficult
box is neither right nor wrong); an image left without objects is skipped, as an image without any object always is.
mini_batch > 0 keeps the first mini_batch ids of each split, before shuffling.  Shuffling is seeded: pass k of a split uses the
same order in every process.

decode="device": `image` is an ops.EncodedImage -- the file's bytes with (H, W, 3) as its .shape, from the JPEG frame header
    where the decoder reads it, else from the annotation's <size>; SSDObjectDetectionModel decodes whole batches with
    ops.image_arena.
decode="host":   `image` is the decoded uint8 array [H,W,3]; needs Pillow.

A split's lazy() yields zero-argument callables, one per kept sample, in iteration order: no image file is opened until one is
called.  A missing image file raises FileNotFoundError; nothing here ever opens a connection."""
import os
import xml.etree.ElementTree as ET

import numpy as np

from ... import ops

EncodedImage = ops.EncodedImage

VOC_CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
               "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
_CLASS_OF = {name: i for i, name in enumerate(VOC_CLASSES)}


def _read_annotation(path):
    """(cls f32 [n], box f32 [n,4] centre form in pixels, difficult u8 [n], (height, width) or None) of one annotation file."""
    if not os.path.isfile(path):
        raise ValueError("VOC annotation file does not exist: %s" % path)
    try:
        root = ET.parse(path).getroot()
    except ET.ParseError as e:
        raise ValueError("%s: %s" % (path, e)) from None
    cls, box, hard = [], [], []
    for obj in root.findall("object"):
        name = (obj.findtext("name") or "").strip()
        if name not in _CLASS_OF:
            raise ValueError("%s: unknown VOC class %r" % (path, name))
        bb = obj.find("bndbox")
        try:
            xmin, ymin, xmax, ymax = (np.float32(float(bb.findtext(k))) for k in ("xmin", "ymin", "xmax", "ymax"))
        except (AttributeError, TypeError, ValueError):
            raise ValueError("%s: object %r has no usable bndbox" % (path, name)) from None
        one = np.float32(1.0)
        x, y, w, h = xmin - one, ymin - one, xmax - xmin + one, ymax - ymin + one
        cls.append(_CLASS_OF[name])
        box.append((x + w / np.float32(2.0), y + h / np.float32(2.0), w, h))
        hard.append(1 if int((obj.findtext("difficult") or "0").strip() or 0) else 0)
    size = root.find("size")
    try:
        hw = (int(size.findtext("height")), int(size.findtext("width")))
    except (AttributeError, TypeError, ValueError):
        hw = None
    return np.array(cls, np.float32), np.array(box, np.float32).reshape(-1, 4), np.array(hard, np.uint8), hw


class _VocSplit:
    def __init__(self, dataset_root, pairs, shuffle, mini_batch, decode, seed, use_difficult):
        ids = []
        for year, name in pairs:
            base = os.path.join(dataset_root, "VOC%s" % year)
            listing = os.path.join(base, "ImageSets", "Main", "%s.txt" % name)
            if not os.path.isfile(listing):
                raise ValueError("VOC image set file does not exist: %s" % listing)
            with open(listing) as f:
                ids.extend((base, line.split()[0]) for line in f if line.strip())
        if mini_batch:
            ids = ids[:int(mini_batch)]
        # the records that have objects, in list order
        self._records = []
        for base, image_id in ids:
            cls, box, hard, hw = _read_annotation(os.path.join(base, "Annotations", image_id + ".xml"))
            if not use_difficult:
                live = hard == 0
                cls, box, hard = cls[live], box[live], hard[live]
            if len(cls):
                self._records.append((os.path.join(base, "JPEGImages", image_id + ".jpg"), cls, box, hard, hw))
        self._shuffle, self._decode, self._seed = shuffle, decode, seed
        self._epoch = 0

    def __len__(self):
        return len(self._records)

    def _sample(self, i):
        path, cls, box, hard, hw = self._records[i]
        if not os.path.isfile(path):
            raise FileNotFoundError("VOC image file does not exist: %s (this loader does not download images)" % path)
        with open(path, "rb") as f:
            data = f.read()
        if self._decode == "host":
            image = ops._pil_decode(data)
        else:
            try:
                h = ops.jpeg_info(data)
                image = ops.EncodedImage(data, h["height"], h["width"])
            except NotImplementedError:                              # the fallback's business; the size is in the annotation
                if hw is None:
                    raise ValueError("%s: no <size> in the annotation of a stream the decoder does not read" % path) from None
                image = ops.EncodedImage(data, hw[0], hw[1])
            except ValueError as e:
                raise ValueError("%s: %s" % (path, e)) from None
        return image, cls.copy(), box.copy(), hard.copy()

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


class VOCDataLoader:
    def __init__(self, dataset_root, train=(("2007", "trainval"), ("2012", "trainval")), val=(("2007", "test"),), shuffle=True,
                 mini_batch=0, decode="device", use_difficult=True):
        if decode not in ("device", "host"):
            raise ValueError("decode must be 'device' or 'host', not %r" % (decode,))
        if decode == "host":
            try:
                import PIL  # noqa: F401
            except ImportError as e:
                raise ImportError("decode='host' needs Pillow; decode='device' does not") from e
        self._names = list(VOC_CLASSES)
        rng = np.random.default_rng(0)
        self._colors = [rng.integers(80, 240, 3).tolist() for _ in self._names]
        self._train_set = _VocSplit(dataset_root, train, shuffle, mini_batch, decode, 977, bool(use_difficult))
        self._val_set = _VocSplit(dataset_root, val, shuffle, mini_batch, decode, 1977, True)

    def get_dataset(self):
        return self._train_set, self._val_set

    def get_names_and_colors(self):
        return self._names, self._colors
