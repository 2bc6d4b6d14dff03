from .make_dataset import VOC_CLASSES, EncodedImage, VOCDataLoader

__all__ = ["VOCDataLoader", "VOC_CLASSES", "EncodedImage"]
