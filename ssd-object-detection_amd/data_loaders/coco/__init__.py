from .make_dataset import COCODataLoader, EncodedImage

__all__ = ["COCODataLoader", "EncodedImage"]
