"""Input pipelines: tf.data-style Dataset, MNIST idx (offline synthetic fallback), HBM-resident
array / image sets (the latter with fused on-device augmentation), synthetic ImageNet / MLM
generators for benchmarks."""
from . import images, mnist
from .dataset import Dataset, Iterator, NativeBatchDataset
from .device import DeviceArrayDataset
from .images import DeviceImageDataset, ImageAugment
from .synthetic import SyntheticImageNet, SyntheticMLM

__all__ = ["images", "mnist", "Dataset", "DeviceArrayDataset", "DeviceImageDataset",
           "ImageAugment", "Iterator", "NativeBatchDataset", "SyntheticImageNet", "SyntheticMLM"]
