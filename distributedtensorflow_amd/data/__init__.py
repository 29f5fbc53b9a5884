"""Input pipelines: tf.data-style Dataset, MNIST idx (offline synthetic fallback), HBM-resident
array / image / token sets (images with fused on-device augmentation, tokens with fused
on-device masked-LM example creation), synthetic ImageNet / MLM generators for benchmarks."""
from . import images, mnist, tokens
from .dataset import Dataset, Iterator, NativeBatchDataset
from .device import DeviceArrayDataset
from .images import (DeviceImageDataset, ImageAugment, ImageMix, ImageRandAugment, MixedLabels,
                     mix_plan, randaugment_plan)
from .synthetic import SyntheticImageNet, SyntheticMLM
from .tokens import (DeviceTokenDataset, TokenMasking, causal_lm_targets, load_continuation,
                     load_token_arrays, wordpiece_continuation)

__all__ = ["images", "mnist", "tokens", "Dataset", "DeviceArrayDataset", "DeviceImageDataset",
           "DeviceTokenDataset", "ImageAugment", "ImageMix", "ImageRandAugment", "Iterator",
           "MixedLabels", "NativeBatchDataset", "SyntheticImageNet", "SyntheticMLM",
           "TokenMasking", "causal_lm_targets", "load_continuation", "load_token_arrays",
           "mix_plan",
           "randaugment_plan", "wordpiece_continuation"]
