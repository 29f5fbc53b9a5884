"""TF1-compatible optimizers on flat fp32 buffers with fused HIP updates."""
from .base import FlatSpace, Optimizer, default_decay_filter, tf_adam_lr_t
from .optimizers import (SGD, AdagradOptimizer, AdamOptimizer, AdamWeightDecayOptimizer,
                         GradientDescentOptimizer, LAMBOptimizer, LARSOptimizer, MomentumOptimizer, clip_by_global_norm_,
                         cosine_decay, piecewise_constant, polynomial_decay)
from .moving_averages import ExponentialMovingAverage
from .sync_replicas import SyncReplicasOptimizer

__all__ = ["ExponentialMovingAverage", "FlatSpace", "Optimizer", "default_decay_filter", "tf_adam_lr_t", "SGD",
           "AdagradOptimizer", "AdamOptimizer", "AdamWeightDecayOptimizer",
           "GradientDescentOptimizer", "LAMBOptimizer",
           "LARSOptimizer", "MomentumOptimizer", "SyncReplicasOptimizer", "clip_by_global_norm_",
           "cosine_decay", "piecewise_constant", "polynomial_decay"]
