"""Optimizers: fused flat-buffer applies (north-star models)."""
from .fused import FusedSGD, FusedAdam, FusedAdagrad, FusedLAMB, FusedLARS, make_optimizer  # noqa: F401
