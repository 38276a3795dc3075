"""8-bit blockwise optimizers (one fused HIP launch per parameter tensor: csrc/optim8.hip)."""
from .optimizer import Adagrad8bit, Adam8bit, AdamW8bit, Lion8bit, Optimizer8bit, RMSprop8bit, SGD8bit

__all__ = ["Optimizer8bit", "Adam8bit", "AdamW8bit", "Lion8bit", "SGD8bit", "RMSprop8bit", "Adagrad8bit"]
