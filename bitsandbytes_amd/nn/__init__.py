from . import parametrize
from .modules import (
    Embedding4bit,
    EmbeddingFP4,
    EmbeddingNF4,
    FFN4bit,
    Linear4bitLoRA,
    Linear4bitMultiLoRA,
    Linear4bit,
    LinearFP4,
    LinearNF4,
    MoERouter,
    Params4bit,
    linear4bit_group_forward,
)

__all__ = ["Linear4bit", "LinearFP4", "LinearNF4", "Params4bit", "Embedding4bit", "EmbeddingFP4", "EmbeddingNF4",
           "parametrize", "linear4bit_group_forward", "FFN4bit", "Linear4bitLoRA", "Linear4bitMultiLoRA", "MoERouter"]
