"""4-bit parametrisation of arbitrary module parameters (reference ``bitsandbytes/nn/parametrize.py``).

For weights that do not live in an ``nn.Linear`` (fused MoE expert tensors, for instance): the parameter
is replaced by its packed 4-bit bytes and a ``torch.nn.utils.parametrize`` hook hands the module the
dequantized tensor whenever it reads the attribute. One ``dequantize_4bit`` launch per access; while a
forward of the owning module is running the result is cached so that repeated reads cost nothing.
The state dict keeps the clean key layout of ``Linear4bit`` (``<name>`` + ``<name>.absmax`` + ...).
"""
from __future__ import annotations

from typing import Any, Literal, Optional

import torch
import torch.nn as nn
import torch.nn.utils.parametrize as P

from .. import functional as F
from ..autograd._functions import matmul_4bit_experts as _matmul_4bit_experts
from ..autograd._functions import moe_ffn_4bit as _moe_ffn_4bit


class Bnb4bitParametrization(nn.Module):
    """``forward(packed) -> dequantized`` for one parameter; owns that parameter's :class:`QuantState`."""

    def __init__(self, quant_state: F.QuantState):
        super().__init__()
        self.quant_state = quant_state

    @torch.no_grad()
    def forward(self, quantized_param: torch.Tensor) -> torch.Tensor:
        return F.dequantize_4bit(quantized_param, self.quant_state)


def _require_parameter(module: nn.Module, param_name: str) -> nn.Parameter:
    if not hasattr(module, param_name):
        raise AttributeError(f"Module does not have parameter '{param_name}'")
    param = getattr(module, param_name)
    if not isinstance(param, nn.Parameter):
        raise TypeError(f"Parameter '{param_name}' is not an instance of nn.Parameter")
    return param


def replace_parameter_4bit_prequantized(module: nn.Module, param_name: str, qs_dict: dict[str, Any],
                                        device: torch.device) -> None:
    """The parameter already holds packed bytes (loaded from a checkpoint); ``qs_dict`` is its quant-state
    dict in the ``QuantState.as_dict`` layout."""
    _require_parameter(module, param_name)
    state = F.QuantState.from_dict(qs_dict, device=device)
    _attach(module, param_name, state)


def replace_parameter_4bit(module: nn.Module, param_name: str, compress_statistics: bool = False,
                           quant_type: Literal["nf4", "fp4"] = "nf4", blocksize: Optional[int] = None) -> None:
    """Quantize ``module.<param_name>`` in place (the tensor must already be on the HIP device) and make
    reads of the attribute return the dequantized value."""
    original = _require_parameter(module, param_name)
    packed, state = F.quantize_4bit(original.data, blocksize=blocksize, compress_statistics=compress_statistics,
                                    quant_type=quant_type)
    setattr(module, param_name, nn.Parameter(packed, requires_grad=False))
    del original
    _attach(module, param_name, state)


def _attach(module: nn.Module, param_name: str, state: F.QuantState) -> None:
    # unsafe=True: the parametrization changes shape and dtype (packed bytes -> fp tensor)
    P.register_parametrization(module, param_name, Bnb4bitParametrization(state), unsafe=True)
    _register_parametrization_hooks(module, param_name)


def _register_parametrization_hooks(module: nn.Module, param_name: str) -> None:
    """State-dict hook (clean key layout) + the forward hook pair that caches the dequantized tensor for the
    duration of one forward of the owning module (same private name as the reference's helper: its tests
    register the pair directly)."""
    if hasattr(module, "register_state_dict_post_hook"):
        module.register_state_dict_post_hook(_StateDictHook(param_name))
    module.register_forward_pre_hook(_enable_parametrization_cache)
    # always_call: also runs when forward raises or is aborted (non-reentrant activation checkpointing stops
    # its recompute mid-forward), otherwise the enable count leaks and the cache is never cleared again
    module.register_forward_hook(_disable_parametrization_cache, always_call=True)


def _enable_parametrization_cache(module: nn.Module, inputs: tuple[Any, ...]) -> None:
    P._cache_enabled += 1


def _disable_parametrization_cache(module: nn.Module, inputs: tuple[Any, ...], output: Any) -> None:
    # never below zero: with always_call the hook may fire without a matching pre-hook, and a negative
    # counter would read as "enabled" forever and pin every dequantized tensor in memory
    P._cache_enabled = max(0, P._cache_enabled - 1)
    if not P._cache_enabled:
        P._cache = {}


def _expert_state(module: nn.Module, param_name: str, what: str):
    """(packed parameter, QuantState) of a parametrized 3D expert tensor."""
    if not P.is_parametrized(module, param_name):
        raise ValueError(f"'{param_name}' is not a parametrized parameter of the module")
    plist = module.parametrizations[param_name]
    hook = next((h for h in plist if isinstance(h, Bnb4bitParametrization)), None)
    if hook is None or hook.quant_state is None:
        raise ValueError(f"'{param_name}' carries no 4-bit parametrization")
    if len(hook.quant_state.shape) != 3:
        raise ValueError(f"{what}: '{param_name}' must be a 3D [E, N, K] expert tensor, got {list(hook.quant_state.shape)}")
    return plist.original, hook.quant_state


def matmul_4bit_experts(module: nn.Module, param_name: str, x: torch.Tensor, expert_ids: torch.Tensor,
                        bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The expert projections of a decode step on a parametrized ``[E, N, K]`` expert tensor WITHOUT the dequantizing read of the
    attribute: ``y[t, s] = x_row(t, s) @ W[expert_ids[t, s]].T (+ bias[expert_ids[t, s]])`` from the packed bytes, one launch
    (:func:`bitsandbytes_amd.matmul_4bit_experts`; ``x`` is ``[T, K]`` or ``[T, S, K]``, ``expert_ids`` ``[T, S]`` on the device,
    an id outside ``[0, E)`` gives a row of zeros). Where the kernel does not serve the geometry the dequantized attribute is
    indexed and multiplied instead - also without looking at the ids on the host. Inference only."""
    packed, state = _expert_state(module, param_name, "matmul_4bit_experts")
    E, N, K = (int(v) for v in state.shape)
    if x.shape[-1] != K:
        raise ValueError(f"matmul_4bit_experts: x inner dim ({x.shape[-1]}) must equal K ({K}); expert tensors in [E, K, N] "
                         "orientation are not supported")
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("matmul_4bit_experts is inference only (no autograd formula): call it under torch.no_grad()")
    from ..backends.hip import gemm_4bit_experts_supported

    served = (x.is_cuda and gemm_4bit_experts_supported(x.dtype, E, N, K, state.blocksize)
              and (not state.nested or state.state2.blocksize == 256) and packed.data_ptr() % 16 == 0)
    if served:
        return _matmul_4bit_experts(x, packed.data, state, expert_ids, bias=bias)
    # unfused: the dequantized stack, gathered per pair (ids clamped for the gather, masked rows zeroed afterwards)
    with torch.no_grad():
        W = getattr(module, param_name).to(x.dtype)
        valid = (expert_ids >= 0) & (expert_ids < E)
        safe = expert_ids.clamp(0, E - 1).long()
        xs = x if x.dim() == expert_ids.dim() + 1 else x.unsqueeze(-2).expand(*expert_ids.shape, K)
        y = torch.matmul(W[safe], xs.unsqueeze(-1)).squeeze(-1)
        if bias is not None:
            y = y + bias[safe]
        return y * valid.unsqueeze(-1).to(y.dtype)


def moe_ffn_4bit(module: nn.Module, gate_up_name: str, down_name: str, x: torch.Tensor, expert_ids: torch.Tensor,
                 routing_weights: torch.Tensor, gate_up_bias: Optional[torch.Tensor] = None,
                 down_bias: Optional[torch.Tensor] = None, gated: str = "chunked") -> torch.Tensor:
    """The gated-SiLU expert FFN block of a decode step on parametrized ``[E, 2 I, H]`` / ``[E, H, I]`` expert tensors, from the
    packed bytes: two launches and one slot sum (:func:`bitsandbytes_amd.moe_ffn_4bit`; ``x`` ``[T, H]``, ``expert_ids`` and
    ``routing_weights`` ``[T, S]`` on the device; returns ``[T, H]``). Where the kernel does not serve one of the two geometries the
    block is composed of :func:`matmul_4bit_experts` of this module and torch's ``silu``, ``*`` and ``sum`` - also without looking at
    the ids or the weights on the host. Inference only."""
    if gated not in ("chunked", "interleaved"):
        raise ValueError(f"moe_ffn_4bit: gated must be 'chunked' or 'interleaved', got {gated!r}")
    gu_packed, gu_state = _expert_state(module, gate_up_name, "moe_ffn_4bit")
    dn_packed, dn_state = _expert_state(module, down_name, "moe_ffn_4bit")
    if expert_ids.dim() != 2 or tuple(routing_weights.shape) != tuple(expert_ids.shape):
        raise ValueError(f"moe_ffn_4bit: expert_ids and routing_weights must both be [T, S], got {tuple(expert_ids.shape)} and "
                         f"{tuple(routing_weights.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or routing_weights.requires_grad):
        raise RuntimeError("moe_ffn_4bit is inference only (no autograd formula): call it under torch.no_grad()")
    from ..backends.hip import gemm_4bit_experts_ffn_supported

    def served(packed, state, mode):
        E, N, K = (int(v) for v in state.shape)
        return (gemm_4bit_experts_ffn_supported(x.dtype, E, N, K, state.blocksize, mode)
                and (not state.nested or state.state2.blocksize == 256) and packed.data_ptr() % 16 == 0)

    if (x.is_cuda and routing_weights.dtype in (torch.float32, x.dtype) and served(gu_packed, gu_state, gated)
            and served(dn_packed, dn_state, "none")):
        return _moe_ffn_4bit(x, gu_packed.data, gu_state, dn_packed.data, dn_state, expert_ids, routing_weights,
                             gate_up_bias=gate_up_bias, down_bias=down_bias, gated=gated)
    with torch.no_grad():
        h = matmul_4bit_experts(module, gate_up_name, x, expert_ids, bias=gate_up_bias)
        g, u = (h[..., 0::2], h[..., 1::2]) if gated == "interleaved" else h.chunk(2, dim=-1)
        y = matmul_4bit_experts(module, down_name, torch.nn.functional.silu(g) * u, expert_ids, bias=down_bias)
        # (a dropped slot contributes zeros whatever its weight, as in the fused form)
        E = int(gu_state.shape[0])
        w = torch.where((expert_ids >= 0) & (expert_ids < E), routing_weights, torch.zeros_like(routing_weights))
        return (y * w.unsqueeze(-1).to(y.dtype)).sum(dim=1)


class _StateDictHook:
    """Rename ``parametrizations.<name>.original`` back to ``<name>`` and add the packed quant state."""

    def __init__(self, param_name: str):
        self.param_name = param_name

    def __call__(self, module: nn.Module, state_dict: dict[str, Any], prefix: str, local_metadata: Any) -> None:
        name = self.param_name
        raw_key = f"{prefix}parametrizations.{name}.original"
        if raw_key not in state_dict:
            return
        state_dict[f"{prefix}{name}"] = state_dict.pop(raw_key)
        assert P.is_parametrized(module, name)
        for hook in module.parametrizations[name]:
            if isinstance(hook, Bnb4bitParametrization):
                if hook.quant_state is not None:
                    for k, v in hook.quant_state.as_dict(packed=True).items():
                        state_dict[f"{prefix}{name}.{k}"] = v
                return
        raise AssertionError("Parametrization not found for the parameter.")
