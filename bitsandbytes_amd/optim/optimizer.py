"""8-bit blockwise optimizers over :func:`bitsandbytes_amd.functional.optimizer_update_8bit_blockwise`: one fused launch per
parameter tensor and step (csrc/optim8.hip).

Per-parameter state, created at the first step, under the reference's keys (bitsandbytes/optim/optimizer.py:492-531), so state
dicts interchange: ``step`` (int), ``state1`` / ``state2`` (uint8 codes, zeros at the start), ``qmap1`` (signed dynamic map) /
``qmap2`` (unsigned dynamic map), ``absmax1`` / ``absmax2`` (fp32, one per 256 elements, zeros at the start). A tensor with fewer
than ``min_8bit_size`` elements keeps fp32 ``state1`` / ``state2`` and goes through ``optimizer_update_32bit``. One-state
optimizers hold no ``state2`` / ``qmap2`` / ``absmax2``.

Not served (NotImplementedError): ``max_unorm > 0``, percentile clipping, paged states, per-parameter overrides.
"""
from __future__ import annotations

from collections import defaultdict
from copy import deepcopy
from itertools import chain

import torch

from .. import functional as F

_WRAPPED_KEY = "__bnb_optimizer_quant_state__"  # the reference's state_dict() nests its quantization tensors under this key


class Optimizer8bit(torch.optim.Optimizer):
    """Base: ``optimizer_name`` is the kernel's update rule, ``betas`` its (beta1, beta2)."""

    def __init__(self, optimizer_name: str, params, lr: float, betas, eps: float, weight_decay: float, min_8bit_size: int = 4096,
                 percentile_clipping: int = 100, max_unorm: float = 0.0):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"invalid hyper-parameters: lr={lr}, betas={betas}, eps={eps}, weight_decay={weight_decay}")
        if max_unorm > 0.0:
            raise NotImplementedError("max_unorm > 0 (update-norm clipping) is not served: it needs a global norm pass")
        if percentile_clipping != 100:
            raise NotImplementedError("percentile clipping is not served")
        if optimizer_name not in ("adam", "momentum", "rmsprop", "adagrad", "lion"):
            raise NotImplementedError(f"optimizer {optimizer_name!r} is not served (adam, momentum, rmsprop, adagrad, lion are)")
        self.optimizer_name = optimizer_name
        self.min_8bit_size = min_8bit_size
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    def _init_state(self, p: torch.Tensor) -> dict:
        state = self.state[p]
        state["step"] = 0
        n, two = p.numel(), self.optimizer_name == "adam"
        names = ("1", "2") if two else ("1",)
        if n < self.min_8bit_size:
            for i in names:
                state["state" + i] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
            return state
        for i in names:
            state["state" + i] = torch.zeros_like(p, dtype=torch.uint8, memory_format=torch.contiguous_format)
            state["qmap" + i] = F.create_dynamic_map(signed=i == "1").to(p.device)
            state["absmax" + i] = torch.zeros(-(n // -256), dtype=torch.float32, device=p.device)
        return state

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_contiguous():
                    raise ValueError("parameters must be contiguous: they are updated in place")
                state = self.state[p]
                if len(state) == 0:
                    state = self._init_state(p)
                state["step"] += 1
                grad = p.grad.contiguous()
                if state["state1"].dtype == torch.float32:
                    F.optimizer_update_32bit(self.optimizer_name, grad, p, state["state1"], beta1, group["eps"], state["step"], group["lr"],
                                             state.get("state2"), beta2, weight_decay=group["weight_decay"])
                else:
                    F.optimizer_update_8bit_blockwise(self.optimizer_name, grad, p, state["state1"], state.get("state2"), beta1, beta2, 0.0, 0.0,
                                                      group["eps"], state["step"], group["lr"], state["qmap1"], state.get("qmap2"),
                                                      state["absmax1"], state.get("absmax2"), group["weight_decay"])
        return loss

    def load_state_dict(self, state_dict) -> None:
        """torch's own loader casts every state tensor to the parameter's dtype, which would destroy uint8 codes and fp32 absmax
        under a 16-bit parameter: the tensors are moved to the parameter's device and otherwise kept as saved. Accepts the
        reference's nested form as well. torch's load_state_dict pre and post hooks run as they do in its loader."""
        for hook in getattr(self, "_optimizer_load_state_dict_pre_hooks", {}).values():
            replaced = hook(self, state_dict)
            state_dict = state_dict if replaced is None else replaced
        state_dict = deepcopy(state_dict)
        groups, saved = self.param_groups, state_dict["param_groups"]
        if len(groups) != len(saved) or any(len(g["params"]) != len(s["params"]) for g, s in zip(groups, saved)):
            raise ValueError("loaded state dict does not match the optimizer's parameter groups")
        id_map = dict(zip(chain.from_iterable(s["params"] for s in saved), chain.from_iterable(g["params"] for g in groups)))
        state = defaultdict(dict)  # (a parameter without saved state gets its state at its first step)
        for key, value in state_dict["state"].items():
            if key not in id_map:  # state that belongs to no parameter is kept as it is, as torch and the reference do
                state[key] = value
                continue
            value.update(value.pop(_WRAPPED_KEY, {}))
            param = id_map[key]
            state[param] = {k: v.to(param.device) if isinstance(v, torch.Tensor) else v for k, v in value.items()}
        for g, s in zip(groups, saved):
            s["params"] = g["params"]
        self.__setstate__({"state": state, "param_groups": saved})
        for hook in getattr(self, "_optimizer_load_state_dict_post_hooks", {}).values():
            hook(self)


class Adam8bit(Optimizer8bit):
    """Adam with decoupled weight decay, as the reference's Adam8bit applies it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **kwargs):
        super().__init__("adam", params, lr, betas, eps, weight_decay, **kwargs)


class AdamW8bit(Optimizer8bit):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kwargs):
        super().__init__("adam", params, lr, betas, eps, weight_decay, **kwargs)


class Lion8bit(Optimizer8bit):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, **kwargs):
        super().__init__("lion", params, lr, betas, 0.0, weight_decay, **kwargs)


class SGD8bit(Optimizer8bit):
    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, **kwargs):
        if momentum == 0 or dampening != 0 or nesterov:
            raise NotImplementedError("SGD8bit serves momentum != 0 without dampening or Nesterov momentum")
        super().__init__("momentum", params, lr, (momentum, 0.0), 0.0, weight_decay, **kwargs)


class RMSprop8bit(Optimizer8bit):
    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, **kwargs):
        if alpha == 0 or momentum != 0 or centered:
            raise NotImplementedError("RMSprop8bit serves alpha != 0 without momentum or centering")
        super().__init__("rmsprop", params, lr, (alpha, 0.0), eps, weight_decay, **kwargs)


class Adagrad8bit(Optimizer8bit):
    def __init__(self, params, lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10, **kwargs):
        if lr_decay != 0 or initial_accumulator_value != 0:
            raise NotImplementedError("Adagrad8bit serves lr_decay == 0 and initial_accumulator_value == 0")
        super().__init__("adagrad", params, lr, (0.0, 0.0), eps, weight_decay, **kwargs)
