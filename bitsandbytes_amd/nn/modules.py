"""``Params4bit`` / ``Linear4bit`` — the module-level face of the 4-bit path
(reference ``bitsandbytes/nn/modules.py:213-716``).

Same contract as the reference: a ``Linear4bit`` holds its weight as a :class:`Params4bit`; the fp
weight is quantised lazily the first time the parameter is moved to a (HIP) device; ``forward`` is
``matmul_4bit(x, weight, bias, quant_state)``; the state-dict layout (``weight`` packed bytes plus
``weight.absmax``, ``weight.quant_map``, optional ``weight.nested_*`` and the JSON blob
``weight.quant_state.bitsandbytes__{nf4,fp4}``) is byte-compatible, so checkpoints written by either
implementation load in the other.
"""
from __future__ import annotations

import copy
import logging
from typing import Any, Optional

import torch
from torch import nn

from .. import functional as F
from .._ops import MOE_GROUP_SCORE_CODES, MOE_SCORING_CODES
from ..autograd import matmul_4bit
from ..functional import QuantState

logger = logging.getLogger(__name__)

# QuantState attributes re-exported on the parameter so that FSDP's dotted-FQN traversal
# (getattr(weight, "absmax") ...) finds them. Implemented as properties, not __getattr__, which
# keeps torch.compile from graph-breaking on tensor subclasses (reference modules.py:261-339).
def _qs_property(attr_path: str, exported_name: str, none_ok: bool = False):
    def getter(self):
        obj = self.__dict__.get("quant_state")
        if obj is not None:
            for part in attr_path.split("."):
                obj = getattr(obj, part, None)
                if obj is None:
                    break
            if obj is not None or none_ok:
                return obj
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{exported_name}'")

    return property(getter)


def _rebuild_params4bit(state):
    new = Params4bit.__new__(Params4bit, data=state["data"], requires_grad=state["requires_grad"])
    new.__setstate__(state)
    return new


class Params4bit(torch.nn.Parameter):
    def __new__(
        cls,
        data: Optional[torch.Tensor] = None,
        requires_grad: bool = False,  # quantised weights are frozen by default
        quant_state: Optional[QuantState] = None,
        blocksize: Optional[int] = None,
        compress_statistics: bool = True,
        quant_type: str = "fp4",
        quant_storage: torch.dtype = torch.uint8,
        module: Optional["Linear4bit"] = None,
        bnb_quantized: bool = False,
        **kwargs,
    ) -> "Params4bit":
        if data is None:
            data = torch.empty(0)
        self = torch.Tensor._make_subclass(cls, data, requires_grad)
        self.blocksize = 64 if blocksize is None else blocksize
        self.compress_statistics = compress_statistics
        self.quant_type = quant_type
        self.quant_state = quant_state
        self.quant_storage = quant_storage
        self.bnb_quantized = bnb_quantized
        self.data = data
        self.module = module
        return self

    # ---- QuantState proxies (FSDP state-dict traversal)
    absmax = _qs_property("absmax", "absmax")
    code = _qs_property("code", "code")
    quant_map = _qs_property("code", "quant_map")
    offset = _qs_property("offset", "offset", none_ok=True)
    state2 = _qs_property("state2", "state2", none_ok=True)
    nested_absmax = _qs_property("state2.absmax", "nested_absmax")
    nested_blocksize = _qs_property("state2.blocksize", "nested_blocksize")
    nested_quant_map = _qs_property("state2.code", "nested_quant_map")
    nested_dtype = _qs_property("state2.dtype", "nested_dtype")
    nested_offset = _qs_property("offset", "nested_offset", none_ok=True)

    # ---- pickling / copying
    _STATE_FIELDS = ("blocksize", "compress_statistics", "quant_type", "quant_state", "quant_storage",
                     "bnb_quantized", "module")

    def __getstate__(self):
        state = self.__dict__.copy()
        state["data"] = self.data
        state["requires_grad"] = self.requires_grad
        return state

    def __setstate__(self, state):
        self.requires_grad = state["requires_grad"]
        for f in self._STATE_FIELDS:
            setattr(self, f, state[f])
        self.data = state["data"]

    def __reduce_ex__(self, proto):
        # torch.nn.Parameter's default reduce rebuilds a plain Parameter; keep the subclass
        return (_rebuild_params4bit, (self.__getstate__(),))

    def __deepcopy__(self, memo):
        new = type(self).__new__(type(self))
        state = self.__getstate__()
        new.__setstate__(state)
        new.quant_state = copy.deepcopy(state["quant_state"])
        new.data = copy.deepcopy(state["data"])
        return new

    def __copy__(self):
        new = type(self).__new__(type(self))
        new.__setstate__(self.__getstate__())
        return new

    # ---- construction from a pre-quantised checkpoint
    @classmethod
    def from_prequantized(cls, data: torch.Tensor, quantized_stats: dict[str, Any], requires_grad: bool = False,
                          device="cuda", module: Optional["Linear4bit"] = None, **kwargs) -> "Params4bit":
        self = torch.Tensor._make_subclass(cls, data.to(device))
        self.requires_grad = requires_grad
        self.quant_state = QuantState.from_dict(qs_dict=quantized_stats, device=device)
        self.blocksize = self.quant_state.blocksize
        self.compress_statistics = self.quant_state.nested
        self.quant_type = self.quant_state.quant_type
        self.bnb_quantized = True
        self.quant_storage = data.dtype
        self.module = module
        if module is not None:
            module.quant_state = self.quant_state
        return self

    # ---- lazy quantisation on device move
    def _quantize(self, device):
        w = self.data.contiguous().to(device)
        packed, state = F.quantize_4bit(
            w,
            blocksize=self.blocksize,
            compress_statistics=self.compress_statistics,
            quant_type=self.quant_type,
            quant_storage=self.quant_storage,
        )
        self.data = packed
        self.quant_state = state
        if self.module is not None:
            self.module.quant_state = state
        self.bnb_quantized = True
        return self

    def cpu(self):
        return self.to(device="cpu")

    def cuda(self, device=None, non_blocking: bool = False):
        return self.to(device="cuda" if device is None else device, non_blocking=non_blocking)

    def to(self, *args, **kwargs):
        device, dtype, non_blocking, _ = torch._C._nn._parse_to(*args, **kwargs)
        if device is not None and device.type != "meta" and not self.bnb_quantized:
            return self._quantize(device)
        if self.quant_state is not None:
            self.quant_state.to(device)
        return Params4bit(
            super().to(device=device, dtype=dtype, non_blocking=non_blocking),
            requires_grad=self.requires_grad,
            quant_state=self.quant_state,
            blocksize=self.blocksize,
            compress_statistics=self.compress_statistics,
            quant_type=self.quant_type,
            quant_storage=self.quant_storage,
            bnb_quantized=self.bnb_quantized,
        )

    # torch.chunk / torch.split (FSDP sharding, fused-QKV splitting) must keep the metadata
    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        result = super().__torch_function__(func, types, args, kwargs)
        if func not in (torch.chunk, torch.split):
            return result
        src = args[0]

        def rewrap(t):
            return cls(
                data=t,
                requires_grad=src.requires_grad,
                quant_state=src.quant_state,
                blocksize=src.blocksize,
                compress_statistics=src.compress_statistics,
                quant_type=src.quant_type,
                quant_storage=src.quant_storage,
                module=src.module,
                bnb_quantized=src.bnb_quantized,
            )

        return tuple(rewrap(t) for t in result) if isinstance(result, tuple) else rewrap(result)


def fix_4bit_weight_quant_state_from_module(module: "Linear4bit") -> None:
    """FSDP and friends may replace the parameter by a plain tensor and lose ``quant_state``; the
    module keeps a copy so it can be put back (reference modules.py:487-501)."""
    if getattr(module.weight, "quant_state", None) is not None:
        return
    if getattr(module, "quant_state", None) is None:
        logger.warning(
            "FP4 quantization state not initialized. Please call .cuda() or .to(device) on the LinearFP4 layer first."
        )
    assert module.weight.shape[1] == 1
    if not isinstance(module.weight, Params4bit):
        module.weight = Params4bit(module.weight, quant_storage=module.quant_storage, bnb_quantized=True)
    module.weight.quant_state = module.quant_state


class _PreparedCall:
    """Owner of one handle of the C++ dispatcher's prepared-call table (csrc/torch_dispatch.cpp: linear4bit_prepare). The handle is
    released when THIS object dies, and the object never travels: ``copy.deepcopy`` / pickling of a module yield ``None`` in its
    place, so a copy (or a module loaded in another process) can never release - or call - the original's handle. The key is
    everything the prepared call captured: the quant state object, the STORAGE of weight and bias (``layer.bias.data = new`` keeps
    the Parameter object but changes ``data_ptr()``; in-place updates write the storage the prepared call aliases), dtypes."""

    __slots__ = ("handle", "quant_state", "weight_ptr", "bias_obj", "bias_ptr", "bias_dtype", "bias_grad", "compute_dtype")

    def __init__(self, handle, quant_state, weight, bias, compute_dtype):
        self.handle = handle
        self.quant_state = quant_state
        self.weight_ptr = weight.data_ptr()
        self.bias_obj = bias
        self.bias_ptr = None if bias is None else bias.data_ptr()
        self.bias_dtype = None if bias is None else bias.dtype
        self.bias_grad = bias is not None and bias.requires_grad
        self.compute_dtype = compute_dtype

    def matches(self, weight, bias, compute_dtype) -> bool:
        if self.handle is None or self.quant_state is not getattr(weight, "quant_state", None) or self.weight_ptr != weight.data_ptr():
            return False
        if bias is not self.bias_obj or self.compute_dtype is not compute_dtype:
            return False
        return bias is None or (bias.data_ptr() == self.bias_ptr and bias.dtype is self.bias_dtype
                                and bias.requires_grad == self.bias_grad)

    def release(self):
        handle, self.handle = self.handle, None
        if handle is not None:
            try:
                torch.ops.bitsandbytes_amd.linear4bit_release(handle)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass

    def __del__(self):
        self.release()

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_no_prepared_call, ())


def _no_prepared_call():
    return None


class Linear4bit(nn.Linear):
    """QLoRA-style 4-bit linear layer (reference modules.py:504-637). Load fp weights into it, then
    ``.to("cuda")`` quantises them on the MI355X."""

    def __init__(self, input_features, output_features, bias=True, compute_dtype=None, compress_statistics=True,
                 quant_type="fp4", quant_storage=torch.uint8, device=None):
        super().__init__(input_features, output_features, bias, device)
        self.weight = Params4bit(
            self.weight.data,
            requires_grad=False,
            compress_statistics=compress_statistics,
            quant_type=quant_type,
            quant_storage=quant_storage,
            module=self,
        )
        self.compute_dtype = compute_dtype
        self.compute_type_is_set = compute_dtype is not None
        self.quant_state = None
        self.quant_storage = quant_storage

    def set_compute_type(self, x: torch.Tensor) -> None:
        if x.dtype in (torch.float32, torch.bfloat16):
            # safe to compute in the input's dtype
            self.compute_dtype = x.dtype
        elif x.dtype == torch.float16 and self.compute_dtype in (None, torch.float32):
            single = x.numel() == x.shape[-1]
            logger.warning(
                "Input type into Linear4bit is torch.float16, but bnb_4bit_compute_dtype=torch.float32 (default). "
                + ("This will lead to slow inference." if single else "This will lead to slow inference or training speed.")
            )

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)  # weight (packed) and bias
        state = getattr(self.weight, "quant_state", None)
        if state is not None:
            for k, v in state.as_dict(packed=True).items():
                destination[prefix + "weight." + k] = v if keep_vars else v.detach()

    # ---- prepared call (MI355X): eager decode is host-bound - the Python below (quant-state repair, dtype policy, matmul_4bit,
    # a ten-argument op call) costs more than the 4 us kernel it launches. Once the layer is quantised on the device, its
    # call is prepared ONCE in the C++ dispatcher library (csrc/torch_dispatch.cpp: linear4bit_prepare) and every later
    # forward that needs no autograd is a two-argument op call; anything that changes the layer (a new weight / quant state /
    # bias object, a moved weight) drops the handle. Results are those of the code below, by construction: the prepared
    # call runs the same gemm_4bit kernel glue with the same dtype policy.
    _prepared = None  # a _PreparedCall (below) or None

    def _prepared_drop(self):
        prep = self.__dict__.pop("_prepared", None)
        if prep is not None:
            prep.release()

    def _apply(self, fn, recurse=True):
        # .to() / .cuda() / .cpu() / .half(): the prepared call holds the packed weight and its statistics alive on the device
        # they were on - drop it before anything moves, the next eager forward prepares again
        self._prepared_drop()
        return super()._apply(fn, recurse)

    def _prepared_make(self, weight, quant_state, bias):
        from ..backends import hip

        self._prepared_drop()
        if not hip.NATIVE_DISPATCH or not weight.is_cuda or len(quant_state.shape) != 2:
            return None
        if quant_state.nested and quant_state.state2.blocksize != 256:
            return None
        if quant_state.nested:
            absmax, a8, code, offset = quant_state.state2.absmax, quant_state.absmax, quant_state.state2.code, quant_state.offset
        else:
            absmax, a8, code, offset = quant_state.absmax, None, None, None
        handle = torch.ops.bitsandbytes_amd.linear4bit_prepare(
            weight.data.view(-1, 1) if weight.dtype == torch.uint8 else weight.data, list(quant_state.shape), absmax, quant_state.blocksize,
            quant_state.quant_type, None if bias is None else bias.data, a8, code, offset, self.compute_dtype)
        prep = _PreparedCall(handle, quant_state, weight, bias, self.compute_dtype)
        self.__dict__["_prepared"] = prep
        return prep

    def forward(self, x: torch.Tensor):
        prep = self._prepared
        if prep is not None and x.is_cuda:
            if (prep.matches(self._parameters["weight"], self._parameters["bias"], self.compute_dtype)
                    and not (torch.is_grad_enabled() and (x.requires_grad or prep.bias_grad))
                    and not torch.compiler.is_compiling()):
                return torch.ops.bitsandbytes_amd.linear4bit_prepared(x, prep.handle)
        fix_4bit_weight_quant_state_from_module(self)
        quant_state = self.weight.quant_state

        if not self.compute_type_is_set:
            self.set_compute_type(x)
            self.compute_type_is_set = True

        inp_dtype = x.dtype
        if self.compute_dtype is not None:
            x = x.to(self.compute_dtype)

        bias = self.bias
        if bias is not None:
            if bias.dtype != x.dtype:
                bias.data = bias.data.to(x.dtype)
            bias = bias.to(self.compute_dtype)

        if (x.is_cuda and quant_state is not None and self.compute_type_is_set and not torch.compiler.is_compiling()
                and K_matches(x, quant_state)):
            # (prepared for the NEXT call; this one takes the ordinary path)
            self._prepared_make(self.weight, quant_state, self.bias)
        return matmul_4bit(x, self.weight, bias=bias, quant_state=quant_state).to(inp_dtype)


def K_matches(x: torch.Tensor, quant_state) -> bool:
    """The [N, K] orientation matmul_4bit's fused path expects (the legacy [K, N] layout keeps the ordinary path)."""
    return len(quant_state.shape) == 2 and x.shape[-1] == quant_state.shape[1]


def linear4bit_group_forward(layers, x: torch.Tensor):
    """``[layer(x) for layer in layers]`` for :class:`Linear4bit` layers that consume the same input (Q/K/V, gate/up).
    Same dtype policy as :meth:`Linear4bit.forward`; when every layer computes in the same dtype the matmuls go through
    :func:`bitsandbytes_amd.matmul_4bit_grouped` - one launch for a decode-sized batch on MI355X - and the outputs are
    bit-identical to calling the layers one by one."""
    from ..autograd import matmul_4bit_grouped

    layers = list(layers)
    # eager decode: every layer already holds a prepared call (csrc/torch_dispatch.cpp) -> ONE native call for the group
    if x.is_cuda and not torch.compiler.is_compiling():
        preps = [layer._prepared for layer in layers]
        if all(prep is not None and prep.matches(layer._parameters["weight"], layer._parameters["bias"], layer.compute_dtype)
               for prep, layer in zip(preps, layers)) and not (torch.is_grad_enabled() and (x.requires_grad or any(p.bias_grad for p in preps))):
            return list(torch.ops.bitsandbytes_amd.linear4bit_group_prepared(x, [p.handle for p in preps]))
    for layer in layers:
        fix_4bit_weight_quant_state_from_module(layer)
        if not layer.compute_type_is_set:
            layer.set_compute_type(x)
            layer.compute_type_is_set = True
    dtypes = {layer.compute_dtype for layer in layers}
    if len(dtypes) != 1:
        return [layer(x) for layer in layers]
    compute_dtype = dtypes.pop()
    inp_dtype = x.dtype
    xc = x if compute_dtype is None else x.to(compute_dtype)
    biases = []
    for layer in layers:
        bias = layer.bias
        if bias is not None:
            if bias.dtype != xc.dtype:
                bias.data = bias.data.to(xc.dtype)
            bias = bias.to(compute_dtype)
        biases.append(bias)
    if x.is_cuda and not torch.compiler.is_compiling():
        for layer in layers:  # (prepared for the NEXT call, as Linear4bit.forward does)
            qs = layer.weight.quant_state
            if qs is not None and layer._prepared is None and K_matches(xc, qs):
                layer._prepared_make(layer.weight, qs, layer.bias)
    ys = matmul_4bit_grouped(xc, [layer.weight for layer in layers], [layer.weight.quant_state for layer in layers], biases)
    return [y.to(inp_dtype) for y in ys]


class FFN4bit(nn.Module):
    """One dense gated-SiLU FFN block, ``down(silu(gate(x)) * up(x))`` (Llama, Mistral, Qwen, Phi-3), as TWO launches for a decode
    step on one GPU: the gate and up rows live in ONE interleaved ``[2 F, H]`` matrix (``functional.interleave_gate_up_4bit``) and
    the activation is the epilogue of its matmul (:func:`bitsandbytes_amd.ffn_4bit`). Outputs are bit-identical to the three
    :class:`Linear4bit` layers with torch's ``F.silu(g) * u``, whatever the batch: calls the gated launch does not serve (more than
    16 rows, fp32, shapes whose plain call runs another kernel family) compose the plain matmul on the interleaved matrix with
    torch's ``silu`` and ``*``. Inference only.

    Build it with :meth:`from_linears` AFTER the checkpoint is loaded and the layers are quantized on the device. The block is not
    part of any state dict: its buffers are derived from the members', which keep owning what a checkpoint stores. The interleaved
    matrix is a second copy of the gate / up packed weights (``F * H`` bytes) plus their statistics as fp32 (``4 / blocksize`` bytes
    per weight, nested or not); with ``keep_members=False`` the two members' packed buffers are released, so the block does not
    double its gate / up memory - the two layers cannot be called on their own afterwards."""

    def __init__(self, gate_up: torch.Tensor, gate_up_state, down: "Linear4bit", gate_up_bias: Optional[torch.Tensor] = None,
                 compute_dtype=None):
        super().__init__()
        self.register_buffer("gate_up", gate_up, persistent=False)
        self.register_buffer("gate_up_absmax", gate_up_state.absmax, persistent=False)
        self.register_buffer("gate_up_bias", gate_up_bias, persistent=False)
        self.gate_up_state = gate_up_state
        self.compute_dtype = compute_dtype
        # (the members are referenced, not registered: they stay where the model holds them, and state_dict() of the block is empty)
        object.__setattr__(self, "down", down)
        object.__setattr__(self, "members", None)

    @classmethod
    def from_linears(cls, gate: "Linear4bit", up: "Linear4bit", down: "Linear4bit", keep_members: bool = False) -> "FFN4bit":
        for layer in (gate, up, down):
            fix_4bit_weight_quant_state_from_module(layer)
            if getattr(layer.weight, "quant_state", None) is None:
                raise ValueError("FFN4bit.from_linears: the layers must be quantized (load the checkpoint and move the model to the device first)")
        if gate.compute_dtype != up.compute_dtype or gate.compute_dtype != down.compute_dtype:
            raise ValueError("FFN4bit.from_linears: gate, up and down must share one compute dtype")
        if gate.out_features != up.out_features or gate.out_features != down.in_features or gate.in_features != up.in_features:
            raise ValueError("FFN4bit.from_linears: gate / up must be [F, H] layers and down must take what they produce")
        packed, state = F.interleave_gate_up_4bit(gate.weight.data, gate.weight.quant_state, up.weight.data, up.weight.quant_state)
        bias = None
        if gate.bias is not None or up.bias is not None:
            ref = gate.bias if gate.bias is not None else up.bias
            parts = [b.detach() if b is not None else torch.zeros_like(ref) for b in (gate.bias, up.bias)]
            bias = torch.stack([parts[0], parts[1].to(parts[0].dtype)], dim=1).reshape(-1).contiguous()  # interleaved like the rows
        block = cls(packed, state, down, bias, gate.compute_dtype)
        if keep_members:
            object.__setattr__(block, "members", (gate, up))
        else:
            for layer in (gate, up):
                layer._prepared_drop()  # (a prepared call keeps the packed weight alive)
                layer.weight.data = torch.empty(0, dtype=layer.weight.dtype, device=layer.weight.device)
        return block

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self.gate_up_state.absmax = self.gate_up_absmax  # (the state's absmax IS the moved buffer)
        return out

    def forward(self, x: torch.Tensor):
        from ..autograd import ffn_4bit, matmul_4bit

        down = self.down
        fix_4bit_weight_quant_state_from_module(down)
        inp_dtype = x.dtype
        cd = self.compute_dtype
        xc = x if cd is None else x.to(cd)
        gb = self.gate_up_bias
        if gb is not None and gb.dtype != xc.dtype:
            gb = gb.to(xc.dtype)
        if xc.dtype != inp_dtype:
            # a compute dtype other than the input's: the members round g and u to the input dtype before the activation
            y = matmul_4bit(xc, self.gate_up, self.gate_up_state, bias=gb).to(inp_dtype)
            return down(torch.nn.functional.silu(y[..., 0::2]) * y[..., 1::2])
        db = down.bias
        if db is not None and db.dtype != xc.dtype:
            db = db.to(xc.dtype)
        return ffn_4bit(xc, self.gate_up, self.gate_up_state, down.weight, down.weight.quant_state, gate_up_bias=gb, down_bias=db)


class Linear4bitLoRA(nn.Module):
    """A :class:`Linear4bit` base layer with ONE LoRA adapter beside it, ``base(x) + scaling * lora_B(lora_A(x))``, as TWO launches for
    a decode step: ``t = F.linear(x, lora_A)`` and the base layer's fused matmul with the adapter term as its epilogue
    (:func:`bitsandbytes_amd.matmul_4bit_lora`; its two-launch composition where the fused launch does not serve the call). Inference
    only; no dropout, no DoRA.

    Build it with :meth:`from_linear` AFTER the checkpoint is loaded and the base layer is quantized on the device. The base layer is
    held by reference - its packed bytes are not copied - and the adapter matrices are cast ONCE to the compute dtype, contiguous. The
    module is not part of any state dict: the base layer and the adapter keep owning what a checkpoint stores."""

    def __init__(self, base: "Linear4bit", lora_A: torch.Tensor, lora_B: torch.Tensor, scaling: float):
        super().__init__()
        object.__setattr__(self, "base", base)  # (referenced, not registered: state_dict() of this module is empty)
        self.register_buffer("lora_A", lora_A, persistent=False)
        self.register_buffer("lora_B", lora_B, persistent=False)
        self.scaling = float(scaling)
        # True: t = x @ lora_A^T comes from the library's own launch (bitsandbytes_amd.lora_shrink) instead of F.linear. Off by
        # default: the two differ in the order of the fp32 sum, so the default forward keeps the bits it had.
        self.fused_shrink = False

    @classmethod
    def from_linear(cls, base: "Linear4bit", lora_A: torch.Tensor, lora_B: torch.Tensor, scaling: float) -> "Linear4bitLoRA":
        fix_4bit_weight_quant_state_from_module(base)
        if getattr(base.weight, "quant_state", None) is None:
            raise ValueError("Linear4bitLoRA.from_linear: the base layer must be quantized (load the checkpoint and move the model to the device first)")
        if lora_A.dim() != 2 or lora_B.dim() != 2 or lora_A.shape[1] != base.in_features or lora_B.shape[0] != base.out_features \
                or lora_A.shape[0] != lora_B.shape[1]:
            raise ValueError(f"Linear4bitLoRA.from_linear: lora_A must be [r, {base.in_features}] and lora_B [{base.out_features}, r], "
                             f"got {tuple(lora_A.shape)} and {tuple(lora_B.shape)}")
        cd = base.compute_dtype if base.compute_dtype is not None else lora_A.dtype
        dev = base.weight.device
        return cls(base, lora_A.detach().to(device=dev, dtype=cd).contiguous(), lora_B.detach().to(device=dev, dtype=cd).contiguous(), scaling)

    def forward(self, x: torch.Tensor, t: Optional[torch.Tensor] = None):
        """``t``: a precomputed ``x @ lora_A.T`` (``[*, r]``) - a caller that shrank the stacked ``lora_A`` of several layers that share
        ``x`` in one launch (``lora_shrink(x, stacked, splits=...)``) passes each member its part."""
        from ..autograd import lora_shrink, matmul_4bit_lora

        base = self.base
        fix_4bit_weight_quant_state_from_module(base)
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Linear4bitLoRA is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
        inp_dtype = x.dtype
        xc = x.to(self.lora_A.dtype)
        bias = base.bias
        if bias is not None:
            bias = bias.detach()
            if bias.dtype != xc.dtype:
                bias = bias.to(xc.dtype)
        if t is None:
            t = lora_shrink(xc, self.lora_A) if self.fused_shrink else torch.nn.functional.linear(xc, self.lora_A)
        elif t.dtype != xc.dtype:
            t = t.to(xc.dtype)
        return matmul_4bit_lora(xc, base.weight, base.weight.quant_state, t, self.lora_B, self.scaling, bias=bias).to(inp_dtype)


class Linear4bitMultiLoRA(nn.Module):
    """A :class:`Linear4bit` base layer with a STACK of LoRA adapters beside it for mixed-adapter decode batches: row ``m`` of ``x`` (a
    request) computes ``base(x[m]) + scalings[id] * lora_B[id](lora_A[id](x[m]))`` with ``id = adapter_ids[m]``; a row whose id is
    outside ``[0, A_n)`` has no adapter and gets ``base(x[m])``. TWO launches for a decode step, whatever the ids
    (:func:`bitsandbytes_amd.lora_shrink_ids`, :func:`bitsandbytes_amd.matmul_4bit_lora_ids`; their gather compositions where the fused
    launches do not serve the call). The ids stay on the device: ``forward`` captures in a graph and a replay follows ids written
    into the same buffer. Inference only; no dropout, no DoRA.

    ``lora_A``: ``[A_n, r, K]``, ``lora_B``: ``[A_n, N, r]``, ``scalings``: ``[A_n]`` - one rank for the stack, ``1 <= A_n <= 64``;
    :meth:`from_adapters` stacks adapters of different ranks. The base layer is held by reference, the stacks are cast ONCE to the
    compute dtype (``scalings`` to float32), and the module is not part of any state dict."""

    def __init__(self, base: "Linear4bit", lora_A: torch.Tensor, lora_B: torch.Tensor, scalings: torch.Tensor):
        super().__init__()
        if lora_A.dim() != 3 or lora_B.dim() != 3 or lora_A.shape[0] != lora_B.shape[0] or lora_A.shape[1] != lora_B.shape[2] \
                or tuple(scalings.shape) != (lora_A.shape[0],) or not 1 <= lora_A.shape[0] <= 64:
            raise ValueError(f"Linear4bitMultiLoRA: lora_A must be [A_n, r, K], lora_B [A_n, N, r] and scalings [A_n] with 1 <= A_n <= 64, "
                             f"got {tuple(lora_A.shape)}, {tuple(lora_B.shape)} and {tuple(scalings.shape)}")
        object.__setattr__(self, "base", base)  # (referenced, not registered: state_dict() of this module is empty)
        self.register_buffer("lora_A", lora_A, persistent=False)
        self.register_buffer("lora_B", lora_B, persistent=False)
        self.register_buffer("scalings", scalings, persistent=False)

    @classmethod
    def from_stacks(cls, base: "Linear4bit", lora_A: torch.Tensor, lora_B: torch.Tensor, scalings) -> "Linear4bitMultiLoRA":
        """From stacked tensors ``[A_n, r, K]``, ``[A_n, N, r]`` and ``A_n`` scalings (a tensor or a sequence of floats): moved to the
        base layer's device, cast to its compute dtype, contiguous."""
        fix_4bit_weight_quant_state_from_module(base)
        if getattr(base.weight, "quant_state", None) is None:
            raise ValueError("Linear4bitMultiLoRA: the base layer must be quantized (load the checkpoint and move the model to the device first)")
        if lora_A.dim() != 3 or lora_B.dim() != 3 or lora_A.shape[2] != base.in_features or lora_B.shape[1] != base.out_features:
            raise ValueError(f"Linear4bitMultiLoRA: lora_A must be [A_n, r, {base.in_features}] and lora_B [A_n, {base.out_features}, r], "
                             f"got {tuple(lora_A.shape)} and {tuple(lora_B.shape)}")
        cd = base.compute_dtype if base.compute_dtype is not None else lora_A.dtype
        dev = base.weight.device
        sc = torch.as_tensor(scalings, dtype=torch.float32).detach().to(device=dev).contiguous()
        return cls(base, lora_A.detach().to(device=dev, dtype=cd).contiguous(), lora_B.detach().to(device=dev, dtype=cd).contiguous(), sc)

    @classmethod
    def from_adapters(cls, base: "Linear4bit", adapters) -> "Linear4bitMultiLoRA":
        """``adapters``: a sequence of ``(lora_A_i [r_i, K], lora_B_i [N, r_i], scaling_i)`` - adapter ``i`` gets id ``i``. Adapters of
        different rank are stacked by ZERO-PADDING to the largest rank rounded up to a multiple of 8 (the kernels' granule): rows of
        zeros appended to ``lora_A_i``, columns of zeros to ``lora_B_i``. The padded adapter is equal in VALUE to the unpadded one - the
        extra terms of both sums are exact zeros - but bit-identity with a call on the unpadded adapter is not promised: the adapter
        sum's order depends on the rank."""
        adapters = list(adapters)
        if not 1 <= len(adapters) <= 64:
            raise ValueError(f"Linear4bitMultiLoRA.from_adapters: 1 ... 64 adapters, got {len(adapters)}")
        K, N = base.in_features, base.out_features
        for a, b, _ in adapters:
            if a.dim() != 2 or b.dim() != 2 or a.shape[1] != K or b.shape[0] != N or a.shape[0] != b.shape[1] or a.shape[0] < 1:
                raise ValueError(f"Linear4bitMultiLoRA.from_adapters: every adapter must be (lora_A [r, {K}], lora_B [{N}, r], scaling), "
                                 f"got {tuple(a.shape)} and {tuple(b.shape)}")
        r = -(-max(int(a.shape[0]) for a, _, _ in adapters) // 8) * 8
        A = torch.zeros(len(adapters), r, K, dtype=adapters[0][0].dtype, device=adapters[0][0].device)
        B = torch.zeros(len(adapters), N, r, dtype=adapters[0][1].dtype, device=adapters[0][1].device)
        for i, (a, b, _) in enumerate(adapters):
            A[i, :a.shape[0]] = a.detach().to(A.dtype)
            B[i, :, :b.shape[1]] = b.detach().to(B.dtype)
        return cls.from_stacks(base, A, B, [float(s) for _, _, s in adapters])

    @staticmethod
    def shrink_group(x: torch.Tensor, members, adapter_ids: torch.Tensor):
        """The ``t`` of several :class:`Linear4bitMultiLoRA` layers that share ``x`` (Q / K / V, gate / up) and the SAME adapter order in
        ONE launch: their ``lora_A`` stacks are concatenated per adapter into ``[A_n, sum r_i, K]`` (build the concatenation once and
        pass it instead of the members to avoid the copy: ``members`` may be ``(stacked, splits)``) and
        ``lora_shrink_ids(x, stacked, adapter_ids, splits)`` returns one contiguous ``[*, r_i]`` tensor per member - pass each to its
        member's ``forward(x, adapter_ids, t=...)``."""
        from ..autograd import lora_shrink_ids

        if isinstance(members, tuple) and len(members) == 2 and isinstance(members[0], torch.Tensor):
            stacked, splits = members
        else:
            stacked = torch.cat([m.lora_A for m in members], dim=1).contiguous()
            splits = [int(m.lora_A.shape[1]) for m in members]
        return lora_shrink_ids(x.to(stacked.dtype), stacked, adapter_ids, splits=tuple(splits))

    def forward(self, x: torch.Tensor, adapter_ids: torch.Tensor, t: Optional[torch.Tensor] = None):
        """``adapter_ids``: ``[*]`` with ``x``'s leading dims, int32 or int64, on ``x``'s device. ``t``: a precomputed mixed-adapter
        shrink (``[*, r]``, :meth:`shrink_group`)."""
        from ..autograd import lora_shrink_ids, matmul_4bit_lora_ids

        base = self.base
        fix_4bit_weight_quant_state_from_module(base)
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Linear4bitMultiLoRA is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
        inp_dtype = x.dtype
        xc = x.to(self.lora_A.dtype)
        bias = base.bias
        if bias is not None:
            bias = bias.detach()
            if bias.dtype != xc.dtype:
                bias = bias.to(xc.dtype)
        if t is None:
            t = lora_shrink_ids(xc, self.lora_A, adapter_ids)
        elif t.dtype != xc.dtype:
            t = t.to(xc.dtype)
        return matmul_4bit_lora_ids(xc, base.weight, base.weight.quant_state, t, self.lora_B, self.scalings, adapter_ids, bias=bias).to(inp_dtype)


class LinearFP4(Linear4bit):
    def __init__(self, input_features, output_features, bias=True, compute_dtype=None, compress_statistics=True,
                 quant_storage=torch.uint8, device=None):
        super().__init__(input_features, output_features, bias, compute_dtype, compress_statistics, "fp4",
                         quant_storage, device)


class LinearNF4(Linear4bit):
    def __init__(self, input_features, output_features, bias=True, compute_dtype=None, compress_statistics=True,
                 quant_storage=torch.uint8, device=None):
        super().__init__(input_features, output_features, bias, compute_dtype, compress_statistics, "nf4",
                         quant_storage, device)


class MoERouter(nn.Module):
    """The router (gate) of a mixture-of-experts block: ``forward(x)`` returns ``(ids, weights)``, ``[*, top_k]`` int32 and fp32 on
    ``x``'s device - what :func:`bitsandbytes_amd.moe_ffn_4bit` takes as ``expert_ids`` and ``routing_weights`` - in two launches where
    :func:`bitsandbytes_amd.moe_route` is served. ``scoring``: ``"softmax"`` (Mixtral, Qwen) or ``"sigmoid"`` (DeepSeek-V3, GLM);
    ``renormalize`` / ``scale``: the chosen scores divided by their sum, then times ``scale`` (``routed_scaling_factor``).
    ``n_group`` > 1: group-limited routing (DeepSeek-V2 / -V3, GLM) - the best ``topk_group`` of ``n_group`` contiguous expert groups,
    ranked by ``group_score`` (``"max"`` or ``"top2sum"``), then the top-k among their experts (:func:`bitsandbytes_amd.moe_route_grouped`).

    State-dict keys: ``weight`` ``[num_experts, hidden]`` - an ``nn.Linear`` gate's checkpoint loads as it is -, ``bias``
    ``[num_experts]`` with ``bias=True`` (added to the logits), and ``e_score_correction_bias`` ``[num_experts]`` fp32 with
    ``select_bias=True`` (added to the scores for the selection only). Inference only: the parameters do not require gradients.

    Dtypes: ``e_score_correction_bias`` STAYS fp32 under ``.to(dtype)`` / ``.half()`` / ``.bfloat16()`` (the kernel reads fp32; a cast
    would cost its precision and a launch per call) - only its device follows the module. The two-launch form needs ``weight`` in
    ``x``'s 16-bit dtype; a gate kept in fp32 under 16-bit activations computes its logits in fp32 from ``x`` cast up, through
    ``F.linear`` (:func:`bitsandbytes_amd.moe_route`)."""

    def __init__(self, hidden: int, num_experts: int, top_k: int, scoring: str = "softmax", renormalize: bool = True, scale: float = 1.0,
                 bias: bool = False, select_bias: bool = False, device=None, dtype=None, n_group: int = 1, topk_group: int = 1,
                 group_score: str = "top2sum"):
        super().__init__()
        if scoring not in MOE_SCORING_CODES:
            raise ValueError(f"MoERouter: scoring must be 'softmax' or 'sigmoid', got {scoring!r}")
        if not 1 <= int(top_k) <= int(num_experts):
            raise ValueError(f"MoERouter: top_k must be in [1, num_experts] = [1, {num_experts}], got {top_k}")
        self.n_group, self.topk_group, self.group_score = int(n_group), int(topk_group), group_score
        if self.n_group > 1:
            if group_score not in MOE_GROUP_SCORE_CODES:
                raise ValueError(f"MoERouter: group_score must be 'max' or 'top2sum', got {group_score!r}")
            if int(num_experts) % self.n_group != 0 or not 1 <= self.topk_group <= self.n_group:
                raise ValueError(f"MoERouter: n_group must divide num_experts = {num_experts} and topk_group be in [1, n_group], got "
                                 f"n_group={n_group}, topk_group={topk_group}")
            G = int(num_experts) // self.n_group
            if int(top_k) > self.topk_group * G or (group_score == "top2sum" and G < 2):
                raise ValueError(f"MoERouter: top_k must be at most topk_group * num_experts / n_group = {self.topk_group * G}, and "
                                 f"'top2sum' needs groups of at least 2 experts; got top_k={top_k}, {G} experts a group")
        self.hidden, self.num_experts, self.top_k = int(hidden), int(num_experts), int(top_k)
        self.scoring, self.renormalize, self.scale = scoring, bool(renormalize), float(scale)
        self.weight = nn.Parameter(torch.empty(self.num_experts, self.hidden, device=device, dtype=dtype), requires_grad=False)
        nn.init.normal_(self.weight, std=self.hidden ** -0.5)
        self.register_parameter("bias", nn.Parameter(torch.zeros(self.num_experts, device=device, dtype=dtype), requires_grad=False) if bias else None)
        self.register_buffer("e_score_correction_bias", torch.zeros(self.num_experts, device=device, dtype=torch.float32) if select_bias else None)

    def _apply(self, fn, recurse=True):
        kept = self.e_score_correction_bias
        super()._apply(fn, recurse)
        if kept is not None and self.e_score_correction_bias.dtype != torch.float32:
            # a dtype cast: the selection bias keeps its fp32 values and only follows the device
            self.e_score_correction_bias = kept.to(self.e_score_correction_bias.device)
        return self

    def forward(self, x: torch.Tensor):
        from ..autograd import moe_route, moe_route_grouped

        if self.n_group > 1:
            return moe_route_grouped(x, self.weight, self.top_k, self.n_group, self.topk_group, group_score=self.group_score, bias=self.bias,
                                     scoring=self.scoring, renormalize=self.renormalize, scale=self.scale,
                                     select_bias=self.e_score_correction_bias)
        return moe_route(x, self.weight, self.top_k, bias=self.bias, scoring=self.scoring, renormalize=self.renormalize, scale=self.scale,
                         select_bias=self.e_score_correction_bias)

    def extra_repr(self) -> str:
        text = (f"hidden={self.hidden}, num_experts={self.num_experts}, top_k={self.top_k}, scoring={self.scoring!r}, "
                f"renormalize={self.renormalize}, scale={self.scale}, bias={self.bias is not None}, "
                f"select_bias={self.e_score_correction_bias is not None}")
        if self.n_group > 1:
            text += f", n_group={self.n_group}, topk_group={self.topk_group}, group_score={self.group_score!r}"
        return text


class Embedding4bit(nn.Embedding):
    """4-bit embedding table (reference modules.py:880-978): load fp rows, ``.to("cuda")`` quantises them.

    Each row is a whole number of quantization blocks when ``embedding_dim % blocksize == 0``; the lookup is
    then ONE fused launch (gather the packed row + its scales, dequantize) instead of the reference's two
    ``F.embedding`` gathers plus ``dequantize_4bit`` - same values bit for bit. Otherwise the whole table is
    dequantized and indexed, as in the reference (slow path, warned about at construction)."""

    def __init__(self, num_embeddings, embedding_dim, dtype=None, quant_type="fp4", quant_storage=torch.uint8,
                 device=None):
        super().__init__(num_embeddings, embedding_dim, device=device, dtype=dtype)
        self.dtype = self.weight.data.dtype
        self.weight = Params4bit(
            self.weight.data,
            requires_grad=False,
            compress_statistics=None,
            quant_type=quant_type,
            quant_storage=quant_storage,
            module=self,
        )
        self.quant_state = None
        self.quant_storage = quant_storage
        if embedding_dim % self.weight.blocksize != 0:
            logger.warning(
                f"Embedding size {embedding_dim} is not divisible by block size {self.weight.blocksize}. "
                "This will lead to slow inference."
            )

    def _forward_with_partial_dequantize(self, input: torch.Tensor) -> torch.Tensor:
        state = self.weight.quant_state
        assert self.embedding_dim % state.blocksize == 0
        absmax = state.absmax
        if state.nested:  # un-nest the scales once per call; the row kernel takes plain fp32 absmax
            absmax = F.dequantize_blockwise(state.absmax, state.state2) + state.offset
            if absmax.dtype != torch.float32:
                absmax = absmax.float()
        if self.embedding_dim % 8 != 0 or input.dtype not in (torch.int32, torch.int64):
            # rows that are not whole packed dwords: compose the lookup from gathers like the reference
            packed = self.weight.data.view(torch.uint8).view(self.num_embeddings, self.embedding_dim // 2)
            rows = torch.nn.functional.embedding(input, packed).reshape(-1, 1)
            scales = torch.nn.functional.embedding(
                input, absmax.view(self.num_embeddings, self.embedding_dim // state.blocksize)
            ).reshape(-1)
            out = torch.ops.bitsandbytes.dequantize_4bit.default(
                rows, scales, state.blocksize, state.quant_type, (*input.shape, self.embedding_dim), state.dtype
            )
            return out.to(self.dtype)
        packed_rows = (self.weight.data.numel() * self.weight.data.element_size() * 2) // self.embedding_dim
        if packed_rows != self.num_embeddings or tuple(state.shape) != (self.num_embeddings, self.embedding_dim):
            raise RuntimeError(
                f"Embedding4bit: packed weight holds {packed_rows} rows of {self.embedding_dim}, quant_state.shape is "
                f"{tuple(state.shape)}, module expects ({self.num_embeddings}, {self.embedding_dim})"
            )
        out = torch.ops.bitsandbytes_amd.dequantize_4bit_rows.default(
            self.weight.data, absmax, input, self.embedding_dim, state.blocksize, state.quant_type, state.dtype
        )
        return out.to(self.dtype)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        raise NotImplementedError("Saving Embedding4bit module is not implemented")

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        fix_4bit_weight_quant_state_from_module(self)
        if self.embedding_dim % self.weight.quant_state.blocksize == 0:
            return self._forward_with_partial_dequantize(input)
        table = F.dequantize_4bit(self.weight.data, self.weight.quant_state)
        return torch.nn.functional.embedding(input, table).to(self.dtype)


class EmbeddingFP4(Embedding4bit):
    def __init__(self, num_embeddings, embedding_dim, dtype=None, quant_storage=torch.uint8, device=None):
        super().__init__(num_embeddings, embedding_dim, dtype=dtype, quant_type="fp4", quant_storage=quant_storage,
                         device=device)


class EmbeddingNF4(Embedding4bit):
    def __init__(self, num_embeddings, embedding_dim, dtype=None, quant_storage=torch.uint8, device=None):
        super().__init__(num_embeddings, embedding_dim, dtype=dtype, quant_type="nf4", quant_storage=quant_storage,
                         device=device)
