"""``matmul_4bit`` and its autograd function — reference ``bitsandbytes/autograd/_functions.py:300-491``.

Forward is one ``bitsandbytes::gemm_4bit`` op call for every M (the op's MI355X kernel picks the
streaming dot kernel or an MFMA kernel); backward is ``grad_A = grad_out @ dequantize_4bit(B)`` - fused into one
launch on the HIP device for batches up to 128 rows (``bitsandbytes_amd::gemm_4bit_grad_input``,
``backends/hip.py: FUSED_BACKWARD_MAX_M``).
Double-quantised states pass their pieces straight into the op so the absmax reconstruction is
fused into the GEMM kernel.
"""
from __future__ import annotations

from collections.abc import Sequence
from typing import Optional
from warnings import warn

import torch

from .. import functional as F
from .._ops import MOE_GROUP_SCORE_CODES, MOE_SCORING_CODES


def _is_compiling() -> bool:
    return torch.compiler.is_compiling()


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """``t`` contiguous and 16-byte aligned, as the fused decode launches want their operands: a view that starts elsewhere (a slice
    of a larger buffer) is copied into storage of its own - one copy launch; the raw ops refuse such a view, and the compositions
    would hand it to another kernel family, with other bits."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _gemm_4bit_from_state(A: torch.Tensor, B: torch.Tensor, quant_state: F.QuantState, bias):
    """Call the gemm_4bit op with the (possibly nested) statistics of ``quant_state``."""
    if not quant_state.nested:
        return torch.ops.bitsandbytes.gemm_4bit.default(
            A, B, quant_state.shape, quant_state.absmax, quant_state.blocksize, quant_state.quant_type, bias=bias
        )
    if quant_state.state2.blocksize != 256:
        raise NotImplementedError("nested quantization with state2.blocksize != 256 is not supported")
    return torch.ops.bitsandbytes.gemm_4bit.default(
        A,
        B,
        quant_state.shape,
        quant_state.state2.absmax,
        quant_state.blocksize,
        quant_state.quant_type,
        bias=bias,
        absmax_8bit=quant_state.absmax,
        absmax_code=quant_state.state2.code,
        absmax_offset=quant_state.offset,
    )


def _grad_input_from_state(grad_output: torch.Tensor, B: torch.Tensor, state: F.QuantState) -> torch.Tensor:
    fused = (
        grad_output.is_cuda
        and grad_output.dtype in (torch.float16, torch.bfloat16)
        and len(state.shape) == 2
        and grad_output.shape[-1] == state.shape[0]
        and (not state.nested or state.state2.blocksize == 256)
        # double backward (create_graph=True: gradient penalties, Hessian-vector products): the fused op has no autograd formula
        # of its own; dequantize + matmul - the reference's formulation - is differentiable in grad_output
        and not (torch.is_grad_enabled() and grad_output.requires_grad)
    )
    if not fused:
        return torch.matmul(grad_output, F.dequantize_4bit(B, state).to(grad_output.dtype))
    if state.nested:
        return torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default(
            grad_output, B, state.shape, state.state2.absmax, state.blocksize, state.quant_type,
            absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset,
        )
    return torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default(
        grad_output, B, state.shape, state.absmax, state.blocksize, state.quant_type
    )


class MatMul4Bit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, out=None, bias=None, quant_state: Optional[F.QuantState] = None):
        ctx.is_empty = A.numel() == 0
        if ctx.is_empty:
            ctx.A, ctx.B, ctx.bias = A, B, bias
            w_shape = quant_state.shape
            tail = w_shape[1:] if A.shape[-1] == w_shape[0] else w_shape[:1]
            return torch.empty(A.shape[:-1] + tail, dtype=A.dtype, device=A.device)

        B = B.view(-1, 1)  # canonical packed layout; quant_state.shape carries N and K
        output = _gemm_4bit_from_state(A, B, quant_state, bias)
        if out is not None:
            out.copy_(output)
            output = out

        ctx.state = quant_state
        ctx.dtype_A, ctx.dtype_B = A.dtype, B.dtype
        ctx.dtype_bias = None if bias is None else bias.dtype
        ctx.tensors = (None, B) if any(ctx.needs_input_grad[:2]) else (None, None)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        if ctx.is_empty:
            grad_bias = None if ctx.bias is None else torch.zeros_like(ctx.bias)
            return torch.zeros_like(ctx.A), torch.zeros_like(ctx.B), None, grad_bias, None

        need_A, _, _, need_bias, _ = ctx.needs_input_grad
        _, B = ctx.tensors
        grad_A = grad_bias = None
        if need_bias:
            grad_bias = grad_output.sum(0, dtype=ctx.dtype_bias)
        if need_A:
            # grad_out[M, N] @ dequantize(B)[N, K] = grad_A[M, K]. On the HIP device this is one fused launch for small and
            # medium batches (bitsandbytes_amd::gemm_4bit_grad_input: the weight tile is dequantized into LDS and never
            # written to HBM); the op itself falls back to dequantize + matmul for the rest - the reference's formulation.
            grad_A = _grad_input_from_state(grad_output, B, ctx.state)
        return grad_A, None, None, grad_bias, None


def matmul_4bit(
    A: torch.Tensor,
    B: torch.Tensor,
    quant_state: F.QuantState,
    out: Optional[torch.Tensor] = None,
    bias: Optional[torch.Tensor] = None,
):
    """``A @ dequant(B).T (+ bias)`` with ``B`` the packed 4-bit weight of a ``[N, K]`` matrix
    (reference autograd/_functions.py:407-491)."""
    if quant_state is None:
        raise ValueError("quant_state is required")
    if len(quant_state.shape) != 2:
        raise ValueError("matmul_4bit: quant_state.shape must be 2D [N, K]")

    B = B.view(-1, 1)
    K = A.shape[-1]

    # Legacy: weight quantised from a [K, N] tensor (A's inner dim matches shape[0], not shape[1]).
    if K == quant_state.shape[0] and K != quant_state.shape[1]:
        if not _is_compiling():
            warn(
                f"matmul_4bit: weight was quantized from a [K, N] tensor (quant_state.shape="
                f"{list(quant_state.shape)}). Re-quantize from the weight in [N, K] (out_features, in_features) "
                "orientation. This will be an error in a future version.",
                DeprecationWarning,
                stacklevel=2,
            )
        W = F.dequantize_4bit(B, quant_state).to(A.dtype)
        result = torch.nn.functional.linear(A, W.t(), bias)
        if out is not None:
            out.copy_(result)
            return out
        return result

    needs_grad = torch.is_grad_enabled() and (A.requires_grad or (bias is not None and bias.requires_grad))
    if needs_grad:
        return MatMul4Bit.apply(A, B, out, bias, quant_state)

    if A.numel() == 0:
        if out is not None:
            return out
        return torch.empty((*A.shape[:-1], quant_state.shape[0]), dtype=A.dtype, device=A.device)
    result = _gemm_4bit_from_state(A, B, quant_state, bias)
    if out is not None:
        out.copy_(result)
        return out
    return result


def matmul_4bit_experts(
    x: torch.Tensor,
    packed: torch.Tensor,
    quant_state: F.QuantState,
    expert_ids: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    *,
    row_scale: Optional[torch.Tensor] = None,
    gated: str = "none",
):
    """``y[t, s] = x_row(t, s) @ dequant(packed)[expert_ids[t, s]].T (+ bias[expert_ids[t, s]])`` in one launch - the expert
    projections of a mixture-of-experts decode step. ``packed`` / ``quant_state``: ONE ``quantize_4bit`` over the fused
    ``[E, N, K]`` expert tensor; ``expert_ids``: ``[T, S]`` (or flat ``[P]``) int32 / int64 ON THE DEVICE - their values are read
    by the kernel only, so the call needs no host synchronisation and can be captured in a graph and replayed with other ids in
    the same buffer; an id outside ``[0, E)`` gives a row of zeros. ``x``: ``[T, K]`` (the slots of a token share its
    activations: gate / up) or ``[T, S, K]`` (one row per slot: down). ``bias``: optional ``[E, N]``. Returns ``[T, S, N]``
    (``[P, N]`` for flat ids). Inference only: there is no autograd formula.

    Two epilogues for the projections of a gated-SiLU expert FFN (they exclude each other; :func:`moe_ffn_4bit` is the block):
    ``gated="chunked"`` / ``"interleaved"``: the stack is ``[E, 2 I, K]`` (gate rows ``[0, I)`` and up rows ``[I, 2 I)``, or gate row
    ``2 i`` and up row ``2 i + 1``) and the result ``[T, S, I]`` is ``F.silu(g) * u`` of the plain call's two halves, bit for bit;
    ``row_scale``: ``[T, S]`` (the shape of ``expert_ids``), fp32 or ``x``'s dtype, on the device - ``y[t, s]`` is multiplied by it
    in fp32 in front of the single rounding."""
    if quant_state is None:
        raise ValueError("quant_state is required")
    if len(quant_state.shape) != 3:
        raise ValueError(f"matmul_4bit_experts: quant_state.shape must be 3D [E, N, K], got {list(quant_state.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or (bias is not None and bias.requires_grad)):
        raise RuntimeError("matmul_4bit_experts is inference only (no autograd formula): call it under torch.no_grad() "
                           "or with detached inputs")
    if x.shape[-1] != quant_state.shape[2]:
        raise ValueError(
            f"matmul_4bit_experts: x inner dim ({x.shape[-1]}) must equal quant_state.shape[2] ({quant_state.shape[2]}); "
            "expert tensors in [E, K, N] orientation (contraction over the unpacked dimension) are not supported")
    packed = packed.view(-1, 1)
    if x.device.type == "cuda" and not _is_compiling():
        # (the kernel wants 16-byte aligned activations and weights and the op refuses anything else: a view that starts elsewhere - a
        # slice of a larger buffer - is copied into storage of its own, one launch, instead of ending the caller's step)
        x, packed = _aligned16(x), _aligned16(packed)
    if row_scale is None and gated == "none":
        op, extra = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default, {}
    else:
        if torch.is_grad_enabled() and row_scale is not None and row_scale.requires_grad:
            raise RuntimeError("matmul_4bit_experts is inference only (no autograd formula): call it under torch.no_grad() "
                               "or with detached inputs")
        op, extra = torch.ops.bitsandbytes_amd.gemm_4bit_experts_ffn.default, {"row_scale": row_scale, "gated": gated}
    if not quant_state.nested:
        return op(x, packed, quant_state.shape, quant_state.absmax, expert_ids, quant_state.blocksize, quant_state.quant_type,
                  bias=bias, **extra)
    if quant_state.state2.blocksize != 256:
        raise NotImplementedError("nested quantization with state2.blocksize != 256 is not supported")
    return op(x, packed, quant_state.shape, quant_state.state2.absmax, expert_ids, quant_state.blocksize, quant_state.quant_type,
              bias=bias, absmax_8bit=quant_state.absmax, absmax_code=quant_state.state2.code, absmax_offset=quant_state.offset, **extra)


def moe_ffn_4bit(
    x: torch.Tensor,
    gate_up: torch.Tensor,
    gate_up_state: F.QuantState,
    down: torch.Tensor,
    down_state: F.QuantState,
    expert_ids: torch.Tensor,
    routing_weights: torch.Tensor,
    gate_up_bias: Optional[torch.Tensor] = None,
    down_bias: Optional[torch.Tensor] = None,
    gated: str = "chunked",
):
    """The expert FFN block of a mixture-of-experts decode step, two launches and one slot sum::

        h[t, s] = silu(g) * u,  (g, u) = x[t] @ dequant(gate_up)[expert_ids[t, s]].T (+ gate_up_bias)      [T, S, I]
        y[t]    = sum_s routing_weights[t, s] * (h[t, s] @ dequant(down)[expert_ids[t, s]].T (+ down_bias))  [T, H]

    ``gate_up`` / ``gate_up_state``: one ``quantize_4bit`` over the ``[E, 2 I, H]`` stack, (gate, up) rows ``gated="chunked"`` or
    ``"interleaved"`` (:func:`matmul_4bit_experts`); ``down`` / ``down_state``: the same over ``[E, H, I]``. ``x``: ``[T, H]`` (or
    ``[T, S, H]``); ``expert_ids`` and ``routing_weights``: ``[T, S]`` on the device, the weights fp32 or of ``x``'s dtype. Neither is
    read on the host, so the block can be captured in a graph and replayed with other ids and weights in the same buffers. A slot
    whose id is outside ``[0, E)`` contributes zeros whatever its weight. Inference only."""
    if gated not in ("chunked", "interleaved"):
        raise ValueError(f"moe_ffn_4bit: gated must be 'chunked' or 'interleaved', got {gated!r}")
    if expert_ids.dim() != 2 or tuple(routing_weights.shape) != tuple(expert_ids.shape):
        raise ValueError(f"moe_ffn_4bit: expert_ids and routing_weights must both be [T, S], got {tuple(expert_ids.shape)} and "
                         f"{tuple(routing_weights.shape)}")
    h = matmul_4bit_experts(x, gate_up, gate_up_state, expert_ids, bias=gate_up_bias, gated=gated)
    y = matmul_4bit_experts(h, down, down_state, expert_ids, bias=down_bias, row_scale=routing_weights)
    return y[:, 0] if y.shape[1] == 1 else y.sum(dim=1)


def _gated_fused(x: torch.Tensor, quant_state: F.QuantState) -> bool:
    """Whether the gated launch serves this call - decided from shapes, dtypes and alignment only (nothing is read on the host)."""
    if x.device.type != "cuda" or quant_state.nested or _is_compiling():
        return False
    from ..backends import hip

    N, K = int(quant_state.shape[0]), int(quant_state.shape[1])
    M = x.numel() // K if K else 0
    with torch.cuda.device(x.device):  # (the route depends on the current device's CU count)
        return hip.gemm_4bit_gated_supported(x.dtype, M, N, K, quant_state.blocksize)


def matmul_4bit_gated(x: torch.Tensor, gate_up: torch.Tensor, gate_up_state: F.QuantState, bias: Optional[torch.Tensor] = None):
    """``silu(g) * u`` with ``(g, u) = x @ dequant(gate_up).T (+ bias)`` - the first stage of a dense gated-SiLU FFN (Llama, Mistral,
    Qwen, Phi-3) - as ONE launch: the activation is the matmul's epilogue. ``gate_up`` / ``gate_up_state``: the packed INTERLEAVED
    ``[2 F, K]`` matrix, gate row ``i`` at row ``2 i`` and up row ``i`` at row ``2 i + 1``
    (:func:`bitsandbytes_amd.functional.interleave_gate_up_4bit`), ``bias`` ``[2 F]`` in the same layout. ``x``: ``[*, K]``; returns
    ``[*, F]``.

    The fused launch exists for 1 ... 16 rows of 16-bit activations where the plain call runs the streaming or the streaming MFMA
    kernel (``backends.hip.gemm_4bit_gated_supported``) and plain fp32 absmax. Every other call composes
    ``y = matmul_4bit(x, gate_up, ...)`` with ``F.silu(y[..., 0::2]) * y[..., 1::2]``: the same bits, three or four launches. Neither
    path reads data on the host, so both can be captured in a graph. Inference only: there is no autograd formula."""
    if gate_up_state is None:
        raise ValueError("quant_state is required")
    if len(gate_up_state.shape) != 2 or int(gate_up_state.shape[0]) % 2:
        raise ValueError(f"matmul_4bit_gated: quant_state.shape must be [2 F, K], got {list(gate_up_state.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or (bias is not None and bias.requires_grad)):
        raise RuntimeError("matmul_4bit_gated is inference only (no autograd formula): call it under torch.no_grad() "
                           "or with detached inputs")
    if x.shape[-1] != gate_up_state.shape[1]:
        raise ValueError(f"matmul_4bit_gated: x inner dim ({x.shape[-1]}) must equal quant_state.shape[1] ({gate_up_state.shape[1]})")
    if x.numel() > 0 and (bias is None or bias.dtype == x.dtype) and _gated_fused(x, gate_up_state):
        # (misaligned views are copied: the composition below would run them on another kernel family - not the same bits)
        return torch.ops.bitsandbytes_amd.gemm_4bit_gated.default(_aligned16(x), _aligned16(gate_up).view(-1, 1), gate_up_state.shape,
                                                                  gate_up_state.absmax, gate_up_state.blocksize, gate_up_state.quant_type, bias=bias)
    y = matmul_4bit(x, gate_up, gate_up_state, bias=bias)
    return torch.nn.functional.silu(y[..., 0::2]) * y[..., 1::2]


def ffn_4bit(
    x: torch.Tensor,
    gate_up: torch.Tensor,
    gate_up_state: F.QuantState,
    down: torch.Tensor,
    down_state: F.QuantState,
    gate_up_bias: Optional[torch.Tensor] = None,
    down_bias: Optional[torch.Tensor] = None,
):
    """One dense gated-SiLU FFN block, ``down(silu(gate(x)) * up(x))``, in two launches where the gated launch serves the call
    (:func:`matmul_4bit_gated`; its composition otherwise - the same bits): ``gate_up`` is the interleaved ``[2 F, H]`` matrix,
    ``down`` the ``[H, F]`` one. Bit-identical to the three ``Linear4bit`` layers and torch's ``F.silu(g) * u``. Inference only."""
    if torch.is_grad_enabled() and down_bias is not None and down_bias.requires_grad:
        raise RuntimeError("ffn_4bit is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
    h = matmul_4bit_gated(x, gate_up, gate_up_state, bias=gate_up_bias)
    return matmul_4bit(h, down, down_state, bias=down_bias)


def _lora_fused(x: torch.Tensor, quant_state: F.QuantState, r: int) -> bool:
    """Whether the LoRA launch serves this call - decided from shapes, dtypes and alignment only (nothing is read on the host)."""
    if x.device.type != "cuda" or _is_compiling() or (quant_state.nested and quant_state.state2.blocksize != 256):
        return False
    from ..backends import hip

    N, K = int(quant_state.shape[0]), int(quant_state.shape[1])
    M = x.numel() // K if K else 0
    with torch.cuda.device(x.device):  # (the route depends on the current device's CU count)
        return hip.gemm_4bit_lora_supported(x.dtype, M, N, K, quant_state.blocksize, quant_state.nested, r)


def matmul_4bit_lora(x: torch.Tensor, weight: torch.Tensor, quant_state: F.QuantState, lora_t: torch.Tensor, lora_b: torch.Tensor,
                     scaling: float, bias: Optional[torch.Tensor] = None):
    """``x @ dequant(weight).T (+ bias) + scaling * lora_t @ lora_b.T`` - a 4-bit base layer with its LoRA adapter beside it - as ONE
    launch: the adapter term is the matmul's epilogue. ``lora_t``: ``[*, r] = F.linear(x, lora_A)`` (the caller's small matmul; layers
    that share ``x`` can stack their ``lora_A``), ``lora_b``: ``[N, r]``, PEFT's ``lora_B.weight`` as stored. ``x``: ``[*, K]``; returns
    ``[*, N]``.

    The fused launch exists for 1 ... 16 rows of 16-bit activations where the plain call runs the streaming or the streaming MFMA
    kernel, ``r % 8 == 0`` and ``8 <= r <= 128`` (``backends.hip.gemm_4bit_lora_supported``), plain or nested statistics; its result
    is rounded ONCE: ``T((acc + bias) + scaling * lora)`` with both sums in fp32. Every other call composes
    ``torch.addmm(matmul_4bit(x, ...), lora_t, lora_b.t(), alpha=scaling)`` - two launches, and NOT bit-identical to the fused call: the
    base result is rounded to the tensor's dtype before the adapter term is added (two roundings). Neither path reads data on the
    host, so both can be captured in a graph. Inference only: there is no autograd formula."""
    if quant_state is None:
        raise ValueError("quant_state is required")
    if len(quant_state.shape) != 2:
        raise ValueError(f"matmul_4bit_lora: quant_state.shape must be [N, K], got {list(quant_state.shape)}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, lora_t, lora_b, bias)):
        raise RuntimeError("matmul_4bit_lora is inference only (no autograd formula): call it under torch.no_grad() "
                           "or with detached inputs")
    N, K = int(quant_state.shape[0]), int(quant_state.shape[1])
    if x.shape[-1] != K:
        raise ValueError(f"matmul_4bit_lora: x inner dim ({x.shape[-1]}) must equal quant_state.shape[1] ({K})")
    if lora_b.dim() != 2 or lora_b.shape[0] != N or tuple(lora_t.shape) != (*x.shape[:-1], lora_b.shape[1]):
        raise ValueError(f"matmul_4bit_lora: lora_b must be [N, r] = [{N}, r] and lora_t [*, r] with x's leading dims, "
                         f"got {tuple(lora_b.shape)} and {tuple(lora_t.shape)}")
    r = int(lora_b.shape[1])
    if (x.numel() > 0 and lora_t.dtype == x.dtype and lora_b.dtype == x.dtype
            and (bias is None or bias.dtype == x.dtype) and _lora_fused(x, quant_state, r)):
        # (misaligned views are copied, so that the call keeps the fused launch and its bits)
        xc, tc, bc, weight = _aligned16(x), _aligned16(lora_t), _aligned16(lora_b), _aligned16(weight)
        op = torch.ops.bitsandbytes_amd.gemm_4bit_lora.default
        if not quant_state.nested:
            return op(xc, weight.view(-1, 1), quant_state.shape, quant_state.absmax, quant_state.blocksize, quant_state.quant_type, tc, bc,
                      float(scaling), bias=bias)
        return op(xc, weight.view(-1, 1), quant_state.shape, quant_state.state2.absmax, quant_state.blocksize, quant_state.quant_type, tc, bc,
                  float(scaling), bias=bias, absmax_8bit=quant_state.absmax, absmax_code=quant_state.state2.code,
                  absmax_offset=quant_state.offset)
    y = matmul_4bit(x, weight, quant_state, bias=bias)
    out = torch.addmm(y.reshape(-1, N), lora_t.reshape(-1, r).to(y.dtype), lora_b.to(y.dtype).t(), alpha=float(scaling))
    return out.view(*x.shape[:-1], N)


def lora_shrink(x: torch.Tensor, lora_A: torch.Tensor, splits: Optional[Sequence[int]] = None):
    """``t = x @ lora_A.T`` - the LoRA "shrink" matmul in front of :func:`matmul_4bit_lora` - as ONE hand-written launch. ``x``:
    ``[*, K]``; ``lora_A``: ``[R, K]``, PEFT's ``lora_A.weight`` as stored, or the ``lora_A`` of several layers that share ``x`` (Q/K/V,
    gate/up) concatenated along dim 0 with ``splits = (r_0, r_1, ...)``. Returns ``[*, R]``, or with ``splits`` a tuple of CONTIGUOUS
    ``[*, r_i]`` tensors - views into one buffer, each 16-byte aligned, each ready to be a member's ``lora_t``.

    The kernel serves 1 ... 16 rows of fp16 / bf16 on the device, ``K % 64 == 0``, ``R % 8 == 0``, ``8 <= R <= 1024``, up to 8 splits
    of 8 ... 128 rows, each a multiple of 8 (``backends.hip.lora_shrink_supported``): an fp32 sum in an order that depends on ``K``
    alone, rounded once, so a stacked call's parts are bit-identical to separate calls on the members. Every other call - CPU tensors,
    fp32, more rows, classes the measurements exclude - composes ``F.linear`` and a ``.contiguous()`` per part,
    whose bits are the BLAS library's. Neither path reads data on the host, so both can be captured in a graph. Inference only: there
    is no autograd formula."""
    if lora_A.dim() != 2 or x.dim() < 1 or x.shape[-1] != lora_A.shape[1]:
        raise ValueError(f"lora_shrink: lora_A must be [R, K] and x [*, K], got {tuple(lora_A.shape)} and {tuple(x.shape)}")
    R, K = int(lora_A.shape[0]), int(lora_A.shape[1])
    if splits is not None:
        splits = [int(r) for r in splits]
        if not splits or min(splits) < 1 or sum(splits) != R:
            raise ValueError(f"lora_shrink: splits must be positive and sum to lora_A.shape[0] ({R}), got {splits}")
    if torch.is_grad_enabled() and (x.requires_grad or lora_A.requires_grad):
        raise RuntimeError("lora_shrink is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
    lead = tuple(x.shape[:-1])
    M = x.numel() // K if K else 0
    if x.device.type == "cuda" and lora_A.device == x.device and lora_A.dtype == x.dtype and M > 0 and not _is_compiling():
        from ..backends import hip

        if hip.lora_shrink_supported(x.dtype, M, R, K) and hip.lora_shrink_splits_ok(splits):
            buf = torch.ops.bitsandbytes_amd.lora_shrink.default(_aligned16(x), _aligned16(lora_A), splits)  # (misaligned views: copied)
            if splits is None:
                return buf
            return tuple(p.view(*lead, r) for p, r in zip(buf.split([M * r for r in splits]), splits))
    t = torch.nn.functional.linear(x, lora_A.to(x.dtype))
    if splits is None:
        return t
    return tuple(p.contiguous() for p in t.split(splits, dim=-1))


def matmul_4bit_lora_ids(x: torch.Tensor, weight: torch.Tensor, quant_state: F.QuantState, lora_t: torch.Tensor, lora_B: torch.Tensor,
                         scalings: torch.Tensor, adapter_ids: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """:func:`matmul_4bit_lora` for a mixed-adapter decode batch: row ``m`` of ``x`` (a request) adds
    ``scalings[id] * lora_t[m] @ lora_B[id].T`` with ``id = adapter_ids[m]``. ``lora_B``: ``[A_n, N, r]``, the ``lora_B.weight`` of
    ``A_n`` adapters of one rank (``1 <= A_n <= 64``; pad smaller ranks with zeros), ``scalings``: ``[A_n]``, ``adapter_ids``: ``[*]``
    with ``x``'s leading dims, int32 or int64, ``lora_t``: ``[*, r]`` from :func:`lora_shrink_ids`; all on ``x``'s device. A row whose
    id is outside ``[0, A_n)`` has no adapter: it gets ``matmul_4bit``'s result, and its ``lora_t`` row is not used.

    ONE launch wherever :func:`matmul_4bit_lora`'s fused launch exists (``backends.hip.gemm_4bit_lora_ids_supported``): the ids stay
    on the device, and a row with an adapter has the bits of ``matmul_4bit_lora`` with that adapter at the same batch size. Every
    other call gathers ``lora_B.index_select(0, ids)`` and adds ``scalings[ids] * torch.bmm(...)`` to ``matmul_4bit``'s output with the
    rows without an adapter masked: NOT bit-identical to the fused call (two roundings), inside the same derived bound
    (``tests/lora_cases.py: tolerance``). Neither path reads data on the host, so both can be captured in a graph and follow ids
    written into the same buffer. Inference only: there is no autograd formula."""
    if quant_state is None:
        raise ValueError("quant_state is required")
    if len(quant_state.shape) != 2:
        raise ValueError(f"matmul_4bit_lora_ids: quant_state.shape must be [N, K], got {list(quant_state.shape)}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, lora_t, lora_B, scalings, bias)):
        raise RuntimeError("matmul_4bit_lora_ids is inference only (no autograd formula): call it under torch.no_grad() "
                           "or with detached inputs")
    N, K = int(quant_state.shape[0]), int(quant_state.shape[1])
    if x.shape[-1] != K:
        raise ValueError(f"matmul_4bit_lora_ids: x inner dim ({x.shape[-1]}) must equal quant_state.shape[1] ({K})")
    if lora_B.dim() != 3 or lora_B.shape[1] != N or tuple(lora_t.shape) != (*x.shape[:-1], lora_B.shape[2]):
        raise ValueError(f"matmul_4bit_lora_ids: lora_B must be [A_n, N, r] = [A_n, {N}, r] and lora_t [*, r] with x's leading dims, "
                         f"got {tuple(lora_B.shape)} and {tuple(lora_t.shape)}")
    A_n, r = int(lora_B.shape[0]), int(lora_B.shape[2])
    if not 1 <= A_n <= 64 or tuple(scalings.shape) != (A_n,):
        raise ValueError(f"matmul_4bit_lora_ids: lora_B must stack 1 ... 64 adapters and scalings be [A_n], got {A_n} and {tuple(scalings.shape)}")
    if adapter_ids.dtype not in (torch.int32, torch.int64) or tuple(adapter_ids.shape) != tuple(x.shape[:-1]) or adapter_ids.device != x.device:
        raise ValueError(f"matmul_4bit_lora_ids: adapter_ids must be an int32 / int64 tensor of shape {tuple(x.shape[:-1])} (x's leading dims) "
                         f"on x's device, got {adapter_ids.dtype} {tuple(adapter_ids.shape)} on {adapter_ids.device}")
    if (x.numel() > 0 and lora_t.dtype == x.dtype and lora_B.dtype == x.dtype and scalings.device == x.device
            and (bias is None or bias.dtype == x.dtype) and _lora_fused(x, quant_state, r)):
        # (misaligned views are copied, so that the call keeps the fused launch and its bits)
        xc, tc, bc, weight, ic = _aligned16(x), _aligned16(lora_t), _aligned16(lora_B), _aligned16(weight), adapter_ids.contiguous()
        sc = scalings.to(torch.float32).contiguous()
        op = torch.ops.bitsandbytes_amd.gemm_4bit_lora_ids.default
        if not quant_state.nested:
            return op(xc, weight.view(-1, 1), quant_state.shape, quant_state.absmax, quant_state.blocksize, quant_state.quant_type, tc, bc,
                      sc, ic, bias=bias)
        return op(xc, weight.view(-1, 1), quant_state.shape, quant_state.state2.absmax, quant_state.blocksize, quant_state.quant_type, tc, bc,
                  sc, ic, bias=bias, absmax_8bit=quant_state.absmax, absmax_code=quant_state.state2.code,
                  absmax_offset=quant_state.offset)
    y = matmul_4bit(x, weight, quant_state, bias=bias).reshape(-1, N)
    ids = adapter_ids.reshape(-1).to(torch.int64)
    valid = (ids >= 0) & (ids < A_n)
    safe = torch.where(valid, ids, torch.zeros_like(ids))
    # (the adapter term in fp32, added to the rounded base result and rounded once more: the two roundings of matmul_4bit_lora's composition)
    term = torch.bmm(lora_B.index_select(0, safe).float(), lora_t.reshape(-1, r, 1).float()).view(-1, N)
    out = (y.float() + term * scalings.to(device=y.device, dtype=torch.float32).index_select(0, safe).view(-1, 1)).to(y.dtype)
    return torch.where(valid.view(-1, 1), out, y).view(*x.shape[:-1], N)  # (a select: no NaN from a t row or an adapter the row does not use)


def lora_shrink_ids(x: torch.Tensor, lora_A: torch.Tensor, adapter_ids: torch.Tensor, splits: Optional[Sequence[int]] = None):
    """:func:`lora_shrink` for a mixed-adapter decode batch: row ``m`` of ``x`` (a request) uses adapter ``adapter_ids[m]`` of the
    stack ``lora_A`` ``[A_n, R, K]`` - the ``lora_A.weight`` of ``A_n`` adapters (``1 <= A_n <= 64``), or with ``splits`` the stacked
    ``lora_A`` of several layers that share ``x``, per adapter. ``adapter_ids``: ``[*]`` with ``x``'s leading dims, int32 or int64, on
    ``x``'s device. A row whose id is outside ``[0, A_n)`` has no adapter: its ``t`` is zeros. Returns ``[*, R]``, or with ``splits`` a
    tuple of contiguous ``[*, r_i]`` tensors, as :func:`lora_shrink` does.

    ONE launch where :func:`lora_shrink`'s kernel preconditions hold (``backends.hip.lora_shrink_ids_supported``): the ids are read by
    the kernel only, the workgroups of adapters no row names read nothing, and a row with an adapter has the bits of
    ``lora_shrink(x, lora_A[id])``'s row at the same batch size. Every other call - CPU tensors, fp32, more than 16 rows -
    gathers ``lora_A.index_select(0, ids)`` and composes ``torch.bmm`` with the rows without an adapter masked: the same
    values inside ``lora_shrink``'s tolerance, the bits the BLAS library's. Neither path reads data on the host, so both can be
    captured in a graph and follow ids written into the same buffer. Inference only: there is no autograd formula."""
    if lora_A.dim() != 3 or x.dim() < 1 or x.shape[-1] != lora_A.shape[2]:
        raise ValueError(f"lora_shrink_ids: lora_A must be [A_n, R, K] and x [*, K], got {tuple(lora_A.shape)} and {tuple(x.shape)}")
    A_n, R, K = (int(v) for v in lora_A.shape)
    if adapter_ids.dtype not in (torch.int32, torch.int64) or tuple(adapter_ids.shape) != tuple(x.shape[:-1]) or adapter_ids.device != x.device:
        raise ValueError(f"lora_shrink_ids: adapter_ids must be an int32 / int64 tensor of shape {tuple(x.shape[:-1])} (x's leading dims) on "
                         f"x's device, got {adapter_ids.dtype} {tuple(adapter_ids.shape)} on {adapter_ids.device}")
    if not 1 <= A_n <= 64:
        raise ValueError(f"lora_shrink_ids: lora_A must stack 1 ... 64 adapters, got {A_n}")
    if splits is not None:
        splits = [int(r) for r in splits]
        if not splits or min(splits) < 1 or sum(splits) != R:
            raise ValueError(f"lora_shrink_ids: splits must be positive and sum to lora_A.shape[1] ({R}), got {splits}")
    if torch.is_grad_enabled() and (x.requires_grad or lora_A.requires_grad):
        raise RuntimeError("lora_shrink_ids is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
    lead = tuple(x.shape[:-1])
    M = x.numel() // K if K else 0
    if x.device.type == "cuda" and lora_A.device == x.device and lora_A.dtype == x.dtype and M > 0 and not _is_compiling():
        from ..backends import hip

        if hip.lora_shrink_ids_supported(x.dtype, M, A_n, R, K) and hip.lora_shrink_splits_ok(splits):
            buf = torch.ops.bitsandbytes_amd.lora_shrink_ids.default(_aligned16(x), _aligned16(lora_A), adapter_ids.contiguous(), splits)
            if splits is None:
                return buf
            return tuple(p.view(*lead, r) for p, r in zip(buf.split([M * r for r in splits]), splits))
    ids = adapter_ids.reshape(-1).to(torch.int64)
    valid = (ids >= 0) & (ids < A_n)
    gathered = lora_A.to(x.dtype).index_select(0, torch.where(valid, ids, torch.zeros_like(ids)))  # [M, R, K]
    t = torch.bmm(gathered, x.reshape(-1, K, 1)).view(-1, R)
    t = torch.where(valid.view(-1, 1), t, torch.zeros_like(t)).view(*lead, R)  # (a select: no 0 * NaN from an adapter the row does not use)
    if splits is None:
        return t
    return tuple(p.contiguous() for p in t.split(splits, dim=-1))


def _moe_selection_order(key, dropped=None):
    """The indices of ``key``'s last dimension in the order of the router's selection: larger key first, the lower index on ties, NaN
    keys behind every other key in ascending index, ``dropped`` entries (bool, optional) behind all of those (two stable sorts -
    ``torch.topk`` promises no order among equal keys and puts NaN first)."""
    nan = torch.isnan(key)
    order = torch.sort(torch.where(nan, torch.full_like(key, float("-inf")), key), dim=-1, descending=True, stable=True).indices
    rank = nan.gather(-1, order).to(torch.uint8)
    if dropped is not None:
        rank = torch.where(dropped.gather(-1, order), torch.full_like(rank, 2), rank)
    return order.gather(-1, torch.sort(rank, dim=-1, stable=True).indices)


def _moe_topk_composition(logits, top_k, scoring, renormalize, scale, select_bias, groups=None):
    """:func:`moe_topk` from torch operations, with the kernel's selection rule: fp32 scores, the lower index on ties, NaN keys behind
    every other key in ascending index. ``groups = (n_group, topk_group, group_score)``: the group stage of :func:`moe_topk_grouped`
    in front of the selection - the experts of dropped groups do not take part."""
    p = torch.softmax(logits.float(), dim=-1) if scoring == "softmax" else torch.sigmoid(logits.float())
    key = p if select_bias is None else p + select_bias.to(device=p.device, dtype=torch.float32)
    dropped = None
    if groups is not None:
        n_group, topk_group, group_score = groups
        by_group = key.reshape(*key.shape[:-1], n_group, key.shape[-1] // n_group)
        best = by_group.gather(-1, _moe_selection_order(by_group)[..., :2 if group_score == "top2sum" else 1])
        group_key = best[..., 0] + best[..., 1] if group_score == "top2sum" else best[..., 0]
        kept = _moe_selection_order(group_key)[..., :topk_group]
        dropped = torch.ones_like(group_key, dtype=torch.bool).scatter_(-1, kept, False)
        dropped = dropped.unsqueeze(-1).expand(by_group.shape).reshape(key.shape)
    ids = _moe_selection_order(key, dropped)[..., :top_k]
    w = p.gather(-1, ids)
    if renormalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return ids.to(torch.int32), w * float(scale)


def _moe_topk_grouped_composition(logits, top_k, n_group, topk_group, group_score, scoring, renormalize, scale, select_bias):
    """:func:`moe_topk_grouped` from torch operations, by the kernel's rules (csrc/moe_route.hip); no data is read on the host. Where
    every group stays (``topk_group == n_group``) it is :func:`_moe_topk_composition` itself."""
    groups = (n_group, topk_group, group_score) if topk_group < n_group else None
    return _moe_topk_composition(logits, top_k, scoring, renormalize, scale, select_bias, groups)


def moe_topk(logits: torch.Tensor, top_k: int, scoring: str = "softmax", renormalize: bool = True, scale: float = 1.0,
             select_bias: Optional[torch.Tensor] = None):
    """The scoring and top-k half of a mixture-of-experts router: ``(ids, weights)`` from router ``logits`` ``[*, E]``, as ONE launch.
    ``ids``: ``[*, top_k]`` int32, ``weights``: ``[*, top_k]`` fp32 - what :func:`moe_ffn_4bit` and :func:`matmul_4bit_experts` take as
    ``expert_ids`` and ``routing_weights`` / ``row_scale``, with no conversion in between.

    ``p = softmax(logits)`` (Mixtral, Qwen) or ``sigmoid(logits)`` (DeepSeek-V3, GLM) in fp32; the selection key is ``p``, or
    ``p + select_bias`` (``[E]``, ``e_score_correction_bias``: it takes part in the selection only). Slot 0 holds the best expert; on
    equal keys the lower index goes first; a NaN key goes behind every other key, so the ids of a row are always distinct and in
    ``[0, E)``. ``weights = p[ids]``, divided by their sum if ``renormalize`` (no epsilon: a zero sum gives inf or NaN, as IEEE division
    does), then times ``scale``. A row's result depends on that row alone.

    The launch serves device tensors with ``E <= 1024`` and ``top_k <= 16`` (``backends.hip.moe_topk_supported``). Every other call -
    CPU tensors, more experts or slots, compilation - composes softmax / sigmoid, two stable sorts and a gather: the same ids wherever
    the keys are not within rounding of each other, weights equal to fp32 rounding. Neither path reads data on the host, so both can
    be captured in a graph. Group-limited routing (``n_group`` / ``topk_group``): :func:`moe_topk_grouped`. Inference only."""
    if scoring not in MOE_SCORING_CODES:
        raise ValueError(f"moe_topk: scoring must be 'softmax' or 'sigmoid', got {scoring!r}")
    if logits.dim() < 1 or logits.shape[-1] < 1 or not logits.is_floating_point():
        raise ValueError(f"moe_topk: logits must be a float tensor [*, E] with E >= 1, got {logits.dtype} {tuple(logits.shape)}")
    E, top_k = int(logits.shape[-1]), int(top_k)
    if not 1 <= top_k <= E:
        raise ValueError(f"moe_topk: top_k must be in [1, E] = [1, {E}], got {top_k}")
    if select_bias is not None and tuple(select_bias.shape) != (E,):
        raise ValueError(f"moe_topk: select_bias must be [E] = [{E}], got {tuple(select_bias.shape)}")
    if torch.is_grad_enabled() and (logits.requires_grad or (select_bias is not None and select_bias.requires_grad)):
        raise RuntimeError("moe_topk is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
    rows = logits.numel() // E
    if logits.device.type == "cuda" and rows > 0 and not _is_compiling() and (select_bias is None or select_bias.device == logits.device):
        from ..backends import hip

        if hip.moe_topk_supported(logits.dtype, rows, E, top_k):
            sb = None if select_bias is None else select_bias.to(torch.float32).contiguous()
            return torch.ops.bitsandbytes_amd.moe_topk.default(logits.contiguous(), top_k, scoring, bool(renormalize), float(scale), sb)
    return _moe_topk_composition(logits, top_k, scoring, bool(renormalize), scale, select_bias)


def _moe_router_logits(name, x, router_weight, bias):
    """The argument checks and the logits of :func:`moe_route` / :func:`moe_route_grouped` (``name``: the caller, for the messages)."""
    if router_weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != router_weight.shape[1]:
        raise ValueError(f"{name}: router_weight must be [E, K] and x [*, K], got {tuple(router_weight.shape)} and {tuple(x.shape)}")
    if bias is not None and tuple(bias.shape) != (router_weight.shape[0],):
        raise ValueError(f"{name}: bias must be [E] = [{router_weight.shape[0]}], got {tuple(bias.shape)}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, router_weight, bias)):
        raise RuntimeError(f"{name} is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
    if bias is None and router_weight.dtype == x.dtype:
        return lora_shrink(x, router_weight)
    return torch.nn.functional.linear(x.to(router_weight.dtype), router_weight, None if bias is None else bias.to(router_weight.dtype))


def moe_route(x: torch.Tensor, router_weight: torch.Tensor, top_k: int, *, bias: Optional[torch.Tensor] = None, scoring: str = "softmax",
              renormalize: bool = True, scale: float = 1.0, select_bias: Optional[torch.Tensor] = None, return_logits: bool = False):
    """A whole mixture-of-experts router, ``(ids, weights) = moe_topk(x @ router_weight.T (+ bias), ...)``, in TWO launches where both
    halves are served: the logits come from :func:`lora_shrink` - ``x @ Wr^T`` with ``[E, K]`` weights is exactly its shape class, and
    it falls back to ``F.linear`` by its own measured predicate -, or from ``F.linear`` when the gate has a logit ``bias``; then
    :func:`moe_topk`. ``x``: ``[*, K]``; ``router_weight``: ``[E, K]``, an ``nn.Linear`` gate's weight as stored. Returns ``(ids, weights)``
    ``[*, top_k]``, and the logits ``[*, E]`` behind them with ``return_logits``. With :func:`moe_ffn_4bit` behind it a decode step's
    MoE block is four launches and one slot sum. Inference only.

    Dtypes: the two-launch form needs ``router_weight`` in ``x``'s 16-bit dtype. A gate kept in another dtype (fp32 under bf16
    activations, as several MoE models do) is never rounded: ``x`` - the small operand - is cast to the weight's dtype, one extra
    launch, and ``F.linear`` computes the logits in that dtype. ``select_bias`` should be fp32: another dtype is cast on every call."""
    logits = _moe_router_logits("moe_route", x, router_weight, bias)
    ids, weights = moe_topk(logits, top_k, scoring=scoring, renormalize=renormalize, scale=scale, select_bias=select_bias)
    return (ids, weights, logits) if return_logits else (ids, weights)


def moe_topk_grouped(logits: torch.Tensor, top_k: int, n_group: int, topk_group: int, group_score: str = "top2sum", scoring: str = "sigmoid",
                     renormalize: bool = True, scale: float = 1.0, select_bias: Optional[torch.Tensor] = None):
    """:func:`moe_topk` with group-limited routing - the router of DeepSeek-V2, DeepSeek-V3 / R1 and GLM-4.5 - still as ONE launch.
    Scores, keys (``p``, or ``p + select_bias``), the order of the selection, weights, shapes and dtypes are :func:`moe_topk`'s. In
    addition the ``E`` experts are ``n_group`` contiguous groups of ``G = E / n_group``:

    * a group's score is its first key in the order of the selection (``group_score="max"``: DeepSeek-V2's ``group_limited_greedy``)
      or the sum of its first two keys, one fp32 add (``"top2sum"``: DeepSeek-V3 / GLM's ``noaux_tc``; needs ``G >= 2``);
    * the ``topk_group`` groups that go first in the same order - ties to the lower group, a NaN score last - stay;
    * the ``top_k`` experts are chosen among the experts of those groups only, ``top_k <= topk_group * G``.

    With ``n_group == 1`` or ``topk_group == n_group`` the result has the bits of :func:`moe_topk`. Two deliberate differences from
    the Hugging Face modelling code: an expert of a dropped group NEVER takes part - HF fills its key with ``0.0``, which goes before a
    kept expert whose biased key is negative; DeepSeek's own inference code fills ``-inf``, as here -, and the renormalisation sum has
    no ``1e-20`` added (no epsilon anywhere in this router).

    The launch serves device tensors with ``E <= 1024``, ``n_group <= 64`` and ``top_k <= 16``
    (``backends.hip.moe_topk_grouped_supported``); every other call - CPU tensors, larger sizes, compilation - composes the same rules
    from torch operations with stable sorts. Neither path reads data on the host. Inference only."""
    if scoring not in MOE_SCORING_CODES:
        raise ValueError(f"moe_topk_grouped: scoring must be 'softmax' or 'sigmoid', got {scoring!r}")
    if group_score not in MOE_GROUP_SCORE_CODES:
        raise ValueError(f"moe_topk_grouped: group_score must be 'max' or 'top2sum', got {group_score!r}")
    if logits.dim() < 1 or logits.shape[-1] < 1 or not logits.is_floating_point():
        raise ValueError(f"moe_topk_grouped: logits must be a float tensor [*, E] with E >= 1, got {logits.dtype} {tuple(logits.shape)}")
    E, top_k, n_group, topk_group = int(logits.shape[-1]), int(top_k), int(n_group), int(topk_group)
    if n_group < 1 or E % n_group != 0:
        raise ValueError(f"moe_topk_grouped: n_group must be >= 1 and divide E = {E}, got {n_group}")
    if not 1 <= topk_group <= n_group:
        raise ValueError(f"moe_topk_grouped: topk_group must be in [1, n_group] = [1, {n_group}], got {topk_group}")
    G = E // n_group
    if group_score == "top2sum" and G < 2:
        raise ValueError(f"moe_topk_grouped: group_score 'top2sum' needs groups of at least 2 experts, got E / n_group = {G}")
    if not 1 <= top_k <= topk_group * G:
        raise ValueError(f"moe_topk_grouped: top_k must be in [1, topk_group * E / n_group] = [1, {topk_group * G}], got {top_k}")
    if select_bias is not None and tuple(select_bias.shape) != (E,):
        raise ValueError(f"moe_topk_grouped: select_bias must be [E] = [{E}], got {tuple(select_bias.shape)}")
    if torch.is_grad_enabled() and (logits.requires_grad or (select_bias is not None and select_bias.requires_grad)):
        raise RuntimeError("moe_topk_grouped is inference only (no autograd formula): call it under torch.no_grad() or with detached inputs")
    rows = logits.numel() // E
    if logits.device.type == "cuda" and rows > 0 and not _is_compiling() and (select_bias is None or select_bias.device == logits.device):
        from ..backends import hip

        if hip.moe_topk_grouped_supported(logits.dtype, rows, E, top_k, n_group, topk_group, group_score):
            sb = None if select_bias is None else select_bias.to(torch.float32).contiguous()
            return torch.ops.bitsandbytes_amd.moe_topk_grouped.default(logits.contiguous(), top_k, n_group, topk_group, group_score, scoring,
                                                                       bool(renormalize), float(scale), sb)
    return _moe_topk_grouped_composition(logits, top_k, n_group, topk_group, group_score, scoring, bool(renormalize), scale, select_bias)


def moe_route_grouped(x: torch.Tensor, router_weight: torch.Tensor, top_k: int, n_group: int, topk_group: int, *,
                      group_score: str = "top2sum", bias: Optional[torch.Tensor] = None, scoring: str = "sigmoid", renormalize: bool = True,
                      scale: float = 1.0, select_bias: Optional[torch.Tensor] = None, return_logits: bool = False):
    """:func:`moe_route` with group-limited routing: ``moe_topk_grouped(x @ router_weight.T (+ bias), ...)``, two launches where both
    halves are served. The logits come exactly as in :func:`moe_route` (:func:`lora_shrink`, or ``F.linear`` for a gate with a logit
    ``bias`` or of another dtype than ``x``); the second launch is :func:`moe_topk_grouped`. Returns ``(ids, weights)`` ``[*, top_k]``,
    and the logits behind them with ``return_logits``. Inference only."""
    logits = _moe_router_logits("moe_route_grouped", x, router_weight, bias)
    ids, weights = moe_topk_grouped(logits, top_k, n_group, topk_group, group_score=group_score, scoring=scoring, renormalize=renormalize,
                                    scale=scale, select_bias=select_bias)
    return (ids, weights, logits) if return_logits else (ids, weights)


def matmul_4bit_grouped(A: torch.Tensor, weights, quant_states, biases=None, outs=None):
    """``[matmul_4bit(A, B_i, state_i, bias=bias_i) for i]`` for 4-bit weights that share their input - the Q/K/V
    projections of an attention block, the gate/up projections of an MLP. On MI355X a decode-sized batch (M <= 4) is
    ONE launch of the streaming kernel over the concatenated output rows (``bnb_mi355x_gemm_4bit_grouped``): one
    kernel boundary, one decode-table build and one activation copy per CU instead of one per matrix; 2 ... 16 rows: one launch
    of the streaming MFMA kernel; small groups of 17 ... 64 rows: the same in row passes. Outputs are bit-identical to the separate
    calls up to 16 rows (above: within the fused calls' tolerance); anything the grouped launch does not cover (autograd, mixed statistics
    formats, legacy [K, N] weights, CPU tensors) takes the separate calls.
    ``outs``: optional pre-allocated contiguous result tensors (slices of one communication buffer - the sharded block of
    ``parallel.py`` gathers a whole group with one collective); they are filled and returned.
    New functionality on top of the reference (which issues one gemm_4bit per Linear4bit, nn/modules.py:609-637)."""
    n = len(weights)
    biases = [None] * n if biases is None else list(biases)
    if len(quant_states) != n or len(biases) != n:
        raise ValueError("weights, quant_states and biases must have the same length")

    def separate():
        res = [matmul_4bit(A, w, s, bias=b) for w, s, b in zip(weights, quant_states, biases)]
        if outs is None:
            return res
        for o, r in zip(outs, res):
            o.copy_(r.reshape(o.shape))
        return list(outs)

    if n == 0:
        return []
    s0 = quant_states[0]
    K = A.shape[-1]
    groupable = (
        A.device.type == "cuda" and A.numel() > 0
        and not (torch.is_grad_enabled() and (A.requires_grad or any(b is not None and b.requires_grad for b in biases)))
        and not _is_compiling()
        and all(len(s.shape) == 2 and s.shape[1] == K and s.blocksize == s0.blocksize and s.quant_type == s0.quant_type
                and s.nested == s0.nested and (not s.nested or s.state2.blocksize == 256) for s in quant_states)
    )
    if not groupable:
        return separate()
    from ..backends import hip

    mats = []
    for w, s, b in zip(weights, quant_states, biases):
        if s.nested:
            mats.append((w.view(-1, 1), s.shape, s.state2.absmax, b, s.absmax, s.state2.code, s.offset))
        else:
            mats.append((w.view(-1, 1), s.shape, s.absmax, b, None, None, None))
    return hip.gemm_4bit_grouped(A, mats, s0.blocksize, s0.quant_type, outs=outs)
