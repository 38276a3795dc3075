"""``torch.ops.bitsandbytes.*`` schemas and fake (meta) kernels for the 4-bit path.

The schemas are string-identical to the reference's (``bitsandbytes/_ops.py:162-406``) so that this
package is a drop-in provider of the same operators: if the real ``bitsandbytes`` is already
imported the ops exist and we only add device kernels; otherwise we define them here.

Ops: quantize_4bit, dequantize_4bit(.out), gemm_4bit, gemv_4bit(.out), quantize_blockwise,
dequantize_blockwise(.out).
"""
from __future__ import annotations

from collections.abc import Sequence
from math import prod
from typing import Optional

import torch

_VALID_BLOCKSIZES_4BIT = (32, 64, 128, 256, 512, 1024, 2048, 4096)
_FLOAT_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
_STORAGE_DTYPES = (torch.uint8, torch.bfloat16, torch.float16, torch.float32)

register_fake = torch.library.register_fake
_OVERRIDE_LIB = None


def register_kernel(op: str, device_types: str, func=None):
    """torch.library.register_kernel, except that a kernel somebody else (the reference package's own backends/cuda/ops.py,
    when this package is loaded through the reference's plug-in point on a box where the reference brought a ROCm build)
    registered first for the same dispatch key is REPLACED instead of raising."""

    def deco(fn):
        global _OVERRIDE_LIB
        try:
            torch.library.register_kernel(op, device_types, fn)
        except RuntimeError as exc:
            if "already" not in str(exc):
                raise
            ns, name = op.split("::")
            if _OVERRIDE_LIB is None:
                _OVERRIDE_LIB = {}
            if ns not in _OVERRIDE_LIB:
                _OVERRIDE_LIB[ns] = torch.library.Library(ns, "IMPL")
            key = {"cuda": "CUDA", "cpu": "CPU"}[device_types]
            _OVERRIDE_LIB[ns].impl(name, fn, key, allow_override=True)
        return fn

    return deco(func) if func is not None else deco


def _op_exists(name: str) -> bool:
    ns, op = name.split("::")
    base = op.split(".")[0]
    try:
        packet = getattr(getattr(torch.ops, ns), base)
    except (AttributeError, RuntimeError):
        return False
    overload = op.split(".")[1] if "." in op else "default"
    return overload in packet.overloads()


def _define(name: str, schema: str) -> bool:
    """Define the op unless somebody (the reference package) already did. Returns True if we own it."""
    if _op_exists(name):
        return False
    torch.library.define(name, schema)
    return True


def _check_4bit_common(blocksize: int, quant_type: str) -> None:
    torch._check(blocksize in _VALID_BLOCKSIZES_4BIT, lambda: f"invalid blocksize {blocksize}")
    torch._check(quant_type in ("nf4", "fp4"), lambda: f"quant_type must be 'nf4' or 'fp4', got {quant_type!r}")


# ---------------------------------------------------------------------------------------------- quantize_4bit
if _define(
    "bitsandbytes::quantize_4bit",
    "(Tensor A, int blocksize, str quant_type, ScalarType quant_storage) -> (Tensor, Tensor)",
):

    @register_fake("bitsandbytes::quantize_4bit")
    def _(A: torch.Tensor, blocksize: int, quant_type: str, quant_storage: torch.dtype):
        _check_4bit_common(blocksize, quant_type)
        torch._check(
            A.dtype in _FLOAT_DTYPES,
            lambda: f"Blockwise 4bit quantization only supports 16/32-bit floats, but got {A.dtype}",
        )
        n = A.numel()
        absmax = torch.empty((-(n // -blocksize),), device=A.device, dtype=torch.float32)
        out = torch.empty(((n + 1) // (quant_storage.itemsize * 2), 1), device=A.device, dtype=quant_storage)
        return out, absmax


# ---------------------------------------------------------------------------------------------- dequantize_4bit
def _check_dequant_4bit(absmax, blocksize, quant_type, dtype):
    _check_4bit_common(blocksize, quant_type)
    torch._check(absmax.dtype == torch.float32, lambda: f"absmax must be float32, got {absmax.dtype}")
    torch._check(
        dtype in _FLOAT_DTYPES,
        lambda: f"Blockwise 4bit dequantization only supports 16/32-bit floats, but got {dtype}",
    )


if _define(
    "bitsandbytes::dequantize_4bit",
    "(Tensor A, Tensor absmax, int blocksize, str quant_type, int[] shape, ScalarType dtype) -> Tensor",
):

    @register_fake("bitsandbytes::dequantize_4bit")
    def _(A, absmax, blocksize: int, quant_type: str, shape: Sequence[int], dtype: torch.dtype):
        _check_dequant_4bit(absmax, blocksize, quant_type, dtype)
        return torch.empty(shape, dtype=dtype, device=A.device)


if _define(
    "bitsandbytes::dequantize_4bit.out",
    "(Tensor A, Tensor absmax, int blocksize, str quant_type, int[] shape, ScalarType dtype, Tensor! out) -> ()",
):

    @register_fake("bitsandbytes::dequantize_4bit.out")
    def _(A, absmax, blocksize: int, quant_type: str, shape: Sequence[int], dtype: torch.dtype, out: torch.Tensor):
        _check_dequant_4bit(absmax, blocksize, quant_type, dtype)
        torch._check(out.shape == shape, lambda: f"Expected out.shape == {shape}, got {out.shape}")
        torch._check(out.device == A.device, lambda: f"Expected out.device == {A.device}, got {out.device}")
        torch._check(out.dtype == dtype, lambda: f"Expected out.dtype == {dtype}, got {out.dtype}")


# ---------------------------------------------------------------------------------------------- gemm_4bit
if _define(
    "bitsandbytes::gemm_4bit",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, str quant_type, "
    "Tensor? bias=None, Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor",
):

    @register_fake("bitsandbytes::gemm_4bit")
    def _(
        A: torch.Tensor,
        B: torch.Tensor,
        shapeB: Sequence[int],
        absmax: torch.Tensor,
        blocksize: int,
        quant_type: str,
        bias: Optional[torch.Tensor] = None,
        absmax_8bit: Optional[torch.Tensor] = None,
        absmax_code: Optional[torch.Tensor] = None,
        absmax_offset: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        torch._check(len(shapeB) == 2, lambda: f"shapeB must be 2D [N, K], got {list(shapeB)}")
        torch._check(A.shape[-1] == shapeB[1], lambda: f"A inner dim ({A.shape[-1]}) must match shapeB ({shapeB[1]})")
        torch._check(A.dtype in _FLOAT_DTYPES, lambda: f"A must be float16, bfloat16, or float32, got {A.dtype}")
        torch._check(
            B.dtype in _STORAGE_DTYPES,
            lambda: f"B must be backed by storage of type uint8, bfloat16, float16, or float32, got {B.dtype}",
        )
        _check_4bit_common(blocksize, quant_type)
        torch._check(absmax.dtype == torch.float32, lambda: f"absmax must be float32, got {absmax.dtype}")
        if absmax_8bit is not None:
            torch._check(absmax_8bit.ndim == 1, lambda: f"absmax_8bit must be 1D, got {absmax_8bit.ndim}D")
            torch._check(absmax_8bit.dtype == torch.uint8, lambda: f"absmax_8bit must be uint8, got {absmax_8bit.dtype}")
            torch._check(absmax_code is not None, lambda: "absmax_code required when absmax_8bit is provided")
            torch._check(absmax_code.ndim == 1, lambda: f"absmax_code must be 1D, got {absmax_code.ndim}D")
            torch._check(
                absmax_code.shape[0] == 256, lambda: f"absmax_code must have 256 entries, got {absmax_code.shape[0]}"
            )
            torch._check(
                absmax_code.dtype == torch.float32, lambda: f"absmax_code must be float32, got {absmax_code.dtype}"
            )
            torch._check(absmax_offset is not None, lambda: "absmax_offset required when absmax_8bit is provided")
            torch._check(
                absmax_offset.ndim == 0, lambda: f"absmax_offset must be a scalar (0-dim), got {absmax_offset.ndim}D"
            )
            torch._check(
                absmax_offset.dtype == torch.float32,
                lambda: f"absmax_offset must be float32, got {absmax_offset.dtype}",
            )
        if bias is not None:
            torch._check(bias.ndim == 1, lambda: f"bias must be 1D, got {bias.ndim}D")
            torch._check(
                bias.shape[0] == shapeB[0], lambda: f"bias length ({bias.shape[0]}) must match N ({shapeB[0]})"
            )
            torch._check(bias.dtype == A.dtype, lambda: f"bias dtype ({bias.dtype}) must match A dtype ({A.dtype})")
        return torch.empty((*A.shape[:-1], shapeB[0]), dtype=A.dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- gemv_4bit
def _check_gemv(A, B, blocksize):
    torch._check(blocksize in _VALID_BLOCKSIZES_4BIT, lambda: f"invalid blocksize {blocksize}")
    torch._check(A.dtype in _FLOAT_DTYPES, lambda: f"A must be float16, bfloat16, or float32, got {A.dtype}")
    torch._check(
        B.dtype in _STORAGE_DTYPES,
        lambda: f"B must be backed by storage of type uint8, bfloat16, float16, or float32, got {B.dtype}",
    )


if _define(
    "bitsandbytes::gemv_4bit",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, Tensor code, int blocksize) -> Tensor",
):

    @register_fake("bitsandbytes::gemv_4bit")
    def _(A, B, shapeB: Sequence[int], absmax, code, blocksize: int) -> torch.Tensor:
        _check_gemv(A, B, blocksize)
        return torch.empty((*A.shape[:-1], shapeB[0]), device=A.device, dtype=A.dtype)


if _define(
    "bitsandbytes::gemv_4bit.out",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, Tensor code, int blocksize, Tensor! out) -> ()",
):

    @register_fake("bitsandbytes::gemv_4bit.out")
    def _(A, B, shapeB: Sequence[int], absmax, code, blocksize: int, out: torch.Tensor) -> None:
        _check_gemv(A, B, blocksize)
        expected = (*A.shape[:-1], shapeB[0])
        torch._check(out.shape == expected, lambda: f"Expected out.shape == {expected}, got {out.shape}")
        torch._check(out.device == A.device, lambda: f"Expected out.device == {A.device}, got {out.device}")
        torch._check(out.dtype == A.dtype, lambda: f"Expected out.dtype == {A.dtype}, got {out.dtype}")


# ---------------------------------------------------------------------------------------------- 8-bit blockwise
if _define("bitsandbytes::quantize_blockwise", "(Tensor A, Tensor code, int blocksize) -> (Tensor, Tensor)"):

    @register_fake("bitsandbytes::quantize_blockwise")
    def _(A: torch.Tensor, code: torch.Tensor, blocksize: int):
        torch._check(blocksize > 0, lambda: f"blocksize must be positive, got {blocksize}")
        torch._check(
            A.dtype in _FLOAT_DTYPES, lambda: f"Blockwise quantization only supports 16/32-bit floats, but got {A.dtype}"
        )
        n = A.numel()
        absmax = torch.empty((-(n // -blocksize),), device=A.device, dtype=torch.float32)
        return torch.empty_like(A, dtype=torch.uint8), absmax


def _check_dequant_blockwise(A, blocksize, dtype):
    torch._check(blocksize > 0, lambda: f"blocksize must be positive, got {blocksize}")
    torch._check(A.dtype == torch.uint8, lambda: f"A must be uint8, got {A.dtype}")
    torch._check(
        dtype in _FLOAT_DTYPES, lambda: f"Blockwise dequantization only supports 16/32-bit floats, but got {dtype}"
    )


if _define(
    "bitsandbytes::dequantize_blockwise",
    "(Tensor A, Tensor absmax, Tensor code, int blocksize, ScalarType dtype) -> Tensor",
):

    @register_fake("bitsandbytes::dequantize_blockwise")
    def _(A, absmax, code, blocksize: int, dtype: torch.dtype) -> torch.Tensor:
        _check_dequant_blockwise(A, blocksize, dtype)
        return torch.empty_like(A, dtype=dtype)


if _define(
    "bitsandbytes::dequantize_blockwise.out",
    "(Tensor A, Tensor absmax, Tensor code, int blocksize, ScalarType dtype, Tensor! out) -> ()",
):

    @register_fake("bitsandbytes::dequantize_blockwise.out")
    def _(A, absmax, code, blocksize: int, dtype: torch.dtype, out: torch.Tensor):
        _check_dequant_blockwise(A, blocksize, dtype)
        torch._check(out.shape == A.shape, lambda: f"Expected out.shape == {A.shape}, got {out.shape}")
        torch._check(out.device == A.device, lambda: f"Expected out.device == {A.device}, got {out.device}")
        torch._check(out.dtype == dtype, lambda: f"Expected out.dtype == {dtype}, got {out.dtype}")


__all__ = ["register_kernel", "register_fake", "prod"]


# ---------------------------------------------------------------------------------------------- dequantize_4bit_rows
# Not a reference op: the fused "gather rows, then dequantize" that Embedding4bit needs (the reference
# composes two F.embedding calls and dequantize_4bit, nn/modules.py:921-951). Lives in this package's own
# namespace so it can never collide with an operator the reference defines later.
torch.library.define(
    "bitsandbytes_amd::dequantize_4bit_rows",
    "(Tensor A, Tensor absmax, Tensor indices, int row_len, int blocksize, str quant_type, ScalarType dtype) -> Tensor",
)


@register_fake("bitsandbytes_amd::dequantize_4bit_rows")
def _(A, absmax, indices, row_len: int, blocksize: int, quant_type: str, dtype: torch.dtype):
    _check_4bit_common(blocksize, quant_type)
    torch._check(dtype in _FLOAT_DTYPES, lambda: f"dtype must be a 16/32-bit float, got {dtype}")
    torch._check(indices.dtype in (torch.int32, torch.int64), lambda: f"indices must be int32/int64, got {indices.dtype}")
    torch._check(row_len % blocksize == 0 and row_len % 8 == 0, lambda: "row_len must be a multiple of blocksize and of 8")
    return torch.empty((*indices.shape, row_len), dtype=dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- quantize_4bit_nested
# Not a reference op: quantize_4bit(compress_statistics=True) as one operator - the 4-bit encoder, the mean of its fp32 absmax, the
# subtraction and the 8-bit blockwise encoder (blocksize 256) of the reference's functional.py:925-951, which there are four operator
# calls. Returns (packed, absmax_8bit, absmax2, offset). code8 is the 256-entry code of the second level (the dynamic map).
torch.library.define(
    "bitsandbytes_amd::quantize_4bit_nested",
    "(Tensor A, Tensor code8, int blocksize, str quant_type, ScalarType quant_storage) -> (Tensor, Tensor, Tensor, Tensor)",
)


@register_fake("bitsandbytes_amd::quantize_4bit_nested")
def _(A, code8, blocksize: int, quant_type: str, quant_storage: torch.dtype):
    _check_4bit_common(blocksize, quant_type)
    torch._check(A.dtype in _FLOAT_DTYPES, lambda: f"Blockwise 4bit quantization only supports 16/32-bit floats, but got {A.dtype}")
    torch._check(code8.dtype == torch.float32 and code8.numel() == 256, lambda: "code8 must be 256 float32 values")
    n = A.numel()
    blocks = -(n // -blocksize)
    return (
        torch.empty(((n + 1) // (quant_storage.itemsize * 2), 1), device=A.device, dtype=quant_storage),
        torch.empty((blocks,), device=A.device, dtype=torch.uint8),
        torch.empty((-(blocks // -256),), device=A.device, dtype=torch.float32),
        torch.empty((), device=A.device, dtype=torch.float32),
    )


# ---------------------------------------------------------------------------------------------- dequantize_4bit_nested
# Not a reference op: dequantize_4bit for double-quantised statistics as one operator / one launch (the reference reconstructs the
# fp32 absmax with two more operator calls first, functional.py:1002-1006). absmax2 / code8 / offset are state2.absmax, state2.code
# and state.offset; second-level blocksize 256.
torch.library.define(
    "bitsandbytes_amd::dequantize_4bit_nested",
    "(Tensor A, Tensor absmax_8bit, Tensor absmax2, Tensor code8, Tensor offset, int blocksize, str quant_type, int[] shape, "
    "ScalarType dtype) -> Tensor",
)


@register_fake("bitsandbytes_amd::dequantize_4bit_nested")
def _(A, absmax_8bit, absmax2, code8, offset, blocksize: int, quant_type: str, shape: Sequence[int], dtype: torch.dtype):
    _check_4bit_common(blocksize, quant_type)
    torch._check(dtype in _FLOAT_DTYPES, lambda: f"dtype must be a 16/32-bit float, got {dtype}")
    torch._check(absmax_8bit.dtype == torch.uint8, lambda: f"absmax_8bit must be uint8, got {absmax_8bit.dtype}")
    return torch.empty(tuple(shape), dtype=dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- gemm_4bit_grad_input
# Not a reference op: the fused backward of gemm_4bit with respect to its activations,
#   grad_A[*, K] = grad_out[*, N] @ dequantize_4bit(B)[N, K]
# (the reference dequantizes the whole weight and calls a dense matmul, autograd/_functions.py:365-386). Own namespace,
# like dequantize_4bit_rows. Argument meaning of the weight side as in bitsandbytes::gemm_4bit.
torch.library.define(
    "bitsandbytes_amd::gemm_4bit_grad_input",
    "(Tensor grad_out, Tensor B, int[] shapeB, Tensor absmax, int blocksize, str quant_type, Tensor? absmax_8bit=None, "
    "Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor",
)


@register_fake("bitsandbytes_amd::gemm_4bit_grad_input")
def _(grad_out, B, shapeB: Sequence[int], absmax, blocksize: int, quant_type: str, absmax_8bit=None, absmax_code=None,
      absmax_offset=None):
    _check_4bit_common(blocksize, quant_type)
    torch._check(len(shapeB) == 2, lambda: "shapeB must be [N, K]")
    torch._check(grad_out.shape[-1] == shapeB[0], lambda: f"grad_out inner dim ({grad_out.shape[-1]}) must equal N ({shapeB[0]})")
    return torch.empty((*grad_out.shape[:-1], shapeB[1]), dtype=grad_out.dtype, device=grad_out.device)


# ---------------------------------------------------------------------------------------------- gemm_4bit_experts
# Not a reference op: the expert-indexed fused matmul of a mixture-of-experts decode step,
#   out[t, s, :] = x_row(t, s) @ dequantize_4bit(B)[ids[t, s]].T (+ bias[ids[t, s]])
# B is ONE quantize_4bit result over a contiguous [E, N, K] tensor (shapeB), ids [T, S] (or flat [P]) int32 / int64 on the device and
# read there only (no host synchronisation: the call can be captured in a hipGraph), A [T, K] (the slots of a token share its
# activations) or [T, S, K] (one row per slot). An id outside [0, E) gives a row of zeros. Inference only: no autograd formula.
# Statistics arguments as in bitsandbytes::gemm_4bit; with nested statistics the groups of 256 blocks run over the flat tensor.
torch.library.define(
    "bitsandbytes_amd::gemm_4bit_experts",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, Tensor ids, int blocksize, str quant_type, Tensor? bias=None, "
    "Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor",
)


def _check_gemm_4bit_experts(A, B, shapeB, absmax, ids, blocksize, quant_type, bias, absmax_8bit, absmax_code, absmax_offset):
    """Argument checks shared by the fake kernel and the device kernels; returns (E, N, K, per_slot)."""
    torch._check(is_pow2_blocksize(blocksize), lambda: f"blocksize must be a power of two >= 32, got {blocksize}")
    torch._check(quant_type in ("nf4", "fp4"), lambda: f"quant_type must be 'nf4' or 'fp4', got {quant_type!r}")
    torch._check(len(shapeB) == 3, lambda: f"shapeB must be [E, N, K] (one quantize_4bit over the expert stack), got {list(shapeB)}")
    E, N, K = (int(v) for v in shapeB)
    torch._check(E > 0 and N > 0 and K > 0, lambda: f"shapeB must be positive, got {list(shapeB)}")
    torch._check(A.dtype in _FLOAT_DTYPES, lambda: f"A must be a 16/32-bit float tensor, got {A.dtype}")
    torch._check(ids.dtype in (torch.int32, torch.int64), lambda: f"ids must be int32 or int64, got {ids.dtype}")
    torch._check(ids.dim() in (1, 2), lambda: f"ids must be [T, S] or flat [P], got {ids.dim()} dims")
    torch._check(A.dim() in (2, 3), lambda: f"A must be [T, K] or [T, S, K], got {A.dim()} dims")
    torch._check(
        A.shape[-1] == K,
        lambda: f"A inner dim ({A.shape[-1]}) must equal K = shapeB[2] ({K}); the [E, K, N] orientation (contraction over "
                "the unpacked dimension) is not supported",
    )
    torch._check(K % blocksize == 0, lambda: f"K ({K}) must be a multiple of blocksize ({blocksize})")
    torch._check(A.shape[0] == ids.shape[0], lambda: f"A has {A.shape[0]} tokens, ids {ids.shape[0]}")
    per_slot = A.dim() == 3
    if per_slot:
        torch._check(ids.dim() == 2 and A.shape[1] == ids.shape[1], lambda: "A [T, S, K] needs ids [T, S] with the same S")
    torch._check(ids.device == A.device and B.device == A.device, lambda: "A, B and ids must live on one device")
    torch._check(B.numel() * B.element_size() * 2 == E * N * K, lambda: f"B holds {B.numel() * B.element_size() * 2} 4-bit values, shapeB {E * N * K}")
    torch._check(absmax.dtype == torch.float32, lambda: f"absmax must be float32, got {absmax.dtype}")
    blocks = E * N * K // blocksize
    if absmax_8bit is None:
        torch._check(absmax.numel() == blocks, lambda: f"absmax must hold {blocks} values, got {absmax.numel()}")
    else:
        torch._check(absmax_8bit.dtype == torch.uint8 and absmax_8bit.numel() == blocks, lambda: f"absmax_8bit must hold {blocks} uint8 codes")
        torch._check(absmax.numel() == -(blocks // -256), lambda: f"nested absmax must hold {-(blocks // -256)} values (groups of 256 blocks)")
        torch._check(absmax_code is not None and absmax_code.numel() == 256, lambda: "nested statistics need a 256-entry absmax_code")
        torch._check(absmax_offset is not None and absmax_offset.numel() == 1, lambda: "nested statistics need absmax_offset")
    if bias is not None:
        torch._check(tuple(bias.shape) == (E, N), lambda: f"bias must be [E, N] = [{E}, {N}], got {tuple(bias.shape)}")
        torch._check(bias.dtype == A.dtype, lambda: f"bias dtype ({bias.dtype}) must equal A's ({A.dtype})")
    return E, N, K, per_slot


def is_pow2_blocksize(blocksize: int) -> bool:
    return isinstance(blocksize, int) and blocksize >= 32 and (blocksize & (blocksize - 1)) == 0


@register_fake("bitsandbytes_amd::gemm_4bit_experts")
def _(A, B, shapeB: Sequence[int], absmax, ids, blocksize: int, quant_type: str, bias=None, absmax_8bit=None, absmax_code=None,
      absmax_offset=None):
    _, N, _, _ = _check_gemm_4bit_experts(A, B, shapeB, absmax, ids, blocksize, quant_type, bias, absmax_8bit, absmax_code, absmax_offset)
    return torch.empty((*ids.shape, N), dtype=A.dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- gemm_4bit_experts_ffn
# gemm_4bit_experts with one of two epilogues - the two projections of a gated-SiLU expert FFN:
#   gated = "chunked" / "interleaved": B is [E, 2 I, K] (gate rows [0, I) and up rows [I, 2 I), or gate row 2 i and up row 2 i + 1),
#     out[t, s, :] = silu(g) * u of the plain call's (g, u) - [T, S, I], bit for bit torch's F.silu(g) * u on that output;
#   row_scale [T, S] (fp32 or A's dtype, on the device): out[t, s, :] = (acc + bias) * row_scale[t, s], rounded once.
# The two exclude each other; with neither, the op equals gemm_4bit_experts. An id outside [0, E) gives zeros whatever its scale.
GATED_CODES = {"none": 0, "chunked": 1, "interleaved": 2}

torch.library.define(
    "bitsandbytes_amd::gemm_4bit_experts_ffn",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, Tensor ids, int blocksize, str quant_type, Tensor? bias=None, "
    "Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None, Tensor? row_scale=None, "
    "str gated=\"none\") -> Tensor",
)


def _check_gemm_4bit_experts_ffn(A, B, shapeB, absmax, ids, blocksize, quant_type, bias, absmax_8bit, absmax_code, absmax_offset,
                                 row_scale, gated):
    """The checks of gemm_4bit_experts and those of the two epilogues; returns (E, N, K, per_slot, output width)."""
    E, N, K, per_slot = _check_gemm_4bit_experts(A, B, shapeB, absmax, ids, blocksize, quant_type, bias, absmax_8bit, absmax_code,
                                                 absmax_offset)
    torch._check(gated in GATED_CODES, lambda: f"gated must be one of {sorted(GATED_CODES)}, got {gated!r}")
    if gated != "none":
        torch._check(N % 2 == 0, lambda: f"a gated call needs an even number of weight rows per expert (gate + up), got N = {N}")
        torch._check(row_scale is None, lambda: "gated and row_scale cannot be given together")
    if row_scale is not None:
        torch._check(tuple(row_scale.shape) == tuple(ids.shape),
                     lambda: f"row_scale must have the shape of ids {tuple(ids.shape)}, got {tuple(row_scale.shape)}")
        torch._check(row_scale.dtype in (torch.float32, A.dtype), lambda: f"row_scale must be float32 or {A.dtype}, got {row_scale.dtype}")
        torch._check(row_scale.device == A.device, lambda: "row_scale must live on A's device")
    return E, N, K, per_slot, (N // 2 if gated != "none" else N)


@register_fake("bitsandbytes_amd::gemm_4bit_experts_ffn")
def _(A, B, shapeB: Sequence[int], absmax, ids, blocksize: int, quant_type: str, bias=None, absmax_8bit=None, absmax_code=None,
      absmax_offset=None, row_scale=None, gated: str = "none"):
    width = _check_gemm_4bit_experts_ffn(A, B, shapeB, absmax, ids, blocksize, quant_type, bias, absmax_8bit, absmax_code, absmax_offset,
                                         row_scale, gated)[4]
    return torch.empty((*ids.shape, width), dtype=A.dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- gemm_4bit_gated
# Not a reference op: the gate / up projections of a dense gated-SiLU FFN (Llama, Mistral, Qwen, Phi-3) with the activation as the
# matmul's epilogue. B is the quantize_4bit result of ONE interleaved [2 F, K] matrix - gate row i at row 2 i, up row i at row 2 i + 1
# (functional.interleave_gate_up_4bit builds it from quantized members) -, bias [2 F] in the same layout, absmax fp32 (nested
# statistics un-nested). A [*, K] -> [*, F]:  F.silu(y[..., 0::2]) * y[..., 1::2] of the plain gemm_4bit's output y, bit for bit.
# Served for 1 ... 16 rows where the plain call runs the streaming or the streaming MFMA kernel (backends/hip.py:
# gemm_4bit_gated_supported); anything else raises. Inference only: no autograd formula.
torch.library.define(
    "bitsandbytes_amd::gemm_4bit_gated",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, str quant_type, Tensor? bias=None) -> Tensor",
)


def _check_gemm_4bit_gated(A, B, shapeB, absmax, blocksize, quant_type, bias):
    """Argument checks shared by the fake kernel and the device kernel; returns (N = 2 F, K)."""
    torch._check(is_pow2_blocksize(blocksize), lambda: f"blocksize must be a power of two >= 32, got {blocksize}")
    torch._check(quant_type in ("nf4", "fp4"), lambda: f"quant_type must be 'nf4' or 'fp4', got {quant_type!r}")
    torch._check(len(shapeB) == 2, lambda: f"shapeB must be [2 F, K] (the interleaved gate / up matrix), got {list(shapeB)}")
    N, K = (int(v) for v in shapeB)
    torch._check(N > 0 and K > 0 and N % 2 == 0, lambda: f"shapeB must be [2 F, K] with an even, positive row count, got {list(shapeB)}")
    torch._check(A.dtype in _FLOAT_DTYPES, lambda: f"A must be a 16/32-bit float tensor, got {A.dtype}")
    torch._check(A.dim() >= 1 and A.shape[-1] == K, lambda: f"A inner dim ({A.shape[-1] if A.dim() else None}) must equal K = shapeB[1] ({K})")
    torch._check(B.device == A.device and absmax.device == A.device, lambda: "A, B and absmax must live on one device")
    torch._check(B.numel() * B.element_size() * 2 == N * K, lambda: f"B holds {B.numel() * B.element_size() * 2} 4-bit values, shapeB {N * K}")
    torch._check(absmax.dtype == torch.float32, lambda: f"absmax must be float32, got {absmax.dtype}")
    torch._check(K % blocksize == 0, lambda: f"K ({K}) must be a multiple of blocksize ({blocksize})")
    torch._check(absmax.numel() == N * K // blocksize, lambda: f"absmax must hold {N * K // blocksize} values, got {absmax.numel()}")
    if bias is not None:
        torch._check(tuple(bias.shape) == (N,), lambda: f"bias must be [2 F] = [{N}] (interleaved like the rows), got {tuple(bias.shape)}")
        torch._check(bias.dtype == A.dtype and bias.device == A.device, lambda: f"bias must be a {A.dtype} tensor on A's device")
    return N, K


@register_fake("bitsandbytes_amd::gemm_4bit_gated")
def _(A, B, shapeB: Sequence[int], absmax, blocksize: int, quant_type: str, bias=None):
    N, _ = _check_gemm_4bit_gated(A, B, shapeB, absmax, blocksize, quant_type, bias)
    return torch.empty((*A.shape[:-1], N // 2), dtype=A.dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- gemm_4bit_lora
# Not a reference op: a LoRA adapter beside a 4-bit base layer, y = base(x) + scaling * lora_B(lora_A(x)), with the adapter term as the
# EPILOGUE of the base layer's fused matmul. A [*, K], B / shapeB / absmax / nested statistics / bias as for gemm_4bit; lora_t [*, r] =
# x @ lora_A^T (the caller's small matmul; same leading dims as A, contiguous), lora_b [N, r] = lora_B.weight as stored; both of A's
# dtype. out = T((acc + bias) + scaling * (t @ lora_b^T)): the plain call's fp32 sum, the adapter sum in fp32, ONE rounding to T.
# Served for 1 ... 16 rows where the plain call runs the streaming or the streaming MFMA kernel, r % 8 == 0, 8 <= r <= 128
# (backends/hip.py: gemm_4bit_lora_supported); anything else raises. Inference only: no autograd formula.
torch.library.define(
    "bitsandbytes_amd::gemm_4bit_lora",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, str quant_type, Tensor lora_t, Tensor lora_b, float scaling, "
    "Tensor? bias=None, Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor",
)


def _check_gemm_4bit_lora(A, B, shapeB, absmax, blocksize, quant_type, lora_t, lora_b, bias, absmax_8bit, absmax_code, absmax_offset):
    """Argument checks shared by the fake kernel and the device kernel; returns (N, K, r)."""
    torch._check(is_pow2_blocksize(blocksize), lambda: f"blocksize must be a power of two >= 32, got {blocksize}")
    torch._check(quant_type in ("nf4", "fp4"), lambda: f"quant_type must be 'nf4' or 'fp4', got {quant_type!r}")
    torch._check(len(shapeB) == 2, lambda: f"shapeB must be [N, K], got {list(shapeB)}")
    N, K = (int(v) for v in shapeB)
    torch._check(N > 0 and K > 0, lambda: f"shapeB must be [N, K] with positive sizes, got {list(shapeB)}")
    torch._check(A.dtype in _FLOAT_DTYPES, lambda: f"A must be a 16/32-bit float tensor, got {A.dtype}")
    torch._check(A.dim() >= 1 and A.shape[-1] == K, lambda: f"A inner dim ({A.shape[-1] if A.dim() else None}) must equal K = shapeB[1] ({K})")
    torch._check(B.device == A.device and absmax.device == A.device, lambda: "A, B and absmax must live on one device")
    torch._check(B.numel() * B.element_size() * 2 == N * K, lambda: f"B holds {B.numel() * B.element_size() * 2} 4-bit values, shapeB {N * K}")
    torch._check(absmax.dtype == torch.float32, lambda: f"absmax must be float32, got {absmax.dtype}")
    torch._check(K % blocksize == 0, lambda: f"K ({K}) must be a multiple of blocksize ({blocksize})")
    blocks = N * K // blocksize
    nested = absmax_8bit is not None
    if nested:
        torch._check(absmax_code is not None and absmax_offset is not None, lambda: "nested statistics need absmax_8bit, absmax_code and absmax_offset together")
        torch._check(absmax_8bit.dtype == torch.uint8 and absmax_8bit.numel() == blocks, lambda: f"absmax_8bit must hold {blocks} uint8 codes")
        torch._check(absmax_code.dtype == torch.float32 and absmax_code.numel() == 256, lambda: "absmax_code must hold 256 float32 values")
        torch._check(absmax.numel() == -(blocks // -256), lambda: f"absmax (second level) must hold {-(blocks // -256)} values, got {absmax.numel()}")
        torch._check(absmax_offset.numel() == 1, lambda: "absmax_offset must hold one value")
    else:
        torch._check(absmax_code is None and absmax_offset is None, lambda: "absmax_code / absmax_offset belong to nested statistics (absmax_8bit)")
        torch._check(absmax.numel() == blocks, lambda: f"absmax must hold {blocks} values, got {absmax.numel()}")
    torch._check(lora_b.dim() == 2 and lora_b.shape[0] == N, lambda: f"lora_b must be [N, r] = [{N}, r] (lora_B.weight as stored), got {tuple(lora_b.shape)}")
    r = int(lora_b.shape[1])
    torch._check(r > 0, lambda: "lora_b must be [N, r] with r > 0")
    torch._check(tuple(lora_t.shape) == (*A.shape[:-1], r), lambda: f"lora_t must be [*, r] = {(*A.shape[:-1], r)} (A's leading dims), got {tuple(lora_t.shape)}")
    torch._check(lora_t.dtype == A.dtype and lora_b.dtype == A.dtype, lambda: f"lora_t and lora_b must have A's dtype ({A.dtype}), got {lora_t.dtype} and {lora_b.dtype}")
    torch._check(lora_t.device == A.device and lora_b.device == A.device, lambda: "lora_t and lora_b must live on A's device")
    torch._check(lora_t.is_contiguous() and lora_b.is_contiguous(), lambda: "lora_t and lora_b must be contiguous")
    if bias is not None:
        torch._check(tuple(bias.shape) == (N,), lambda: f"bias must be [N] = [{N}], got {tuple(bias.shape)}")
        torch._check(bias.dtype == A.dtype and bias.device == A.device, lambda: f"bias must be a {A.dtype} tensor on A's device")
    return N, K, r


@register_fake("bitsandbytes_amd::gemm_4bit_lora")
def _(A, B, shapeB: Sequence[int], absmax, blocksize: int, quant_type: str, lora_t, lora_b, scaling: float, bias=None, absmax_8bit=None,
      absmax_code=None, absmax_offset=None):
    N, _, _ = _check_gemm_4bit_lora(A, B, shapeB, absmax, blocksize, quant_type, lora_t, lora_b, bias, absmax_8bit, absmax_code, absmax_offset)
    return torch.empty((*A.shape[:-1], N), dtype=A.dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- lora_shrink
# Not a reference op: the LoRA "shrink" matmul of a decode step, t = x @ lora_a^T, as a kernel of this library - the launch in front of
# gemm_4bit_lora. x [*, K], lora_a [R, K] = lora_A.weight as stored, or several of them concatenated along dim 0 (`splits`: their row
# counts); both 16-bit, contiguous. t[m, j] = T(sum_k x[m, k] * lora_a[j, k]): fp32 sum in an order that depends on K alone, ONE rounding.
# Returns ONE buffer: without splits it is viewed as [*, R]; with splits it is flat, [M * R], and part i is the CONTIGUOUS [M, r_i]
# matrix at element offset M * (r_0 + ... + r_{i-1}) - what gemm_4bit_lora takes as lora_t. Served for 1 ... 16 rows, K % 64 == 0,
# R % 8 == 0, 8 <= R <= 1024, up to 8 splits of 8 ... 128 rows each a multiple of 8 (backends/hip.py: lora_shrink_supported); anything
# else raises. Inference only: no autograd formula.
torch.library.define("bitsandbytes_amd::lora_shrink", "(Tensor x, Tensor lora_a, int[]? splits=None) -> Tensor")

LORA_SHRINK_MAX_SPLITS = 8


def _check_lora_shrink(x, lora_a, splits):
    """Argument checks shared by the fake kernel and the device kernel; returns (M, R, K)."""
    torch._check(lora_a.dim() == 2, lambda: f"lora_a must be [R, K] (lora_A.weight as stored), got {tuple(lora_a.shape)}")
    R, K = int(lora_a.shape[0]), int(lora_a.shape[1])
    torch._check(R > 0 and K > 0, lambda: f"lora_a must be [R, K] with positive sizes, got {tuple(lora_a.shape)}")
    torch._check(x.dtype in _FLOAT_DTYPES, lambda: f"x must be a 16/32-bit float tensor, got {x.dtype}")
    torch._check(x.dim() >= 1 and x.shape[-1] == K, lambda: f"x inner dim ({x.shape[-1] if x.dim() else None}) must equal lora_a.shape[1] ({K})")
    torch._check(lora_a.dtype == x.dtype and lora_a.device == x.device, lambda: f"lora_a must be a {x.dtype} tensor on x's device")
    torch._check(x.is_contiguous() and lora_a.is_contiguous(), lambda: "x and lora_a must be contiguous")
    if splits is not None:
        torch._check(1 <= len(splits) <= LORA_SHRINK_MAX_SPLITS, lambda: f"splits must hold 1 ... {LORA_SHRINK_MAX_SPLITS} row counts, got {len(splits)}")
        torch._check(all(int(r) > 0 for r in splits) and sum(int(r) for r in splits) == R,
                     lambda: f"splits must be positive and sum to R = lora_a.shape[0] ({R}), got {list(splits)}")
    return x.numel() // K, R, K


@register_fake("bitsandbytes_amd::lora_shrink")
def _(x, lora_a, splits: Optional[Sequence[int]] = None):
    M, R, _ = _check_lora_shrink(x, lora_a, splits)
    if splits is None:
        return torch.empty((*x.shape[:-1], R), dtype=x.dtype, device=x.device)
    return torch.empty((M * R,), dtype=x.dtype, device=x.device)


# ---------------------------------------------------------------------------------------------- lora_shrink_ids
# Not a reference op: lora_shrink for a mixed-adapter decode batch - every row of x (a request) names its own adapter. lora_a
# [A_n, R, K] = the lora_A.weight of A_n adapters, stacked (1 <= A_n <= 64); ids [*] with x's leading dims, int32 or int64, on x's device
# and read by the kernel only. t[m] = lora_shrink(x, lora_a[ids[m]])[m], bit for bit, where 0 <= ids[m] < A_n; a row with any other id
# has no adapter and is zeros. `splits` and the returned buffer: as for lora_shrink. Served where lora_shrink's preconditions hold
# (backends/hip.py: lora_shrink_ids_supported); anything else raises. Inference only: no autograd formula.
torch.library.define("bitsandbytes_amd::lora_shrink_ids", "(Tensor x, Tensor lora_a, Tensor ids, int[]? splits=None) -> Tensor")

LORA_MAX_ADAPTERS = 64


def _check_lora_shrink_ids(x, lora_a, ids, splits):
    """Argument checks shared by the fake kernel and the device kernel; returns (M, A_n, R, K)."""
    torch._check(lora_a.dim() == 3, lambda: f"lora_a must be [A_n, R, K] (the adapters' lora_A.weight, stacked), got {tuple(lora_a.shape)}")
    A_n, R, K = (int(v) for v in lora_a.shape)
    torch._check(A_n > 0 and R > 0 and K > 0, lambda: f"lora_a must be [A_n, R, K] with positive sizes, got {tuple(lora_a.shape)}")
    torch._check(A_n <= LORA_MAX_ADAPTERS, lambda: f"lora_a stacks {A_n} adapters, at most {LORA_MAX_ADAPTERS} are served")
    torch._check(x.dtype in _FLOAT_DTYPES, lambda: f"x must be a 16/32-bit float tensor, got {x.dtype}")
    torch._check(x.dim() >= 1 and x.shape[-1] == K, lambda: f"x inner dim ({x.shape[-1] if x.dim() else None}) must equal lora_a.shape[2] ({K})")
    torch._check(lora_a.dtype == x.dtype and lora_a.device == x.device, lambda: f"lora_a must be a {x.dtype} tensor on x's device")
    torch._check(ids.dtype in (torch.int32, torch.int64), lambda: f"ids must be int32 or int64, got {ids.dtype}")
    torch._check(tuple(ids.shape) == tuple(x.shape[:-1]), lambda: f"ids must be [*] = {tuple(x.shape[:-1])} (x's leading dims), got {tuple(ids.shape)}")
    torch._check(ids.device == x.device, lambda: "ids must live on x's device")
    torch._check(x.is_contiguous() and lora_a.is_contiguous() and ids.is_contiguous(), lambda: "x, lora_a and ids must be contiguous")
    if splits is not None:
        torch._check(1 <= len(splits) <= LORA_SHRINK_MAX_SPLITS, lambda: f"splits must hold 1 ... {LORA_SHRINK_MAX_SPLITS} row counts, got {len(splits)}")
        torch._check(all(int(r) > 0 for r in splits) and sum(int(r) for r in splits) == R,
                     lambda: f"splits must be positive and sum to R = lora_a.shape[1] ({R}), got {list(splits)}")
    return x.numel() // K, A_n, R, K


@register_fake("bitsandbytes_amd::lora_shrink_ids")
def _(x, lora_a, ids, splits: Optional[Sequence[int]] = None):
    M, _, R, _ = _check_lora_shrink_ids(x, lora_a, ids, splits)
    if splits is None:
        return torch.empty((*x.shape[:-1], R), dtype=x.dtype, device=x.device)
    return torch.empty((M * R,), dtype=x.dtype, device=x.device)


# ---------------------------------------------------------------------------------------------- gemm_4bit_lora_ids
# Not a reference op: gemm_4bit_lora for a mixed-adapter decode batch. lora_b [A_n, N, r] = the lora_B.weight of A_n adapters of one
# rank, stacked (1 <= A_n <= 64); scalings [A_n] float32; ids [*] with A's leading dims, int32 or int64; all on A's device and read by
# the kernel only. Row m: out = T((acc + bias) + scalings[ids[m]] * (t[m] @ lora_b[ids[m]]^T)), the bits of gemm_4bit_lora with that
# adapter, where 0 <= ids[m] < A_n; a row with any other id has no adapter and gets gemm_4bit's bits (its lora_t row is never read).
# Served exactly where gemm_4bit_lora is (backends/hip.py: gemm_4bit_lora_ids_supported); anything else raises. Inference only.
torch.library.define(
    "bitsandbytes_amd::gemm_4bit_lora_ids",
    "(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, str quant_type, Tensor lora_t, Tensor lora_b, Tensor scalings, Tensor ids, "
    "Tensor? bias=None, Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor",
)


def _check_gemm_4bit_lora_ids(A, B, shapeB, absmax, blocksize, quant_type, lora_t, lora_b, scalings, ids, bias, absmax_8bit, absmax_code, absmax_offset):
    """Argument checks shared by the fake kernel and the device kernel; returns (N, K, r, A_n)."""
    torch._check(lora_b.dim() == 3, lambda: f"lora_b must be [A_n, N, r] (the adapters' lora_B.weight, stacked), got {tuple(lora_b.shape)}")
    A_n = int(lora_b.shape[0])
    torch._check(1 <= A_n <= LORA_MAX_ADAPTERS, lambda: f"lora_b must stack 1 ... {LORA_MAX_ADAPTERS} adapters, got {A_n}")
    torch._check(lora_b.is_contiguous(), lambda: "lora_t and lora_b must be contiguous")
    N, K, r = _check_gemm_4bit_lora(A, B, shapeB, absmax, blocksize, quant_type, lora_t, lora_b[0], bias, absmax_8bit, absmax_code, absmax_offset)
    torch._check(scalings.dtype == torch.float32 and tuple(scalings.shape) == (A_n,) and scalings.device == A.device and scalings.is_contiguous(),
                 lambda: f"scalings must be a contiguous float32 tensor [A_n] = [{A_n}] on A's device, got {scalings.dtype} {tuple(scalings.shape)}")
    torch._check(ids.dtype in (torch.int32, torch.int64), lambda: f"ids must be int32 or int64, got {ids.dtype}")
    torch._check(tuple(ids.shape) == tuple(A.shape[:-1]), lambda: f"ids must be [*] = {tuple(A.shape[:-1])} (A's leading dims), got {tuple(ids.shape)}")
    torch._check(ids.device == A.device and ids.is_contiguous(), lambda: "ids must be contiguous and live on A's device")
    return N, K, r, A_n


@register_fake("bitsandbytes_amd::gemm_4bit_lora_ids")
def _(A, B, shapeB: Sequence[int], absmax, blocksize: int, quant_type: str, lora_t, lora_b, scalings, ids, bias=None, absmax_8bit=None,
      absmax_code=None, absmax_offset=None):
    N, _, _, _ = _check_gemm_4bit_lora_ids(A, B, shapeB, absmax, blocksize, quant_type, lora_t, lora_b, scalings, ids, bias, absmax_8bit, absmax_code,
                                           absmax_offset)
    return torch.empty((*A.shape[:-1], N), dtype=A.dtype, device=A.device)


# ---------------------------------------------------------------------------------------------- moe_topk
# Not a reference op: the scoring and top-k half of a mixture-of-experts router, ONE launch (csrc/moe_route.hip) between the router
# matmul and gemm_4bit_experts / gemm_4bit_experts_ffn. logits [*, E], 16/32-bit float, contiguous; all arithmetic in fp32:
#   p = softmax(logits) or sigmoid(logits) (scoring "softmax" / "sigmoid");  key = p (+ select_bias: fp32 [E], selection only)
#   ids [*, top_k] int32: the experts of largest key, best first, the lower index on ties, NaN keys last - always distinct and in [0, E)
#   weights [*, top_k] fp32: p[ids], divided by their sum in slot order if `renormalize` (no epsilon), then times `scale`
# Served for 1 <= E <= 1024 and 1 <= top_k <= min(E, 16) (backends/hip.py: moe_topk_supported); anything else raises. Nothing is read
# on the host. Inference only: no autograd formula.
torch.library.define("bitsandbytes_amd::moe_topk",
                     "(Tensor logits, int top_k, str scoring, bool renormalize, float scale, Tensor? select_bias=None) -> (Tensor, Tensor)")

MOE_SCORING_CODES = {"softmax": 0, "sigmoid": 1}


def _check_moe_topk(logits, top_k, scoring, select_bias):
    """Argument checks shared by the fake kernel and the device kernel; returns (rows, E)."""
    torch._check(scoring in MOE_SCORING_CODES, lambda: f"scoring must be 'softmax' or 'sigmoid', got {scoring!r}")
    torch._check(logits.dtype in _FLOAT_DTYPES, lambda: f"logits must be a 16/32-bit float tensor, got {logits.dtype}")
    torch._check(logits.dim() >= 1 and logits.shape[-1] >= 1, lambda: f"logits must be [*, E] with E >= 1, got {tuple(logits.shape)}")
    E = int(logits.shape[-1])
    torch._check(1 <= int(top_k) <= E, lambda: f"top_k must be in [1, E] = [1, {E}], got {top_k}")
    torch._check(logits.is_contiguous(), lambda: "logits must be contiguous")
    if select_bias is not None:
        torch._check(select_bias.dtype == torch.float32 and tuple(select_bias.shape) == (E,) and select_bias.device == logits.device
                     and select_bias.is_contiguous(),
                     lambda: f"select_bias must be a contiguous float32 tensor [E] = [{E}] on the logits' device, got {select_bias.dtype} "
                             f"{tuple(select_bias.shape)}")
    return logits.numel() // E, E


@register_fake("bitsandbytes_amd::moe_topk")
def _(logits, top_k: int, scoring: str, renormalize: bool, scale: float, select_bias=None):
    _check_moe_topk(logits, top_k, scoring, select_bias)
    lead = tuple(logits.shape[:-1])
    return (torch.empty((*lead, int(top_k)), dtype=torch.int32, device=logits.device),
            torch.empty((*lead, int(top_k)), dtype=torch.float32, device=logits.device))


# ---------------------------------------------------------------------------------------------- moe_topk_grouped
# Not a reference op: moe_topk with group-limited routing (DeepSeek-V2 / -V3 / R1, GLM-4.5), still ONE launch (csrc/moe_route.hip).
# The experts are n_group contiguous groups of G = E / n_group. A group's score is its first key in the order of the selection
# (group_score "max") or first + second key, one fp32 add ("top2sum", G >= 2); the topk_group groups first in that order on
# (score, group index) stay, and ids / weights are moe_topk's over the experts of those groups only - an expert of a dropped group
# never takes part (it is not a key of 0). n_group == 1 or topk_group == n_group: the bits of moe_topk.
# Served for E % n_group == 0, 1 <= topk_group <= n_group <= 64, E <= 1024 and 1 <= top_k <= min(topk_group * G, 16)
# (backends/hip.py: moe_topk_grouped_supported); anything else raises. Nothing is read on the host. Inference only.
torch.library.define("bitsandbytes_amd::moe_topk_grouped",
                     "(Tensor logits, int top_k, int n_group, int topk_group, str group_score, str scoring, bool renormalize, float scale, "
                     "Tensor? select_bias=None) -> (Tensor, Tensor)")

MOE_GROUP_SCORE_CODES = {"max": 0, "top2sum": 1}


def _check_moe_topk_grouped(logits, top_k, n_group, topk_group, group_score, scoring, select_bias):
    """Argument checks shared by the fake kernel and the device kernel; returns (rows, E)."""
    torch._check(group_score in MOE_GROUP_SCORE_CODES, lambda: f"group_score must be 'max' or 'top2sum', got {group_score!r}")
    rows, E = _check_moe_topk(logits, top_k, scoring, select_bias)
    n_group, topk_group = int(n_group), int(topk_group)
    torch._check(n_group >= 1 and E % n_group == 0, lambda: f"n_group must be >= 1 and divide E = {E}, got {n_group}")
    torch._check(1 <= topk_group <= n_group, lambda: f"topk_group must be in [1, n_group] = [1, {n_group}], got {topk_group}")
    G = E // n_group
    torch._check(G >= 2 or group_score != "top2sum", lambda: f"group_score 'top2sum' needs groups of at least 2 experts, got E / n_group = {G}")
    torch._check(int(top_k) <= topk_group * G,
                 lambda: f"top_k must be at most topk_group * E / n_group = {topk_group * G} (the experts of the kept groups), got {top_k}")
    return rows, E


@register_fake("bitsandbytes_amd::moe_topk_grouped")
def _(logits, top_k: int, n_group: int, topk_group: int, group_score: str, scoring: str, renormalize: bool, scale: float, select_bias=None):
    _check_moe_topk_grouped(logits, top_k, n_group, topk_group, group_score, scoring, select_bias)
    lead = tuple(logits.shape[:-1])
    return (torch.empty((*lead, int(top_k)), dtype=torch.int32, device=logits.device),
            torch.empty((*lead, int(top_k)), dtype=torch.float32, device=logits.device))
