"""Native-library loader for the MI355X backend.

Plays the role of the reference's ``bitsandbytes/cextension.py`` (:348-405) for this path, with one
deliberate difference: there is no CPU library and no deferred-error mock. The product path needs
``libbitsandbytes_mi355x.so`` (built by ``make -C bitsandbytes_amd/csrc`` / ``__graft_entry__.build()``);
if it is missing, ``lib`` is a stub whose every attribute access raises, so any attempt to compute
without the HIP library fails loudly instead of falling back to something else.

ctypes signatures mirror the reference's (``bitsandbytes/backends/cuda/ops.py:16-66``).
"""
from __future__ import annotations

import ctypes as ct
import logging
import os
from pathlib import Path

logger = logging.getLogger(__name__)

PACKAGE_DIR = Path(__file__).resolve().parent
LIB_NAME = "libbitsandbytes_mi355x.so"
LIB_PATH = Path(os.environ.get("BNB_MI355X_LIBRARY", PACKAGE_DIR / LIB_NAME))


class MissingNativeLibrary:
    """Stands in for the library when it cannot be loaded. Import succeeds (so that host-only code —
    QuantState, op schemas, fake kernels — stays usable), any native call raises."""

    def __init__(self, reason: str):
        self._reason = reason

    def __getattr__(self, name):
        raise RuntimeError(
            f"bitsandbytes_amd: native symbol '{name}' requested but {LIB_NAME} is not loaded ({self._reason}). "
            f"Build it with `make -C {PACKAGE_DIR / 'csrc'}` (needs hipcc, targets gfx950). "
            "There is no CPU or PyTorch fallback for the 4-bit kernels in this package."
        )

    def __bool__(self):
        return False


_VOID_P = ct.c_void_p
_I32 = ct.c_int32


class MoeTopkArgs(ct.Structure):
    """``bnb_mi355x_moe_topk_args`` of include/bnb_mi355x.h: the argument block of ``bnb_mi355x_moe_topk``. ``struct_bytes`` is
    ``ctypes.sizeof(MoeTopkArgs)``; the library refuses a block of another size."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("logits_dtype", ct.c_int), ("scoring", ct.c_int), ("renormalize", ct.c_int),
                ("rows", ct.c_int), ("experts", ct.c_int), ("top_k", ct.c_int), ("scale", ct.c_float),
                ("logits", ct.c_void_p), ("select_bias", ct.c_void_p), ("ids", ct.c_void_p), ("weights", ct.c_void_p),
                ("stream", ct.c_void_p)]


class MoeTopkGroupedArgs(ct.Structure):
    """``bnb_mi355x_moe_topk_grouped_args`` of include/bnb_mi355x.h: the argument block of ``bnb_mi355x_moe_topk_grouped``
    (``group_score``: 0 max, 1 top2sum). ``struct_bytes`` is ``ctypes.sizeof(MoeTopkGroupedArgs)``."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("logits_dtype", ct.c_int), ("scoring", ct.c_int), ("renormalize", ct.c_int),
                ("rows", ct.c_int), ("experts", ct.c_int), ("top_k", ct.c_int), ("n_group", ct.c_int), ("topk_group", ct.c_int),
                ("group_score", ct.c_int), ("scale", ct.c_float),
                ("logits", ct.c_void_p), ("select_bias", ct.c_void_p), ("ids", ct.c_void_p), ("weights", ct.c_void_p),
                ("stream", ct.c_void_p)]


class ExpertsCombineArgs(ct.Structure):
    """``bnb_mi355x_gemm_4bit_experts_combine_args`` of include/bnb_mi355x.h; ``struct_bytes`` is ``ctypes.sizeof(ExpertsCombineArgs)``."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("dtype", ct.c_int), ("quant_type", ct.c_int), ("blocksize", ct.c_int),
                ("index_bytes", ct.c_int), ("weights_dtype", ct.c_int), ("S", ct.c_int), ("E", ct.c_int), ("N", ct.c_int), ("K", ct.c_int),
                ("T", ct.c_long), ("h", ct.c_void_p), ("B", ct.c_void_p), ("absmax", ct.c_void_p), ("absmax_8bit", ct.c_void_p),
                ("absmax_code", ct.c_void_p), ("absmax_offset", ct.c_void_p), ("bias", ct.c_void_p), ("ids", ct.c_void_p),
                ("weights", ct.c_void_p), ("out", ct.c_void_p), ("stream", ct.c_void_p)]


class ExpertsGateUpArgs(ct.Structure):
    """``bnb_mi355x_gemm_4bit_experts_gate_up_args`` of include/bnb_mi355x.h; ``struct_bytes`` is ``ctypes.sizeof(ExpertsGateUpArgs)``."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("dtype", ct.c_int), ("quant_type", ct.c_int), ("blocksize", ct.c_int),
                ("index_bytes", ct.c_int), ("gated", ct.c_int), ("S", ct.c_int), ("E", ct.c_int), ("N", ct.c_int), ("K", ct.c_int),
                ("T", ct.c_long), ("x", ct.c_void_p), ("B", ct.c_void_p), ("absmax", ct.c_void_p), ("absmax_8bit", ct.c_void_p),
                ("absmax_code", ct.c_void_p), ("absmax_offset", ct.c_void_p), ("bias", ct.c_void_p), ("ids", ct.c_void_p),
                ("out", ct.c_void_p), ("stream", ct.c_void_p)]


class ExpertsMfmaArgs(ct.Structure):
    """``bnb_mi355x_gemm_4bit_experts_mfma_args`` of include/bnb_mi355x.h; ``struct_bytes`` is ``ctypes.sizeof(ExpertsMfmaArgs)``."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("dtype", ct.c_int), ("quant_type", ct.c_int), ("blocksize", ct.c_int),
                ("index_bytes", ct.c_int), ("gated", ct.c_int), ("row_scale_dtype", ct.c_int), ("S", ct.c_int), ("E", ct.c_int),
                ("N", ct.c_int), ("K", ct.c_int), ("P", ct.c_long), ("a_slot_stride", ct.c_long), ("A", ct.c_void_p), ("B", ct.c_void_p),
                ("absmax", ct.c_void_p), ("absmax_8bit", ct.c_void_p), ("absmax_code", ct.c_void_p), ("absmax_offset", ct.c_void_p),
                ("bias", ct.c_void_p), ("ids", ct.c_void_p), ("row_scale", ct.c_void_p), ("out", ct.c_void_p), ("stream", ct.c_void_p)]


class GemmInt8Args(ct.Structure):
    """``bnb_mi355x_gemm_int8_args`` of include/bnb_mi355x.h; ``struct_bytes`` is ``ctypes.sizeof(GemmInt8Args)``."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("epilogue", ct.c_int), ("out_dtype", ct.c_int), ("bias_dtype", ct.c_int),
                ("M", ct.c_long), ("N", ct.c_long), ("K", ct.c_long), ("A", ct.c_void_p), ("B", ct.c_void_p), ("row_stats", ct.c_void_p),
                ("col_stats", ct.c_void_p), ("bias", ct.c_void_p), ("out", ct.c_void_p), ("stream", ct.c_void_p)]


class Int8QuantArgs(ct.Structure):
    """``bnb_mi355x_int8_vectorwise_quant_args`` of include/bnb_mi355x.h."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("dtype", ct.c_int), ("threshold", ct.c_float), ("rows", ct.c_long), ("cols", ct.c_long),
                ("A", ct.c_void_p), ("q", ct.c_void_p), ("row_stats", ct.c_void_p), ("stream", ct.c_void_p)]


class Int8QuantMaskArgs(ct.Structure):
    """``bnb_mi355x_int8_vectorwise_quant_mask_args`` of include/bnb_mi355x.h."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("dtype", ct.c_int), ("threshold", ct.c_float), ("rows", ct.c_long), ("cols", ct.c_long),
                ("A", ct.c_void_p), ("q", ct.c_void_p), ("row_stats", ct.c_void_p), ("mask", ct.c_void_p), ("stream", ct.c_void_p)]


class Int8OutlierAddmmArgs(ct.Structure):
    """``bnb_mi355x_int8_outlier_addmm_args`` of include/bnb_mi355x.h."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("dtype", ct.c_int), ("M", ct.c_long), ("N", ct.c_long), ("K", ct.c_long), ("A", ct.c_void_p),
                ("CB", ct.c_void_p), ("SCB", ct.c_void_p), ("mask", ct.c_void_p), ("out", ct.c_void_p), ("stream", ct.c_void_p)]


class Int8MmDequantArgs(ct.Structure):
    """``bnb_mi355x_int8_mm_dequant_args`` of include/bnb_mi355x.h."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("out_dtype", ct.c_int), ("bias_dtype", ct.c_int), ("M", ct.c_long), ("N", ct.c_long),
                ("C", ct.c_void_p), ("row_stats", ct.c_void_p), ("col_stats", ct.c_void_p), ("bias", ct.c_void_p), ("out", ct.c_void_p),
                ("stream", ct.c_void_p)]


INT8_OK, INT8_MALFORMED, INT8_REFUSED_K = 0, 1, 2  # BNB_MI355X_INT8_* of include/bnb_mi355x.h


class OptimizerUpdateArgs(ct.Structure):
    """``bnb_mi355x_optimizer_update_args`` of include/bnb_mi355x.h (both optimizer entry points take it)."""

    _fields_ = [("struct_bytes", ct.c_size_t), ("optimizer", ct.c_int), ("dtype", ct.c_int), ("n", ct.c_long), ("g", ct.c_void_p),
                ("p", ct.c_void_p), ("state1", ct.c_void_p), ("state2", ct.c_void_p), ("qmap1", ct.c_void_p), ("qmap2", ct.c_void_p),
                ("absmax1", ct.c_void_p), ("absmax2", ct.c_void_p), ("step", ct.c_int), ("gnorm_scale", ct.c_float), ("beta1", ct.c_float),
                ("one_minus_beta1", ct.c_float), ("beta2", ct.c_float), ("one_minus_beta2", ct.c_float), ("sqrt_correction2", ct.c_float),
                ("eps", ct.c_float), ("weight_decay", ct.c_float), ("decay", ct.c_float), ("step_scale", ct.c_float), ("neg_lr", ct.c_float),
                ("stream", ct.c_void_p)]


OPTIMIZER_CODES = {"adam": 0, "momentum": 1, "rmsprop": 2, "adagrad": 3, "lion": 4}  # BNB_MI355X_OPT_* of include/bnb_mi355x.h


def _declare(dll: ct.CDLL) -> None:
    def sig(names, argtypes, restype=None):
        for n in names:
            fn = getattr(dll, n)
            fn.argtypes = argtypes
            fn.restype = restype

    dts = ("fp32", "bf16", "fp16")
    qts = ("nf4", "fp4")
    # (code, A, absmax, out, blocksize, n)
    sig([f"cquantize_blockwise_{d}_{q}" for d in dts for q in qts] + [f"cquantize_blockwise_{d}" for d in dts],
        [_VOID_P] * 4 + [_I32, _I32])
    # (code, A, absmax, out, blocksize, n, stream)
    sig([f"cdequantize_blockwise_{d}_{q}" for d in dts for q in qts] + [f"cdequantize_blockwise_{d}" for d in dts],
        [_VOID_P] * 4 + [_I32, _I32, _VOID_P])
    # (A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, M, N, K, blocksize, quant_type, stream)
    sig([f"cgemm_4bit_{d}" for d in dts], [_VOID_P] * 8 + [_I32] * 5 + [_VOID_P])
    # (m, n, k, A, B, absmax, code, out, lda, ldb, ldc, blocksize, stream)
    sig([f"cgemm_4bit_inference_naive_{d}" for d in dts], [_I32] * 3 + [_VOID_P] * 5 + [_I32] * 4 + [_VOID_P])
    sig(["get_context"], [], _VOID_P)
    sig(["cget_managed_ptr"], [ct.c_size_t], _VOID_P)
    # extensions
    sig(["bnb_mi355x_quantize_4bit"], [_VOID_P, _I32, _VOID_P, _VOID_P, _I32, ct.c_long, _I32, _VOID_P])
    sig(["bnb_mi355x_quantize_8bit"], [_VOID_P, _VOID_P, _I32, _VOID_P, _VOID_P, _I32, ct.c_long, _VOID_P])
    sig(["bnb_mi355x_quantize_4bit_nested"], [_VOID_P, _I32, ct.c_long, _I32, _I32] + [_VOID_P] * 7)
    sig(["bnb_mi355x_dequantize_4bit_nested"], [_I32] + [_VOID_P] * 6 + [_I32, ct.c_long, _I32, _VOID_P])
    sig(["bnb_mi355x_dequantize_4bit_rows"],
        [_I32, _VOID_P, _VOID_P, _VOID_P, _I32, _VOID_P, ct.c_long, ct.c_long, _I32, _I32, _I32, _VOID_P])
    sig(["bnb_mi355x_gemm_4bit"], [_I32, _I32] + [_VOID_P] * 9 + [_I32] * 5 + [_VOID_P, ct.c_size_t, _VOID_P])
    sig(["bnb_mi355x_gemm_4bit_workspace_bytes"], [_I32] * 6, ct.c_size_t)
    sig(["bnb_mi355x_gemm_4bit_route"], [_I32] * 6, _I32)
    sig(["bnb_mi355x_gemm_4bit_fused_max_m"], [_I32] * 5, _I32)  # (dtype, N, K, blocksize, nested)
    sig(["bnb_mi355x_last_gemm_kernel"], [], _I32)
    # (dtype, A, a_slot_stride, B, absmax, absmax_8bit, absmax_code, absmax_offset, bias, ids, index_bytes, out, P, S, E, N, K, blocksize,
    #  quant_type, stream)
    sig(["bnb_mi355x_gemm_4bit_experts"],
        [_I32, _VOID_P, ct.c_long] + [_VOID_P] * 7 + [_I32, _VOID_P, ct.c_long] + [_I32] * 6 + [_VOID_P])
    sig(["bnb_mi355x_gemm_4bit_experts_supported"], [_I32] * 5, _I32)
    # (dtype, A, a_slot_stride, B, absmax, absmax_8bit, absmax_code, absmax_offset, bias, ids, index_bytes, row_scale, row_scale_dtype,
    #  gated, out, P, S, E, N, K, blocksize, quant_type, stream)
    sig(["bnb_mi355x_gemm_4bit_experts_ffn"],
        [_I32, _VOID_P, ct.c_long] + [_VOID_P] * 7 + [_I32, _VOID_P, _I32, _I32, _VOID_P, ct.c_long] + [_I32] * 6 + [_VOID_P])
    sig(["bnb_mi355x_gemm_4bit_experts_ffn_supported"], [_I32] * 6, _I32)
    # (one argument block, passed with ctypes.byref(ExpertsCombineArgs(...)); non-zero: refused, nothing launched)
    sig(["bnb_mi355x_gemm_4bit_experts_combine"], [_VOID_P], _I32)
    sig(["bnb_mi355x_gemm_4bit_experts_combine_supported"], [_I32] * 6, _I32)  # (dtype, E, N, K, blocksize, S)
    sig(["bnb_mi355x_gemm_4bit_experts_combine_plan"], [ct.c_long, _I32, _I32, _I32, _VOID_P], _I32)  # (T, S, N, K, out4: int32[4] on the host)
    # (one argument block, passed with ctypes.byref(ExpertsGateUpArgs(...)); non-zero: refused, nothing launched)
    sig(["bnb_mi355x_gemm_4bit_experts_gate_up"], [_VOID_P], _I32)
    sig(["bnb_mi355x_gemm_4bit_experts_gate_up_supported"], [_I32] * 7, _I32)  # (dtype, E, N = 2 I, K, blocksize, S, gated)
    sig(["bnb_mi355x_gemm_4bit_experts_gate_up_plan"], [ct.c_long, _I32, _I32, _I32, _VOID_P], _I32)  # (T, S, N, K, out4: int32[4] on the host)
    # (one argument block, passed with ctypes.byref(ExpertsMfmaArgs(...)); non-zero: refused, nothing launched)
    sig(["bnb_mi355x_gemm_4bit_experts_mfma"], [_VOID_P], _I32)
    sig(["bnb_mi355x_gemm_4bit_experts_mfma_supported"], [_I32] * 6, _I32)  # (dtype, E, N, K, blocksize, gated)
    # LLM.int8(): one argument block each (ctypes.byref(Int8QuantArgs / GemmInt8Args / Int8MmDequantArgs)); non-zero: nothing launched
    # (bnb_mi355x_gemm_int8: INT8_REFUSED_K = take the fallback)
    sig(["bnb_mi355x_int8_vectorwise_quant", "bnb_mi355x_gemm_int8", "bnb_mi355x_int8_mm_dequant"], [_VOID_P], _I32)
    # the sync-free mixed decomposition: Int8QuantMaskArgs / Int8OutlierAddmmArgs (the second answers INT8_REFUSED_K like the matmul)
    sig(["bnb_mi355x_int8_vectorwise_quant_mask", "bnb_mi355x_int8_outlier_addmm"], [_VOID_P], _I32)
    sig(["bnb_mi355x_gemm_int8_route"], [ct.c_long] * 3, _I32)  # (M, N, K): 13 / 14, 0 for a refused K (host logic)
    # the fused optimizer updates: one argument block (ctypes.byref(OptimizerUpdateArgs)); non-zero: nothing launched
    sig(["bnb_mi355x_optimizer_update_8bit_blockwise", "bnb_mi355x_optimizer_update_32bit"], [_VOID_P], _I32)
    sig(["bnb_mi355x_optimizer_update_grid"], [ct.c_long], _I32)  # workgroups of that launch for n elements (host logic)
    # (dtype, A, B, absmax, out, bias, M, N = 2 F, K, blocksize, quant_type, stream)
    sig(["bnb_mi355x_gemm_4bit_gated"], [_I32] + [_VOID_P] * 5 + [_I32] * 5 + [_VOID_P])
    sig(["bnb_mi355x_gemm_4bit_gated_supported"], [_I32] * 5, _I32)
    # (dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, lora_t, lora_b, scaling, r, M, N, K, blocksize, quant_type, stream)
    sig(["bnb_mi355x_gemm_4bit_lora"], [_I32] + [_VOID_P] * 10 + [ct.c_float] + [_I32] * 6 + [_VOID_P])
    sig(["bnb_mi355x_gemm_4bit_lora_supported"], [_I32] * 7, _I32)  # (dtype, M, N, K, blocksize, nested, r)
    # (dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, lora_t, lora_b, scalings, ids, index_bytes, A_n, r, M, N, K,
    #  blocksize, quant_type, stream)
    sig(["bnb_mi355x_gemm_4bit_lora_ids"], [_I32] + [_VOID_P] * 12 + [_I32] * 8 + [_VOID_P])
    sig(["bnb_mi355x_gemm_4bit_lora_ids_supported"], [_I32] * 8, _I32)  # (dtype, M, N, K, blocksize, nested, r, A_n)
    # (dtype, x, lora_a, t, M, R, K, splits (host int[n_splits] or NULL), n_splits, stream)
    sig(["bnb_mi355x_lora_shrink"], [_I32] + [_VOID_P] * 3 + [_I32] * 3 + [_VOID_P, _I32, _VOID_P])
    sig(["bnb_mi355x_lora_shrink_supported"], [_I32] * 4, _I32)  # (dtype, M, R, K)
    # (dtype, x, lora_a, ids, index_bytes, t, M, A_n, R, K, splits (host int[n_splits] or NULL), n_splits, stream)
    sig(["bnb_mi355x_lora_shrink_ids"], [_I32] + [_VOID_P] * 3 + [_I32, _VOID_P] + [_I32] * 4 + [_VOID_P, _I32, _VOID_P])
    sig(["bnb_mi355x_lora_shrink_ids_supported"], [_I32] * 5, _I32)  # (dtype, M, A_n, R, K)
    # (one argument block, passed with ctypes.byref(MoeTopkArgs(...)); non-zero: refused, nothing launched)
    sig(["bnb_mi355x_moe_topk"], [_VOID_P], _I32)
    sig(["bnb_mi355x_moe_topk_supported"], [_I32] * 4, _I32)  # (logits_dtype, rows, experts, top_k)
    sig(["bnb_mi355x_moe_topk_grouped"], [_VOID_P], _I32)  # (ctypes.byref(MoeTopkGroupedArgs(...)))
    # (logits_dtype, rows, experts, top_k, n_group, topk_group, group_score)
    sig(["bnb_mi355x_moe_topk_grouped_supported"], [_I32] * 7, _I32)
    # (dtype, A, count, B[], absmax[], absmax_8bit[], absmax_code[], absmax_offset[], out[], bias[], N[], M, K, blocksize, quant_type, stream)
    sig(["bnb_mi355x_gemm_4bit_grouped"], [_I32, _VOID_P, _I32] + [_VOID_P] * 8 + [_I32] * 4 + [_VOID_P])
    sig(["bnb_mi355x_gemm_4bit_grouped_route"], [_I32, _I32, _VOID_P, _I32, _I32, _I32], _I32)  # (dtype, count, N[], M, K, blocksize)
    # (dtype, grad_out, B, absmax, absmax_8bit, absmax_code, absmax_offset, grad_A, M, N, K, blocksize, quant_type, ws, ws_bytes, stream)
    sig(["bnb_mi355x_gemm_4bit_grad_input"], [_I32] + [_VOID_P] * 7 + [_I32] * 5 + [_VOID_P, ct.c_size_t, _VOID_P])
    sig(["bnb_mi355x_gemm_4bit_grad_input_workspace_bytes"], [_I32] * 3, ct.c_size_t)
    sig(["bnb_mi355x_gemm_4bit_grad_input_supported"], [_I32] * 5, _I32)
    sig(["bnb_mi355x_peer_buffer_bytes"], [_I32, ct.c_size_t], ct.c_size_t)
    sig(["bnb_mi355x_peer_alloc"], [ct.c_size_t], _VOID_P)
    sig(["bnb_mi355x_peer_free", "bnb_mi355x_peer_close"], [_VOID_P])
    sig(["bnb_mi355x_peer_export"], [_VOID_P, _VOID_P], _I32)
    sig(["bnb_mi355x_peer_open"], [_VOID_P], _VOID_P)
    # (bufs[], world, rank, src, out, bytes, max_bytes, stream)
    sig(["bnb_mi355x_peer_allgather"], [_VOID_P, _I32, _I32, _VOID_P, _VOID_P, ct.c_size_t, ct.c_size_t, _VOID_P])
    sig(["bnb_mi355x_peer_status"], [_VOID_P], _I32)
    sig(["bnb_mi355x_peer_chain_buffer_bytes"], [ct.c_long], ct.c_size_t)
    sig(["bnb_mi355x_peer_chain_alloc"], [ct.c_size_t, _I32], _VOID_P)
    # (world, ns, K, blocksize, mode, max_values, wg_limit)
    sig(["bnb_mi355x_gemv_4bit_peer_serves"], [_I32] * 5 + [ct.c_long, _I32], _I32)
    # (bufs[], epoch_word, world, rank, dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, bias, out_local, ns, K, blocksize,
    #  quant_type, mode, max_values, wg_limit, epoch_offset, stream)
    sig(["bnb_mi355x_gemv_4bit_peer"], [_VOID_P, _VOID_P, _I32, _I32, _I32] + [_VOID_P] * 8 + [_I32] * 5 + [ct.c_long, _I32, _I32, _VOID_P], _I32)
    # (bufs[], epoch_word, world, rank, dtype, out, nvalues, max_values, epoch_offset, stream)
    sig(["bnb_mi355x_peer_chain_read"], [_VOID_P, _VOID_P, _I32, _I32, _I32, _VOID_P, _I32, ct.c_long, _I32, _VOID_P])
    sig(["bnb_mi355x_set_stream_tuning"], [_I32] * 5)
    sig(["bnb_mi355x_gemv_4bit_stream_exact"], [_I32] * 6, _I32)
    # (form, dtype, M, rows, K, blocksize, out8: int32[8] on the host)
    sig(["bnb_mi355x_stream_geometry"], [_I32] * 3 + [ct.c_long, _I32, _I32, _VOID_P], _I32)
    sig(["bnb_mi355x_set_tuning"], [_I32] * 4)
    sig(["bnb_mi355x_set_cu_count"], [_I32])
    # (kernel, dtype, M, N, K, blocksize, nested, out16: int32[16] on the host)
    sig(["bnb_mi355x_gemm_4bit_plan"], [_I32] * 7 + [_VOID_P], _I32)
    # (form, dtype, M, N, group_N: int32[N] on the host or NULL, K, blocksize, nested, out16)
    sig(["bnb_mi355x_gemm_4bit_sm_form_plan"], [_I32] * 4 + [_VOID_P] + [_I32] * 3 + [_VOID_P], _I32)
    sig(["bnb_mi355x_gemm_4bit_grad_input_plan"], [_I32] * 5 + [_VOID_P], _I32)  # (dtype, M, N, K, blocksize, out16)
    sig(["bnb_mi355x_set_stamp_buffer"], [_VOID_P])
    sig(["bnb_mi355x_version"], [], ct.c_char_p)


def load_native_library():
    if not LIB_PATH.exists():
        return MissingNativeLibrary(f"{LIB_PATH} does not exist")
    try:
        dll = ct.CDLL(str(LIB_PATH))
        _declare(dll)
    except (OSError, AttributeError) as exc:  # missing libamdhip64, missing symbol, ...
        logger.error("bitsandbytes_amd: failed to load %s: %s", LIB_PATH, exc)
        return MissingNativeLibrary(str(exc))
    return dll


lib = load_native_library()

# every symbol include/bnb_mi355x.h declares; tests check that the loaded library exports all of them
EXPORTED_SYMBOLS = tuple(
    [f"cquantize_blockwise_{d}_{q}" for d in ("fp32", "bf16", "fp16") for q in ("nf4", "fp4")]
    + [f"cdequantize_blockwise_{d}_{q}" for d in ("fp32", "bf16", "fp16") for q in ("nf4", "fp4")]
    + [f"cquantize_blockwise_{d}" for d in ("fp32", "bf16", "fp16")]
    + [f"cdequantize_blockwise_{d}" for d in ("fp32", "bf16", "fp16")]
    + [f"cgemm_4bit_{d}" for d in ("fp32", "bf16", "fp16")]
    + [f"cgemm_4bit_inference_naive_{d}" for d in ("fp32", "bf16", "fp16")]
    + ["get_context", "cget_managed_ptr", "bnb_mi355x_quantize_4bit", "bnb_mi355x_quantize_8bit", "bnb_mi355x_quantize_4bit_nested", "bnb_mi355x_dequantize_4bit_nested", "bnb_mi355x_dequantize_4bit_rows",
       "bnb_mi355x_gemm_4bit", "bnb_mi355x_gemm_4bit_workspace_bytes", "bnb_mi355x_gemm_4bit_route", "bnb_mi355x_gemm_4bit_fused_max_m",
       "bnb_mi355x_last_gemm_kernel",
       "bnb_mi355x_gemm_4bit_grouped", "bnb_mi355x_gemm_4bit_grouped_route",
       "bnb_mi355x_gemm_4bit_experts", "bnb_mi355x_gemm_4bit_experts_supported",
       "bnb_mi355x_gemm_4bit_experts_ffn", "bnb_mi355x_gemm_4bit_experts_ffn_supported",
       "bnb_mi355x_gemm_4bit_experts_combine", "bnb_mi355x_gemm_4bit_experts_combine_supported",
       "bnb_mi355x_gemm_4bit_experts_combine_plan",
       "bnb_mi355x_gemm_4bit_experts_gate_up", "bnb_mi355x_gemm_4bit_experts_gate_up_supported",
       "bnb_mi355x_gemm_4bit_experts_gate_up_plan",
       "bnb_mi355x_gemm_4bit_experts_mfma", "bnb_mi355x_gemm_4bit_experts_mfma_supported",
       "bnb_mi355x_int8_vectorwise_quant", "bnb_mi355x_gemm_int8", "bnb_mi355x_int8_mm_dequant", "bnb_mi355x_gemm_int8_route",
       "bnb_mi355x_int8_vectorwise_quant_mask", "bnb_mi355x_int8_outlier_addmm",
       "bnb_mi355x_optimizer_update_8bit_blockwise", "bnb_mi355x_optimizer_update_32bit", "bnb_mi355x_optimizer_update_grid",
       "bnb_mi355x_gemm_4bit_gated", "bnb_mi355x_gemm_4bit_gated_supported",
       "bnb_mi355x_gemm_4bit_lora", "bnb_mi355x_gemm_4bit_lora_supported",
       "bnb_mi355x_gemm_4bit_lora_ids", "bnb_mi355x_gemm_4bit_lora_ids_supported",
       "bnb_mi355x_lora_shrink", "bnb_mi355x_lora_shrink_supported",
       "bnb_mi355x_lora_shrink_ids", "bnb_mi355x_lora_shrink_ids_supported",
       "bnb_mi355x_moe_topk", "bnb_mi355x_moe_topk_supported",
       "bnb_mi355x_moe_topk_grouped", "bnb_mi355x_moe_topk_grouped_supported",
       "bnb_mi355x_gemm_4bit_grad_input", "bnb_mi355x_gemm_4bit_grad_input_workspace_bytes", "bnb_mi355x_gemm_4bit_grad_input_supported",
       "bnb_mi355x_peer_buffer_bytes", "bnb_mi355x_peer_alloc", "bnb_mi355x_peer_free", "bnb_mi355x_peer_export", "bnb_mi355x_peer_open",
       "bnb_mi355x_peer_close", "bnb_mi355x_peer_allgather", "bnb_mi355x_peer_status",
       "bnb_mi355x_peer_chain_buffer_bytes", "bnb_mi355x_peer_chain_alloc", "bnb_mi355x_gemv_4bit_peer_serves", "bnb_mi355x_gemv_4bit_peer",
       "bnb_mi355x_peer_chain_read",
       "bnb_mi355x_set_stream_tuning", "bnb_mi355x_gemv_4bit_stream_exact", "bnb_mi355x_stream_geometry", "bnb_mi355x_set_tuning",
       "bnb_mi355x_set_cu_count", "bnb_mi355x_gemm_4bit_plan", "bnb_mi355x_gemm_4bit_sm_form_plan", "bnb_mi355x_gemm_4bit_grad_input_plan",
       "bnb_mi355x_set_stamp_buffer", "bnb_mi355x_version"]
)
