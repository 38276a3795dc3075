/*
 * bnb_mi355x.h — C ABI of libbitsandbytes_mi355x.so, the MI355X (gfx950) native backend for the
 * bitsandbytes 4-bit quantized-linear path.
 *
 * The first group of entry points is exactly what the reference's ctypes layer binds for this path
 * (reference bitsandbytes/backends/cuda/ops.py:16-66): same names, same argument order, same types,
 * `void` return, errors reported as the reference's BNB_CHECK_RETURN does (message on stderr and
 * exit(1), reference csrc/compat.cuh:78-85). A reference build pointed at this library (see
 * INTEGRATION.md) runs its quantize_4bit / dequantize_4bit / gemm_4bit / gemv_4bit ops on these
 * kernels unchanged.
 *
 * Conventions (reference SURVEY §8b):
 *   - every pointer is a raw device address owned by the caller; outputs are pre-allocated; the
 *     library allocates nothing and keeps no pointer after return;
 *   - calls only enqueue work on `stream` (no synchronisation, no allocation): legal inside
 *     hipGraph capture;
 *   - packed weights: row-major flat over [N, K]; element 2i in the HIGH nibble and 2i+1 in the
 *     low nibble of byte i; quantization block j covers flat elements [j*bs, (j+1)*bs);
 *   - quant_type: 1 = FP4, 2 = NF4 (reference csrc/common.h:3-7);
 *   - `bnb_stream_t` is a hipStream_t passed as void*.
 *
 * fp16 / bf16 buffers are declared `void*` here so the header is usable from plain C.
 */
#ifndef BNB_MI355X_H
#define BNB_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bnb_stream_t;

/* ------------------------------------------------------------------------------------------------
 * 4-bit blockwise quantize — replaces reference csrc/pythonInterface.cpp:364-426
 * (cquantize_blockwise_<T>_{fp4,nf4}); `code` is unused (NULL). As in the reference these take NO
 * stream and run on the NULL stream. out: (n+1)/2 bytes; absmax: ceil(n/blocksize) floats.
 * blocksize in {32,64,...,4096}. Results are bit-identical to the reference CPU backend
 * (bitsandbytes/backends/default/ops.py:233-259).
 * ---------------------------------------------------------------------------------------------- */
void cquantize_blockwise_fp32_nf4(float* code, float* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_fp32_fp4(float* code, float* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_fp16_nf4(float* code, void* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_fp16_fp4(float* code, void* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_bf16_nf4(float* code, void* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_bf16_fp4(float* code, void* A, float* absmax, unsigned char* out, int blocksize, const int n);

/* 4-bit blockwise dequantize — replaces reference csrc/pythonInterface.cpp:346-444
 * (cdequantize_blockwise_<T>_{fp4,nf4}); n = number of OUTPUT elements. */
void cdequantize_blockwise_fp32_nf4(float* code, unsigned char* A, float* absmax, float* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_fp32_fp4(float* code, unsigned char* A, float* absmax, float* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_fp16_nf4(float* code, unsigned char* A, float* absmax, void* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_fp16_fp4(float* code, unsigned char* A, float* absmax, void* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_bf16_nf4(float* code, unsigned char* A, float* absmax, void* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_bf16_fp4(float* code, unsigned char* A, float* absmax, void* out, int blocksize, const int n, bnb_stream_t stream);

/* 8-bit blockwise pair with a 256-entry fp32 `code` (General8bit) — replaces reference
 * csrc/pythonInterface.cpp:346-444 (cquantize_blockwise_<T> / cdequantize_blockwise_<T>). On this
 * path they only (de)compress the absmax vector for double quantization. Quantize follows the
 * reference CPU kernel's 65536-bin rule (csrc/cpu_ops.cpp:501-665). Quantize: NULL stream. */
void cquantize_blockwise_fp32(float* code, float* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_fp16(float* code, void* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cquantize_blockwise_bf16(float* code, void* A, float* absmax, unsigned char* out, int blocksize, const int n);
void cdequantize_blockwise_fp32(float* code, unsigned char* A, float* absmax, float* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_fp16(float* code, unsigned char* A, float* absmax, void* out, int blocksize, const int n, bnb_stream_t stream);
void cdequantize_blockwise_bf16(float* code, unsigned char* A, float* absmax, void* out, int blocksize, const int n, bnb_stream_t stream);

/* Fused dequantize + GEMM — replaces reference csrc/gemm_4bit.cu:138-166.
 *   out[M,N] = A[M,K] * dequant(B)[N,K]^T (+ bias[N])
 *   scale of block b = absmax[b]                                            (absmax_8bit == NULL)
 *                    = absmax_code[absmax_8bit[b]] * absmax[b >> 8] + *absmax_offset   (nested)
 * K % blocksize == 0 is guaranteed by the caller (reference backends/cuda/ops.py:956-962);
 * absmax_offset is fp32; bias has A's dtype. M is any positive value: M = 1 (and M <= 4 on matrices of fewer than 128 rows,
 * M = 2 on long rows of small matrices) runs the streaming kernel (gemv4_stream.hip: persistent workgroups, weights through a
 * register ring, any M in row passes of up to four); 2 ... 16 rows on matrices of >= 128 rows the streaming MFMA kernel
 * (gemm4_mfma_sm.hip: one persistent workgroup per CU, one decode for all rows, activations once per CU; K % 256 != 0: to 128 rows); larger M and smaller
 * matrices the other MFMA kernels (gemm4_mfma_rt.hip / gemm4_mfma.hip / gemm4_mfma_kq.hip: bf16 / fp16, K % 256 == 0, blocksize
 * >= 64, aligned pointers; any M in row tiles); shapes the MFMA kernels do not take (fp32, odd K, small blocks) run the
 * streaming kernel at any M. */
void cgemm_4bit_bf16(const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
void cgemm_4bit_fp16(const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
void cgemm_4bit_fp32(const float* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, float* out, const float* bias, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);

/* Legacy gemv (M = 1) — replaces reference csrc/pythonInterface.cpp:594-613.
 * m = N (output features), n = 1, k = K; `datatype` = the 16-entry fp32 code table on the device;
 * absmax already un-nested; lda/ldb/ldc are ignored exactly as the reference kernel ignores them
 * (it indexes B flat, reference csrc/kernels.cu:1452-1567). */
void cgemm_4bit_inference_naive_fp16(int m, int n, int k, void* A, unsigned char* B, float* absmax, float* datatype, void* out, int lda, int ldb, int ldc, int blocksize, bnb_stream_t stream);
void cgemm_4bit_inference_naive_bf16(int m, int n, int k, void* A, unsigned char* B, float* absmax, float* datatype, void* out, int lda, int ldb, int ldc, int blocksize, bnb_stream_t stream);
void cgemm_4bit_inference_naive_fp32(int m, int n, int k, float* A, unsigned char* B, float* absmax, float* datatype, float* out, int lda, int ldb, int ldc, int blocksize, bnb_stream_t stream);

/* Loader symbols the reference's cextension.py:109-115,371-372 probes to classify a GPU library.
 * get_context returns an opaque non-NULL token (this path needs no BLAS handle);
 * cget_managed_ptr returns hipMallocManaged memory (reference csrc/pythonInterface.cpp:522,557-563). */
void* get_context(void);
void* cget_managed_ptr(size_t bytes);

/* ------------------------------------------------------------------------------------------------
 * Extensions (not in the reference ABI). Used by bitsandbytes_amd's own host layer.
 * ---------------------------------------------------------------------------------------------- */

/* Stream-ordered 4-bit / 8-bit quantize: same kernels as the cquantize_blockwise_* family above but
 * enqueued on `stream`. dtype: 0 = fp32, 1 = fp16, 2 = bf16. */
void bnb_mi355x_quantize_4bit(const void* A, int dtype, float* absmax, unsigned char* out, int blocksize, long n, int quant_type, bnb_stream_t stream);
void bnb_mi355x_quantize_8bit(const float* code, const void* A, int dtype, float* absmax, unsigned char* out, int blocksize, long n, bnb_stream_t stream);

/* quantize_4bit(compress_statistics=True) as ONE call (reference bitsandbytes/functional.py:925-951: quantize_4bit, absmax.mean(),
 * absmax - offset, quantize_blockwise(..., blocksize=256) - four to six launches and host dispatches; here three launches behind one).
 * A: n elements of dtype; out: (n + 1) / 2 packed bytes; scratch: device buffer of ceil(n / blocksize) + 1536 floats (the fp32 absmax of
 * the 4-bit blocks, then 256 partial sums, then 1280 dwords of encoder tables built once per call; contents are unspecified afterwards); code8: the 256-entry 8-bit code (fp32, device, ascending:
 * the dynamic map); absmax_8bit: ceil(n / blocksize) codes; absmax2: ceil(ceil(n / blocksize) / 256) floats; offset: 1 float =
 * the mean of the fp32 absmax, summed in a FIXED order (a balanced binary tree over 1024-element steps, see csrc/blockwise8.hip:
 * the same bits on every launch, any device). absmax_8bit / absmax2 are bit for bit what quantize_blockwise gives on absmax - offset. */
void bnb_mi355x_quantize_4bit_nested(const void* A, int dtype, long n, int blocksize, int quant_type, unsigned char* out, float* scratch, const float* code8, unsigned char* absmax_8bit, float* absmax2, float* offset, bnb_stream_t stream);

/* dequantize_4bit for double-quantised statistics in ONE launch (reference bitsandbytes/functional.py:1002-1006 is three operator
 * calls: dequantize_blockwise(absmax, state2), `+= offset`, dequantize_4bit): the scale of 4-bit block b is reconstructed in the kernel as
 * absmax_code[absmax_8bit[b]] * absmax2[b >> 8] + *absmax_offset (fp32 product, then fp32 sum: the same two roundings). Second-level
 * blocksize 256. n = number of OUTPUT elements; dtype: 0 = fp32, 1 = fp16, 2 = bf16. */
void bnb_mi355x_dequantize_4bit_nested(int dtype, const unsigned char* A, const unsigned char* absmax_8bit, const float* absmax2, const float* absmax_code, const float* absmax_offset, void* out, int blocksize, long n, int quant_type, bnb_stream_t stream);

/* Row gather + 4-bit dequantize in one launch: out[t, 0:row_len] = dequantize(row indices[t]) for
 * t < rows_out. The fused form of the Embedding4bit lookup (reference bitsandbytes/nn/modules.py:921-951:
 * F.embedding on the packed bytes, F.embedding on absmax, dequantize_4bit). A is the packed
 * [num_rows, row_len] table, absmax its fp32 scales (un-nested); row_len % 8 == 0 and
 * row_len % blocksize == 0; indices are int32 (index_bytes 4) or int64 (8). Values are bit-identical to
 * cdequantize_blockwise_* applied to the gathered rows. An index outside [0, num_rows) gives a row of NaN. A must be 4-byte aligned
 * (the packed rows are read a dword at a time) and out 16-byte aligned; absmax and indices need their element's alignment. A call
 * outside these preconditions prints a message and ends the process, like every failed launch of this ABI. */
void bnb_mi355x_dequantize_4bit_rows(int dtype, const unsigned char* A, const float* absmax, const void* indices, int index_bytes, void* out, long rows_out, long num_rows, int row_len, int blocksize, int quant_type, bnb_stream_t stream);

/* gemm_4bit with an explicit kernel choice and a caller-owned split-K workspace:
 * kernel = 0 auto, 1 / 3 streaming dot kernel, 2 MFMA kernels. dtype as above; code16 may be NULL.
 * workspace: device buffer of bnb_mi355x_gemm_4bit_workspace_bytes(...) bytes (may be NULL / smaller:
 * the MFMA kernel then uses fewer K slices, or a library-owned per-stream buffer when NULL and the
 * stream is not being captured). Its contents are scratch; no initialisation is required. */
void bnb_mi355x_gemm_4bit(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const float* code16, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, void* workspace, size_t workspace_bytes, bnb_stream_t stream);
size_t bnb_mi355x_gemm_4bit_workspace_bytes(int kernel, int dtype, int M, int N, int K, int blocksize);
/* Which kernel family bnb_mi355x_gemm_4bit(kernel, ...) runs for this problem (aligned pointers assumed): 0 = streaming
 * kernel, 1 = MFMA kernels. The grouped entry point below goes matrix by matrix when any member answers 1.
 * Size: the streaming kernel and every MFMA kernel serve weights of N * K < 2^32 elements (the K-quarter kernel N * K < 2^31; 32-bit
 * byte offsets under descriptors of 2^31 - 1 records). From 2^32 elements on the answer is 0 at every M and the call runs the generic
 * scalar kernel (family 2, 64-bit addressing, correct and slow); the gated, LoRA and grouped-streaming forms answer "not supported"
 * there. The expert-indexed kernel (E * N < 2^31 rows) and the fused backward have no element limit. */
int bnb_mi355x_gemm_4bit_route(int kernel, int dtype, int M, int N, int K, int blocksize);
/* The fused range of bitsandbytes::gemm_4bit, stated once for every dispatcher of the op (the C++-registered kernel, the Python one,
 * the tests): the largest M at which a call on an N x K weight of this blocksize and kind of statistics (nested: double-quantised)
 * stays on the fused kernels above; taller batches dequantize once and run a dense GEMM. fp16 / bf16: one of 16, 128, 512, 640, 1024
 * (the measurements are quoted at the definition, csrc/gemm4_mfma.hip); fp32: 4. A pure function of its arguments: it reads neither the
 * CU count nor the tuning knobs, so a caller may cache the answer. K % blocksize != 0 is the caller's to refuse. */
int bnb_mi355x_gemm_4bit_fused_max_m(int dtype, int N, int K, int blocksize, int nested);
/* Which kernel family the calling thread's LAST gemm_4bit / gemv_4bit call (any entry point) launched: 0 none yet, 1 streaming
 * kernel (gemv4_stream_kernel), 2 generic scalar kernel (odd shapes), 3 register-transposed MFMA kernel (gemm4_mfma_rt_kernel),
 * 4 producer/consumer MFMA kernel (gemm4_mfma_pc_kernel), 6 K-quarter MFMA kernel (gemm4_mfma_kq_kernel),
 * 7 streaming MFMA kernel (gemm4_mfma_sm_kernel: 2 ... 16 rows, one persistent workgroup per CU), 9 expert-indexed kernel
 * (gemm4_experts_kernel: bnb_mi355x_gemm_4bit_experts). Debug / test query:
 * a test that forces a kernel with bnb_mi355x_set_tuning asserts here that it ran (a geometry the forced kernel does not
 * serve falls back to another family by design). */
int bnb_mi355x_last_gemm_kernel(void);

/* Expert-indexed gemm_4bit for mixture-of-experts decode, ONE launch for any id pattern:
 *   out[p, 0:N] = x_row(p) * dequant(B[ids[p]])^T (+ bias[ids[p], 0:N])        p = 0 .. P-1, P = T * S (token, slot) pairs
 * B / absmax (/ absmax_8bit, absmax_code, absmax_offset: nested statistics, as in cgemm_4bit_*) are the result of ONE quantize_4bit
 * over a contiguous [E, N, K] tensor: expert e is rows e * N .. (e + 1) * N - 1 of the flat [E * N, K] matrix, and the second-level
 * groups of 256 blocks run over the flat tensor (they may straddle experts). ids: P values on the DEVICE, int32 (index_bytes 4) or
 * int64 (8), read by the kernel only - the host never looks at them, so the call needs no synchronisation and can be captured in a
 * hipGraph and replayed with other ids in the same buffer. An id outside [0, E) gives a row of zeros (no bias) and reads no weight.
 * x_row(p) = A + p * K when a_slot_stride == K (A is [P, K]: one activation row per pair) and A + (p / S) * K when a_slot_stride == 0
 * (A is [P / S, K]: the S slots of a token share its row). bias: NULL or [E, N] of A's dtype. dtype: 0 = fp32, 1 = fp16, 2 = bf16;
 * fp32 accumulation, one rounding. Workgroups of experts nobody selected leave after reading the id list; an expert's weights are
 * streamed once per four pairs that select it; every output element is summed in a fixed order that does not depend on the other
 * pairs of the call (no atomics). A, B and out must be 16-byte aligned. P <= 0 returns without a launch. A geometry for which
 * bnb_mi355x_gemm_4bit_experts_supported (pure host logic, no device needed) answers 0 - K not a multiple of blocksize, blocksize not
 * a power of two >= 32, K > 131072, E > 65535 - terminates like every failed launch of this ABI: ask first. */
void bnb_mi355x_gemm_4bit_experts(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes, void* out, long P, int S, int E, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
int bnb_mi355x_gemm_4bit_experts_supported(int dtype, int E, int N, int K, int blocksize);
/* The same launch with one of two epilogues - the two expert projections of a gated-SiLU MoE FFN block (family 9 as well):
 *   gated = 1 (chunked) / 2 (interleaved): an expert's matrix is [N = 2 I, K] with gate rows 0 .. I-1 and up rows I .. 2 I - 1
 *     (chunked: torch.chunk(2, -1) of the fused projection's output) or gate row 2 i and up row 2 i + 1 (interleaved); bias, if given,
 *     [E, 2 I] in the same layout. out is [P, I]:  g = T(acc_g + bias_g), u = T(acc_u + bias_u), out = T(float(T(silu(g))) * float(u))
 *     with silu(g) = g / (1 + expf(-g)) in fp32 - bit for bit what `F.silu(g) * u` gives on the T-valued output of the plain call.
 *   row_scale != NULL: out[p, n] = T((acc + bias) * w[p]), w[P] on the device, fp32 (row_scale_dtype 0) or of A's dtype
 *     (row_scale_dtype == dtype), read as it is: the routing weights of the down projection, one fp32 multiply in front of the
 *     single rounding.
 * The two exclude each other; with gated = 0 and row_scale = NULL this is bnb_mi355x_gemm_4bit_experts. A pair whose id is outside
 * [0, E) stays a row of zeros (I wide when gated) and its scale is never read into the result. N is the number of WEIGHT rows per
 * expert. bnb_mi355x_gemm_4bit_experts_ffn_supported: the predicate above, and N even when gated != 0 (pure host logic). */
void bnb_mi355x_gemm_4bit_experts_ffn(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes, const void* row_scale, int row_scale_dtype, int gated, void* out, long P, int S, int E, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
int bnb_mi355x_gemm_4bit_experts_ffn_supported(int dtype, int E, int N, int K, int blocksize, int gated);
/* Dense gated-SiLU FFN: the fused matmul over ONE interleaved matrix B [N = 2 F, K] - gate row i at row 2 i, up row i at row 2 i + 1;
 * bias, if given, [N] in the same layout - with silu(gate) * up as its epilogue. A is [M, K], out is [M, F]:
 *     g = T(acc_g + bias_g), u = T(acc_u + bias_u), out[m, i] = T(float(T(silu(g))) * float(u)),  silu(g) = g / (1 + expf(-g)) in fp32
 * - bit for bit what `F.silu(y[:, 0::2]) * y[:, 1::2]` gives on the output y of bnb_mi355x_gemm_4bit on the same matrix, because the
 * launch is the kernel family that call runs, and it exists only where that family is the streaming kernel (1) or the streaming MFMA
 * kernel (7); bnb_mi355x_last_gemm_kernel reports 1 or 7 as for the plain call. dtype 1 / 2 (fp16 / bf16) only, fp32 absmax only
 * (un-nest double-quantised statistics first), 1 <= M <= 16, N even, blocksize >= 64, K % blocksize == 0, A / B 16-byte aligned.
 * N is the number of WEIGHT rows (2 F). A call outside these preconditions prints a message and ends the process, like every failed
 * launch of this ABI: ask bnb_mi355x_gemm_4bit_gated_supported first (pure host logic over the shapes, aligned pointers assumed; it
 * needs no device beyond the CU count the route queries use) and compose the plain call with silu and a multiply where it says 0. */
void bnb_mi355x_gemm_4bit_gated(int dtype, const void* A, const uint8_t* B, const float* absmax, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
int bnb_mi355x_gemm_4bit_gated_supported(int dtype, int M, int N, int K, int blocksize);
/* LoRA adapter beside a 4-bit base layer, y = base(x) + scaling * lora_B(lora_A(x)), with the adapter term as the EPILOGUE of the
 * fused matmul: A [M, K], B / statistics / bias as for bnb_mi355x_gemm_4bit (fp32 absmax, or nested statistics with absmax_8bit != NULL),
 * lora_t [M, r] = x @ lora_A^T (the caller's small matmul), lora_b [N, r] = lora_B.weight as stored (row-major), both of A's type:
 *     lora[m, n] = sum_{j < r} float(t[m, j]) * float(B_l[n, j])      fp32, in an order that depends on r (and the family) only
 *     out[m, n]  = T((acc[m, n] + bias[n]) + scaling * lora[m, n])    acc = the plain call's fp32 sum; ONE rounding to T
 * The launch is the kernel family the plain call on the same matrix, M and statistics runs, and it exists only where that family is the
 * streaming kernel (1) or the streaming MFMA kernel (7); bnb_mi355x_last_gemm_kernel reports 1 or 7. With t == 0 the result is the
 * plain call's. dtype 1 / 2 (fp16 / bf16) only, 1 <= M <= 16, blocksize >= 64, K % blocksize == 0, r % 8 == 0, 8 <= r <= 128,
 * A / B / lora_t / lora_b 16-byte aligned. A call outside these preconditions prints a message and ends the process, like every failed
 * launch of this ABI: ask bnb_mi355x_gemm_4bit_lora_supported first (pure host logic over the shapes, aligned pointers assumed, 256 CUs
 * without a device) and add the adapter term with a second launch where it says 0. */
void bnb_mi355x_gemm_4bit_lora(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, void* out, const void* bias, const void* lora_t, const void* lora_b, float scaling, int r, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
int bnb_mi355x_gemm_4bit_lora_supported(int dtype, int M, int N, int K, int blocksize, int nested, int r);
/* Mixed-adapter form of bnb_mi355x_gemm_4bit_lora: a decode batch in which every row (request) has its own adapter. lora_b [A_n, N, r]
 * row-major - the lora_B.weight of A_n adapters of ONE rank r, stacked -, scalings [A_n] fp32 and ids [M] (int32 / int64: index_bytes
 * 4 / 8) on the DEVICE, read by the kernel only; 1 <= A_n <= 64:
 *     out[m, n] = T((acc[m, n] + bias[n]) + scalings[ids[m]] * sum_j float(t[m, j]) * float(lora_b[ids[m], n, j]))    0 <= ids[m] < A_n
 *     out[m, n] = the plain bnb_mi355x_gemm_4bit call's bits                                                          otherwise
 * The whole 64-bit id is compared before any address is formed from it. A row without an adapter SKIPS the adapter term: its lora_t
 * row and the scalings are never read. A row with one is BIT-IDENTICAL to row m of bnb_mi355x_gemm_4bit_lora(..., lora_t,
 * lora_b + ids[m] * N * r, scalings[ids[m]], ...) at the same M, N, K and statistics: the same kernel family and instance skeleton,
 * the same order of the adapter sum. Streaming kernel: the row's thread reads B_l's row from its adapter's matrix. Streaming MFMA
 * kernel: the tile's wavefront loops over the distinct in-range ids of the batch in ascending order, one MFMA chain from a zero
 * accumulator per adapter (t's lanes of other rows are out-of-range loads; lora_b's buffer resource is rebased per adapter with 64-bit
 * arithmetic, so no bound on A_n * N * r), and keeps of each product only the rows of that adapter. Every other precondition: as for
 * bnb_mi355x_gemm_4bit_lora; ids aligned to index_bytes. bnb_mi355x_gemm_4bit_lora_ids_supported answers 1 exactly where
 * bnb_mi355x_gemm_4bit_lora_supported does, for every 1 <= A_n <= 64. */
void bnb_mi355x_gemm_4bit_lora_ids(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, void* out, const void* bias, const void* lora_t, const void* lora_b, const float* scalings, const void* ids, int index_bytes, int A_n, int r, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t stream);
int bnb_mi355x_gemm_4bit_lora_ids_supported(int dtype, int M, int N, int K, int blocksize, int nested, int r, int A_n);
/* LoRA shrink, the launch in front of bnb_mi355x_gemm_4bit_lora: x [M, K] and lora_a [R, K] row-major (lora_A.weight as stored, or up
 * to eight of them concatenated along dim 0), T = fp16 / bf16 (dtype 1 / 2) for both and for t:
 *     t[m, j] = T( sum_{k < K} float(x[m, k]) * float(lora_a[j, k]) )      fp32 sum, ONE rounding to T
 * The order of the sum is a function of K alone: K is cut into steps of 32 k, wavefront w of sixteen adds steps w, w + 16, ... in
 * ascending order into one fp32 accumulator (a step is one v_mfma_f32_16x16x32), and the sixteen accumulators are added in ascending
 * w. It does not depend on M, on R, on where row j sits in lora_a, on the splits or on the grid: a stacked call's parts are
 * bit-identical to separate calls on the members. One launch, no workspace, no traffic between workgroups.
 * splits (a HOST array of n_splits ints, read during the call and passed to the kernel by value; n_splits 0 ... 8): with n_splits == 0
 * t is [M, R]. Otherwise part i is a CONTIGUOUS [M, splits[i]] matrix at element offset M * (splits[0] + ... + splits[i-1]) of t (M * R
 * elements in all), so every part is 16-byte aligned and can be passed as lora_t to bnb_mi355x_gemm_4bit_lora as it is.
 * 1 <= M <= 16, K % 64 == 0, R % 8 == 0, 8 <= R <= 1024, every splits[i] % 8 == 0 and in [8, 128], sum of splits == R, x / lora_a / t
 * 16-byte aligned. A call outside these preconditions prints a message and ends the process. bnb_mi355x_lora_shrink_supported (pure
 * host logic, aligned pointers assumed) answers 1 where the preconditions hold AND the launch measured ahead of the BLAS matmul it
 * replaces; compose the matmul yourself where it says 0. */
void bnb_mi355x_lora_shrink(int dtype, const void* x, const void* lora_a, void* t, int M, int R, int K, const int* splits, int n_splits, bnb_stream_t stream);
int bnb_mi355x_lora_shrink_supported(int dtype, int M, int R, int K);
/* Mixed-adapter LoRA shrink: a decode batch in which every row (request) has its own adapter. lora_a [A_n, R, K] row-major - the
 * lora_A.weight of A_n adapters, stacked -, 1 <= A_n <= 64; ids: M values on the DEVICE, int32 (index_bytes 4) or int64 (8), read by
 * the kernel only: no host synchronisation, and a captured graph follows new ids written into the same buffer.
 *     t[m, j] = T( sum_{k < K} float(x[m, k]) * float(lora_a[ids[m], j, k]) )      0 <= ids[m] < A_n
 *     t[m, :] = 0                                                                  otherwise: the row has no adapter
 * The whole 64-bit id is compared (2^32 + 1 is out of range, not adapter 1), before any address is formed. A row with an adapter is
 * BIT-IDENTICAL to row m of bnb_mi355x_lora_shrink(x, lora_a + ids[m] * R * K, ...) at the same M: same steps, same order. One launch
 * on a grid of (R / 8, A_n) workgroups; those of an adapter that no row names return before they read lora_a or x, so the traffic is
 * that of the distinct adapters of the batch; every element of t is written exactly once (rows without an adapter by adapter 0's
 * workgroups). splits, t's layout and every other precondition: as for bnb_mi355x_lora_shrink; ids aligned to index_bytes. A call
 * outside the preconditions prints a message and ends the process. bnb_mi355x_lora_shrink_ids_supported (pure host logic, aligned
 * pointers assumed) answers 1 where the preconditions hold, minus the classes in which the launch measured behind the gathered
 * torch.bmm it replaces (none excluded so far). */
void bnb_mi355x_lora_shrink_ids(int dtype, const void* x, const void* lora_a, const void* ids, int index_bytes, void* t, int M, int A_n, int R, int K, const int* splits, int n_splits, bnb_stream_t stream);
int bnb_mi355x_lora_shrink_ids_supported(int dtype, int M, int A_n, int R, int K);

/* MoE router, scoring and top-k: the launch between the router matmul (logits = x * Wr^T, the caller's launch: the shape class of
 * bnb_mi355x_lora_shrink with R = experts) and bnb_mi355x_gemm_4bit_experts / _ffn, which take ids and weights as written here.
 * Per row of logits [rows, experts] (row-major, fp32 / fp16 / bf16), all arithmetic in fp32:
 *     p_j = softmax(l)_j = expf(l_j - max l) / Z          scoring 0; Z summed lane-local over j = lane + 64 i in ascending i, then over
 *                                                          the 64 lanes by the xor butterfly 32, 16, ... 1
 *     p_j = 1 / (1 + expf(-l_j))                           scoring 1 (sigmoid)
 *     c_j = p_j, or p_j + select_bias[j]                   the selection key (select_bias: fp32 [experts], DeepSeek-V3 / GLM's
 *                                                          e_score_correction_bias; it takes part in the selection only)
 *     ids[r, 0 ... top_k) = the experts of largest key, best first. a goes before b when c_a > c_b, or c_a == c_b and a < b (ties:
 *                           the lower index). A NaN key goes behind every other key; NaN keys among themselves by ascending index.
 *                           The ids of a row are therefore always distinct and in [0, experts), whatever the logits hold.
 *     weights[r, s] = p_ids[r,s]                           the UNBIASED score, fp32
 *                     / (w_0 + w_1 + ... + w_top_k-1)      if renormalize: summed in slot order. No epsilon: a zero sum gives what IEEE
 *                                                          division gives (inf, or NaN for 0 / 0)
 *                     * scale                              always (routed_scaling_factor; 1.0f is exact)
 * A row's result depends on that row alone: not on rows, on the row's place or on the grid. One launch, one wavefront per row, four
 * per workgroup, no LDS, no workspace, no traffic between workgroups; nothing is read on the host, so the call can be captured.
 * 1 <= experts <= 1024 (any value, not only multiples of 8 or 64), 1 <= top_k <= min(experts, 16), rows >= 0; every pointer aligned
 * to its element (2 or 4 bytes), nothing more. Group-limited routing (n_group / topk_group): bnb_mi355x_moe_topk_grouped, below.
 * The call takes ONE pointer to an argument block; struct_bytes must be sizeof of the block the caller was compiled with, so a
 * caller built against another version of this header is refused instead of misread. Returns 0 after the launch (rows == 0: 0, nothing
 * launched). A call outside the preconditions - wrong struct_bytes, a NULL logits / ids / weights, a dtype, scoring, experts or top_k
 * out of range, rows < 0, a misaligned pointer - prints one line on stderr, launches nothing and returns non-zero; unlike the void
 * entry points above it does NOT end the process. bnb_mi355x_moe_topk_supported (pure host logic, aligned pointers assumed)
 * answers 1 where the preconditions hold and rows >= 1, minus the classes in which the launch measured behind the torch composition
 * it replaces (none excluded so far). */
typedef struct bnb_mi355x_moe_topk_args {
    size_t struct_bytes;            /* sizeof of this struct as the caller was compiled */
    int logits_dtype;               /* 0 fp32, 1 fp16, 2 bf16 */
    int scoring;                    /* 0 softmax, 1 sigmoid */
    int renormalize;
    int rows, experts, top_k;
    float scale;
    const void* logits;             /* [rows, experts] row-major */
    const float* select_bias;       /* [experts] or NULL */
    int* ids; float* weights;       /* [rows, top_k] each */
    bnb_stream_t stream;
} bnb_mi355x_moe_topk_args;
int bnb_mi355x_moe_topk(const bnb_mi355x_moe_topk_args* args);
int bnb_mi355x_moe_topk_supported(int logits_dtype, int rows, int experts, int top_k);
/* Group-limited routing - the router of DeepSeek-V2, DeepSeek-V3 / R1 and GLM-4.5 - as the same ONE launch. Scores, keys, the order
 * of the selection, weights, layouts and every convention of the call: as for bnb_mi355x_moe_topk, above. In addition the experts
 * are n_group contiguous groups of G = experts / n_group: group g holds the experts g G ... g G + G - 1.
 *     group score, group_score 0 (max):      the first key of the group in the order of the selection (DeepSeek-V2)
 *                  group_score 1 (top2sum):  first key + second key, one fp32 add (DeepSeek-V3 / GLM); needs G >= 2
 *     the topk_group groups that go first in the same order, taken on the pair group score / group index, stay: ties go to the
 *     lower group, a NaN score goes last
 *     ids = top_k rounds of the selection over the experts of the groups that stay. An expert of a dropped group never takes part:
 *     it is not a key of 0, so it never goes before an expert of a kept group whose biased key is negative
 * Any G is served, also one that is no power of two and no divisor of 64. With n_group == 1 or topk_group == n_group the result has
 * the bits of bnb_mi355x_moe_topk. experts % n_group == 0, 1 <= topk_group <= n_group <= 64, 1 <= experts <= 1024,
 * 1 <= top_k <= min of topk_group * G and 16. A call outside the preconditions prints one line on stderr, launches nothing and returns
 * non-zero. bnb_mi355x_moe_topk_grouped_supported answers 1 where the preconditions hold and rows >= 1, minus the classes in which
 * the launch measured behind the torch composition it replaces (none excluded so far). */
typedef struct bnb_mi355x_moe_topk_grouped_args {
    size_t struct_bytes;            /* sizeof of this struct as the caller was compiled */
    int logits_dtype;               /* 0 fp32, 1 fp16, 2 bf16 */
    int scoring;                    /* 0 softmax, 1 sigmoid */
    int renormalize;
    int rows, experts, top_k;
    int n_group, topk_group;
    int group_score;                /* 0 max, 1 top2sum */
    float scale;
    const void* logits;             /* [rows, experts] row-major */
    const float* select_bias;       /* [experts] or NULL */
    int* ids; float* weights;       /* [rows, top_k] each */
    bnb_stream_t stream;
} bnb_mi355x_moe_topk_grouped_args;
int bnb_mi355x_moe_topk_grouped(const bnb_mi355x_moe_topk_grouped_args* args);
int bnb_mi355x_moe_topk_grouped_supported(int logits_dtype, int rows, int experts, int top_k, int n_group, int topk_group, int group_score);

/* Grouped gemm_4bit: `count` weight matrices applied to the SAME activations A[M, K] in one launch -
 *   out[i][M, N[i]] = A * dequant(B[i])^T (+ bias[i])        i = 0 .. count-1
 * (the Q/K/V projections of an attention block, the gate/up projections of an MLP: reference callers issue one
 * gemm_4bit per matrix, bitsandbytes/nn/modules.py:609-637). All matrices share K, blocksize, quant_type and
 * nested-ness (absmax_8bit is NULL, or non-NULL for every matrix). The arrays are HOST arrays of device pointers
 * / ints, read during the call. count <= 8: ONE launch - of the streaming MFMA kernel when every member's own route is that
 * kernel (2 ... 16 rows; workgroups dealt to the members by rows), of the streaming kernel over the concatenated rows when no
 * member's route is an MFMA kernel (M <= 4) - one kernel boundary, one decode-table build, one activation copy per CU;
 * otherwise the matrices are launched one by one. Results are bit-identical to `count` separate cgemm_4bit_* calls - with ONE
 * exception: groups of 17 ... 64 rows up to 96 M weights (72 M from 33 rows) are one launch of the streaming MFMA kernel - its 32-row
 * instances - although the members' own route at that many rows is another MFMA kernel (4 x 4096^2 at 32 rows: 17.3 us against 33.4
 * matrix by matrix): same values within the fused calls' tolerance, bit-reproducible, not bit-identical to separate calls.
 * bnb_mi355x_gemm_4bit_grouped_route: which of these a group takes (2 / 1 / 0), from shapes alone (aligned pointers assumed). */
int bnb_mi355x_gemm_4bit_grouped_route(int dtype, int count, const int* N, int M, int K, int blocksize);
void bnb_mi355x_gemm_4bit_grouped(int dtype, const void* A, int count, const uint8_t* const* B, const float* const* absmax, const uint8_t* const* absmax_8bit, const float* const* absmax_code, const float* const* absmax_offset, void* const* out, const void* const* bias, const int* N, int M, int K, int blocksize, int quant_type, bnb_stream_t stream);

/* Fused backward of the 4-bit linear layer (MatMul4Bit.backward, reference bitsandbytes/autograd/_functions.py:365-386, which
 * dequantizes the whole weight and calls a dense matmul):
 *   grad_A[M, K] = grad_out[M, N] * dequant(B)[N, K]      dequant = T(code * scale), exactly dequantize_4bit's arithmetic
 * dtype 1 = fp16, 2 = bf16; argument meaning of the weight side as in cgemm_4bit_*. Requires N % 64 == 0, K % 128 == 0,
 * blocksize >= 64, 16-byte aligned grad_out / B (bnb_mi355x_gemm_4bit_grad_input_supported; an unsupported call is a fatal
 * error like a failed launch). workspace: device scratch of bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K) bytes
 * (fp32 slabs of the N slices; contents need no initialisation; with less the launch uses fewer slices). */
void bnb_mi355x_gemm_4bit_grad_input(int dtype, const void* grad_out, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, void* grad_A, int M, int N, int K, int blocksize, int quant_type, void* workspace, size_t workspace_bytes, bnb_stream_t stream);
size_t bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(int M, int N, int K);
int bnb_mi355x_gemm_4bit_grad_input_supported(int dtype, int M, int N, int K, int blocksize);

/* One-shot all-gather of small per-rank outputs over peer-mapped buffers (bitsandbytes_amd/csrc/peer_gather.hip): the exchange
 * step of the N-sharded 4-bit linear layer at decode sizes (2.7 KB per rank), one kernel per collective, capturable in a hipGraph.
 * Nothing in the reference to mirror (it has no collective code); bitsandbytes_amd/peer.py is the host side.
 *   buffer_bytes : size of one rank's buffer for shards of up to max_bytes in a group of `world` (<= 8) ranks
 *   alloc / free : fine-grained device memory on the current device, zeroed
 *   export       : 64-byte hipIpc handle of an allocated buffer (0 = ok); open / close: map / unmap a peer's buffer
 *   allgather    : bufs = HOST array of `world` device pointers (rank r's buffer as mapped into this process, bufs[rank] local);
 *                  src = this rank's shard (bytes <= max_bytes), out = world x bytes, rank-major (all_gather_into_tensor's layout).
 *                  Every rank of the group must call it the same number of times with the same `bytes`.
 *   status       : 0, or 1 once a wait ran into its bound (tens of seconds; BNB_MI355X_PEER_WAIT_POLLS) because a peer never arrived
 *                  (synchronises the device). */
size_t bnb_mi355x_peer_buffer_bytes(int world, size_t max_bytes);
void* bnb_mi355x_peer_alloc(size_t bytes);
void bnb_mi355x_peer_free(void* buffer);
int bnb_mi355x_peer_export(void* buffer, void* handle64);
void* bnb_mi355x_peer_open(const void* handle64);
void bnb_mi355x_peer_close(void* mapped);
void bnb_mi355x_peer_allgather(void* const* bufs, int world, int rank, const void* src, void* out, size_t bytes, size_t max_bytes, bnb_stream_t stream);
int bnb_mi355x_peer_status(const void* local_buffer);

/* Peer chain: the all-gather of the N-sharded layer FUSED into the gemv launches on either side of it (M = 1 decode; fp16 /
 * bf16). Each rank owns an exchange buffer of bnb_mi355x_peer_chain_buffer_bytes(max_values) bytes (max_values a multiple of 4) from
 * bnb_mi355x_peer_chain_alloc (zeroed; fine_grained != 0 = hipDeviceMallocFinegrained, REQUIRED whenever the ranks sit on different
 * devices: remote stores into coarse-grained memory that a running kernel of the owner polls are outside what HIP guarantees;
 * 0 = ordinary cacheable memory, enough where all ranks share one device), exported / mapped / freed like the gather buffers above;
 * bufs[r] = rank r's buffer as mapped here. bnb_mi355x_gemv_4bit_peer_serves = the launcher's own shape check without a launch. y travels as
 * 8-byte granules {two consecutive values, u32 tag}: the producing launch stores them straight into every rank's buffer, the
 * consuming launch - the next layer - fetches them behind its weight requests and re-fetches the ones whose tag is not there
 * yet. No separate collective launch, no flag, no fence (csrc/gemv4_stream.hip, PeerChain).
 *   mode bit 0: x = the current exchange (K values; A is ignored)     bit 1: y (ns values of this rank, rank-major) goes to the
 *   exchange; it is also written to out_local[ns] when that is non-NULL. A launch with bit 1 completes one exchange.
 *   mode bit 3 (with bit 1), "gated": the launch runs over a matrix whose rows INTERLEAVE this rank's gate and up rows (row 2 r =
 *   gate row r, row 2 r + 1 = up row r; ns % 4 == 0) and what goes to the exchange is a[r] = T(T(silu(g_r)) * u_r) - ns / 2 values
 *   per rank, each op in fp32 and rounded once to T: torch's arithmetic for F.silu(g) * u on 16-bit tensors. One Llama-style FFN
 *   block = this launch over [gate; up], then a plain consuming launch over the down shard (K = F = world x ns / 2).
 *   wg_limit: at most that many workgroups (0 = one per CU) - ranks that share ONE device must be co-resident.
 *   epoch_word: 4 bytes of ORDINARY device memory owned by this rank, zeroed once (exchanges completed up to the last read-out;
 *   on the device because a replayed hipGraph re-runs its launches; only the read-out advances it).
 *   epoch_offset: exchanges completed (launches with bit 1) since the last bnb_mi355x_peer_chain_read on these buffers.
 * Every rank issues the same sequence of launches; a chain ends with bnb_mi355x_peer_chain_read (epoch_offset = the number of
 * exchanges since the previous read-out, this chain's included) and holds AT LEAST TWO exchanges: an exchange lives in the region
 * of its position in the chain (epoch_offset + 1 of the producing launch, modulo 64), only its tag carries the epoch. Returns 1 when launched, 0 when the problem is outside the form's
 * preconditions (ns even, K % 32 == 0, K <= 16384 with bit 0, one phase, blocksize >= 32, 16-byte aligned B / A, world * ns and
 * K <= max_values) - nothing was launched and the caller takes the unfused path. A wait that runs into its bound
 * (BNB_MI355X_PEER_WAIT_POLLS) sets the buffer's status word (bnb_mi355x_peer_status) and yields NaN, never a hang; once the word
 * is set every later wait on the buffer gives up after a few polls (a dead peer costs the bound once, not once per round and layer).
 * bnb_mi355x_peer_chain_read: the current exchange as a plain [nvalues] tensor (the end of a chain). */
size_t bnb_mi355x_peer_chain_buffer_bytes(long max_values);
void* bnb_mi355x_peer_chain_alloc(size_t bytes, int fine_grained);
int bnb_mi355x_gemv_4bit_peer_serves(int world, int ns, int K, int blocksize, int mode, long max_values, int wg_limit);
int bnb_mi355x_gemv_4bit_peer(void* const* bufs, void* epoch_word, int world, int rank, int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const void* bias, void* out_local, int ns, int K, int blocksize, int quant_type, int mode, long max_values, int wg_limit, int epoch_offset, bnb_stream_t stream);
void bnb_mi355x_peer_chain_read(void* const* bufs, void* epoch_word, int world, int rank, int dtype, void* out, int nvalues, long max_values, int epoch_offset, bnb_stream_t stream);

/* Tuning overrides for sweeps and tests (0 = built-in heuristic). reserved0: encoder of the 8-bit blockwise quantize - 1 =
 * cell-table kernel, 2 = byte-table kernel, anything else = by input size; 3 = the one-tile form of the 4-bit quantize kernel
 * everywhere (A/B of its pipelined FP4 form); 4 / 5 = 4 / 8 chunks per workgroup of the 4-bit quantize kernel instead of the shipped 2
 * (large NF4 inputs); 6 = one unit in flight per lane in the 8-bit dequantize kernel (its first form); 10 + v = tile / lane-mapping
 * variants of the 4-bit dequantize kernel (csrc/dequantize4.hip); reserved1: N slices of the fused backward (> 0; the
 * workspace-size query follows it). MFMA kernels: knob0 bit 0 = round 2's form of the register-transposed kernel (measurement build only; ignored by the product library),
 * knob0 bit 1 = the built-in route without the streaming MFMA kernel (round 5's routing: A/B runs), bit 2 = its weights-first experiment,
 * knob1 = 100 * cfg + K-slice count (cfg 11-14 producer/consumer geometries, 20/21/22
 * register-transposed kernel with built-in / 8 / 16 wavefronts, 40 K-quarter kernel, 50 streaming MFMA kernel). Every setting
 * computes correct results - the knobs only choose a launch geometry. THREAD-LOCAL: a setting applies to the calls the
 * SAME host thread makes afterwards and to nothing else in the process. */
void bnb_mi355x_set_tuning(int reserved0, int reserved1, int mfma_knob0, int mfma_knob1);

/* Sweep-only overrides of the streaming kernel (0 / -1 = built-in choice): ring depth (2, 3, 6; bf16 M = 1 fp32-absmax
 * NF4 only), 2048-k segments side by side, rows per workgroup, non-temporal weight loads (0 / 1, -1 = default on),
 * wavefronts per workgroup (8; same restriction as ring depth). Every setting computes the same results. Thread-local
 * like bnb_mi355x_set_tuning. */
void bnb_mi355x_set_stream_tuning(int ring_depth, int segments, int rows_per_workgroup, int nontemporal, int waves);

/* Which instance of the streaming kernel a single-matrix call of this shape launches under the calling thread's stream tuning:
 * 1 = the exact-geometry instance (M = 1, 16-bit activations, fp32 absmax (nested = 0), K = 4096, rows that divide evenly over
 * workgroups and row groups: csrc/gemv4_stream.hip exact_geometry), 0 = the general one. Host logic only (the launcher's own
 * geometry and rule, no launch). Stream tuning `nontemporal` = 2 forces the general instance, 3 the general instance with the
 * epilogue's pointers loaded late (A/B runs: tools/stream_fixed_cost_ab.py); 4 keeps the selection and runs the instance with the
 * row sum combined through v_readlane (the form before the in-lane sum), 5 does so on the general instance (A/B runs:
 * tools/stream_post_barrier_ab.py; bf16, NF4 fp32 absmax and FP4 nested only). */
int bnb_mi355x_gemv_4bit_stream_exact(int dtype, int M, int N, int K, int blocksize, int nested);

/* Test and tool infrastructure: the launch geometry of a streaming-kernel call (csrc/gemv4_stream.hip), without the call. Host logic
 * only - no device pointer, no HIP call beyond the CU count of the current device (256 without one) -, under the calling thread's
 * stream tuning, computed by the functions the launch itself calls. form: 0 = bnb_mi355x_gemm_4bit (single matrix), 1 = the grouped
 * call (rows = the rows of the whole group), 2 = gated (rows = 2 F), 3 = LoRA, 4 = LoRA with adapter ids. dtype: 0 = fp32, 1 = fp16,
 * 2 = bf16. Returns 0, out8 untouched, where the streaming kernel's own predicates refuse that form of the call (K % 32, K > 511 * 2048,
 * rows * K >= 2^32, fp32 on a fused form, a grouped row of several phases, a gated call whose workgroups cannot hold row pairs ...);
 * it does NOT ask the router - whether bnb_mi355x_gemm_4bit sends the shape to this kernel is bnb_mi355x_gemm_4bit_route's answer.
 * Returns 1 and out8 = {R rows per workgroup, SW segment columns, G row groups, P phases, grid_x workgroups, dynamic LDS bytes,
 * mb activation rows per pass, waves wavefronts per workgroup}. */
int bnb_mi355x_stream_geometry(int form, int dtype, int M, long rows, int K, int blocksize, int* out8);

/* CU-count override for tests and tools (0 = ask the device, the default): every launch plan the calling thread makes afterwards -
 * rows per workgroup, K / N slices, row tiles, wavefronts, the route's "fills the chip" tests, the quantizers' grid caps - is made for a
 * device of `cus` compute units, what a partitioned MI355X presents (DPX / QPX / CPX: 128 / 64 / 32), whatever device runs it; the
 * size and plan queries follow it. Every setting computes correct results - it only chooses a launch geometry. THREAD-LOCAL like
 * bnb_mi355x_set_tuning (autograd's backward thread does not see it); it bypasses the per-device cache of the real count and never
 * writes to it. Negative values count as 0. Not for the peer-chain kernels, whose workgroups wait for one another. */
void bnb_mi355x_set_cu_count(int cus);

/* Test and tool infrastructure: the launch plan of a bnb_mi355x_gemm_4bit call, without the call. Host logic only - no device
 * pointer, no HIP call beyond the CU count of the current device (256 without one; bnb_mi355x_set_cu_count goes first) -, under the
 * calling thread's tuning, computed by the functions the launch itself calls. Aligned pointers and literal code tables are assumed, as
 * in bnb_mi355x_gemm_4bit_route; nested: the call carries double-quantised statistics. Returns 0, out16 untouched, where no plan can be
 * named: a call the streaming kernel's predicates refuse (it runs the generic kernel) or the tall-tile kernel of a tuning knob.
 * Returns 1 and out16 =
 *   [0]  family, as bnb_mi355x_last_gemm_kernel names it (1 streaming, 3 register-transposed, 4 producer/consumer, 6 K-quarter,
 *        7 streaming MFMA)
 *   [1] [2] [3]  grid x, y, z
 *   [4]  K slices (grid y of families 3, 4, 6; 1 otherwise)     [5]  k units per slice     [6]  k units of a row
 *   [7]  row tiles per workgroup (families 3, 4, 6: mt; 7: 16-row tiles of weight rows, tt; 1: activation rows per pass, mb)
 *   [8]  wavefronts per workgroup
 *   [9]  batch rows per step of the grid axis that carries M (y for families 1 and 7, z otherwise)
 *   [10] output columns (weight rows) per workgroup along grid x: R of families 1 and 7
 *   [11] family 7: weight rows the instance's tiles hold (16 x tiles); family 6: floats / 1024 of one slice's workspace slab;
 *        family 1: segment columns SW; else 0
 *   [12] dynamic LDS bytes
 *   [13] k per unit (family 1: 2048, [5] = phases P, [6] = segments)
 *   [14] family 7: rows instance (4, 8, 16, 32); 3: direct activation fragments (0 / 1); 4: ring depth; 1: row groups G
 *   [15] family 7: single-item instance (0 / 1); 4: cfg; else 0 */
int bnb_mi355x_gemm_4bit_plan(int kernel, int dtype, int M, int N, int K, int blocksize, int nested, int* out16);

/* ... of the streaming MFMA kernel's fused forms and grouped launch (the streaming kernel's: bnb_mi355x_stream_geometry). form:
 * 1 = gated (N = 2 F), 2 = LoRA, 3 = LoRA with adapter ids: 0 where bnb_mi355x_gemm_4bit_gated / _lora on this shape does not run the
 * streaming MFMA kernel. form 4 = grouped: N points to `count` (= the `N` argument) row counts on the host, 0 where
 * bnb_mi355x_gemm_4bit_grouped_route does not answer 2; out16[1] = the workgroups of all members, out16[10] = the rows of each. */
int bnb_mi355x_gemm_4bit_sm_form_plan(int form, int dtype, int M, int N, const int* group_N, int K, int blocksize, int nested, int* out16);

/* ... of bnb_mi355x_gemm_4bit_grad_input: out16 as above with [0] = 0, grid x = K / 128, [4] N slices (grid y), [5] 32-n blocks per
 * slice, [6] blocks of a column, [7] row tiles, [10] = 128 k-columns per workgroup. 0 outside bnb_mi355x_gemm_4bit_grad_input_supported. */
int bnb_mi355x_gemm_4bit_grad_input_plan(int dtype, int M, int N, int K, int blocksize, int* out16);

/* Profiling builds only (libbitsandbytes_mi355x_prof.so, -DBNB_PROFILING): when non-NULL the kernels write s_memtime
 * stamps per wavefront (u64) into this device buffer (tools/timeline_*.py). The product library contains no stamp or
 * ablation code; there the call is accepted and ignored. */
void bnb_mi355x_set_stamp_buffer(void* device_u64_buffer);

/* Version / build identification: returns "bitsandbytes_amd <ver> gfx950". */
const char* bnb_mi355x_version(void);

#ifdef __cplusplus
}
#endif

#endif /* BNB_MI355X_H */
