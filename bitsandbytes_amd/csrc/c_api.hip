// c_api.hip — the extern "C" surface of libbitsandbytes_mi355x.so (declared in include/bnb_mi355x.h).
// Thin, un-mangled wrappers over the launchers of the other files (declared in bnb_launchers.h). Mirrors the symbol set the
// reference exports for this path from csrc/pythonInterface.cpp:343-841 and csrc/gemm_4bit.cu:136-168.
#include "bnb_launchers.h"

#include "../../include/bnb_mi355x.h"

namespace bnb {
thread_local int g_last_gemm_kernel = kKernelNone;
#ifdef BNB_PROFILING
unsigned long long* g_dbg_buf = nullptr; // profiling builds only: device buffer for the kernels' s_memtime stamps
#endif

namespace {

// Error convention of the reference ABI (bnb_common.h): an entry point that cannot serve its call prints and terminates.
void require_quant_type(const char* entry, int quant_type) {
    if (quant_type != kFP4 && quant_type != kNF4) {
        fprintf(stderr, "bitsandbytes_amd: %s: quant_type must be 1 (FP4) or 2 (NF4), got %d\n", entry, quant_type);
        exit(1);
    }
}

void gemm_4bit_dispatch(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax,
                        const uint8_t* absmax8, const float* absmax_code, const float* absmax_offset,
                        const float* code16, void* out, const void* bias, int M, int N, int K, int blocksize,
                        int quant_type, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (M <= 0 || N <= 0)
        return;
    require_quant_type("gemm_4bit", quant_type);
    gemm_4bit(kernel, dtype, A, B, absmax, absmax8, absmax_code, absmax_offset, code16, out, bias, M, N, K, blocksize, quant_type, workspace,
              workspace_bytes, stream);
}

} // namespace
} // namespace bnb

using namespace bnb;

static inline hipStream_t S(bnb_stream_t s) { return static_cast<hipStream_t>(s); }

extern "C" {
// the library is built with -fvisibility=hidden: the C ABI declared in include/bnb_mi355x.h is ALL it exports
#pragma GCC visibility push(default)

// ------------------------------------------------------------------ 4-bit quantize (NULL stream, like the reference)
void cquantize_blockwise_fp32_nf4(float*, float* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_4bit_f32(A, absmax, out, bs, n, kNF4, nullptr);
}
void cquantize_blockwise_fp32_fp4(float*, float* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_4bit_f32(A, absmax, out, bs, n, kFP4, nullptr);
}
void cquantize_blockwise_fp16_nf4(float*, void* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_4bit_f16(A, absmax, out, bs, n, kNF4, nullptr);
}
void cquantize_blockwise_fp16_fp4(float*, void* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_4bit_f16(A, absmax, out, bs, n, kFP4, nullptr);
}
void cquantize_blockwise_bf16_nf4(float*, void* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_4bit_bf16(A, absmax, out, bs, n, kNF4, nullptr);
}
void cquantize_blockwise_bf16_fp4(float*, void* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_4bit_bf16(A, absmax, out, bs, n, kFP4, nullptr);
}

// ------------------------------------------------------------------ 4-bit dequantize
void cdequantize_blockwise_fp32_nf4(float*, unsigned char* A, float* absmax, float* out, int bs, const int n,
                                    bnb_stream_t s) {
    dequantize_4bit_f32(A, absmax, out, bs, n, kNF4, S(s));
}
void cdequantize_blockwise_fp32_fp4(float*, unsigned char* A, float* absmax, float* out, int bs, const int n,
                                    bnb_stream_t s) {
    dequantize_4bit_f32(A, absmax, out, bs, n, kFP4, S(s));
}
void cdequantize_blockwise_fp16_nf4(float*, unsigned char* A, float* absmax, void* out, int bs, const int n,
                                    bnb_stream_t s) {
    dequantize_4bit_f16(A, absmax, out, bs, n, kNF4, S(s));
}
void cdequantize_blockwise_fp16_fp4(float*, unsigned char* A, float* absmax, void* out, int bs, const int n,
                                    bnb_stream_t s) {
    dequantize_4bit_f16(A, absmax, out, bs, n, kFP4, S(s));
}
void cdequantize_blockwise_bf16_nf4(float*, unsigned char* A, float* absmax, void* out, int bs, const int n,
                                    bnb_stream_t s) {
    dequantize_4bit_bf16(A, absmax, out, bs, n, kNF4, S(s));
}
void cdequantize_blockwise_bf16_fp4(float*, unsigned char* A, float* absmax, void* out, int bs, const int n,
                                    bnb_stream_t s) {
    dequantize_4bit_bf16(A, absmax, out, bs, n, kFP4, S(s));
}

// ------------------------------------------------------------------ 8-bit blockwise (double-quant helper)
void cquantize_blockwise_fp32(float* code, float* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_8bit_f32(code, A, absmax, out, bs, n, nullptr);
}
void cquantize_blockwise_fp16(float* code, void* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_8bit_f16(code, A, absmax, out, bs, n, nullptr);
}
void cquantize_blockwise_bf16(float* code, void* A, float* absmax, unsigned char* out, int bs, const int n) {
    quantize_8bit_bf16(code, A, absmax, out, bs, n, nullptr);
}
void cdequantize_blockwise_fp32(float* code, unsigned char* A, float* absmax, float* out, int bs, const int n,
                                bnb_stream_t s) {
    dequantize_8bit_f32(code, A, absmax, out, bs, n, S(s));
}
void cdequantize_blockwise_fp16(float* code, unsigned char* A, float* absmax, void* out, int bs, const int n,
                                bnb_stream_t s) {
    dequantize_8bit_f16(code, A, absmax, out, bs, n, S(s));
}
void cdequantize_blockwise_bf16(float* code, unsigned char* A, float* absmax, void* out, int bs, const int n,
                                bnb_stream_t s) {
    dequantize_8bit_bf16(code, A, absmax, out, bs, n, S(s));
}

// ------------------------------------------------------------------ fused dequant + GEMM
void cgemm_4bit_bf16(const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit,
                     const float* absmax_code, const float* absmax_offset, void* out, const void* bias, int M, int N,
                     int K, int blocksize, int quant_type, bnb_stream_t s) {
    gemm_4bit_dispatch(0, 2, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, nullptr, out, bias, M, N, K,
                       blocksize, quant_type, nullptr, 0, S(s));
}
void cgemm_4bit_fp16(const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit,
                     const float* absmax_code, const float* absmax_offset, void* out, const void* bias, int M, int N,
                     int K, int blocksize, int quant_type, bnb_stream_t s) {
    gemm_4bit_dispatch(0, 1, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, nullptr, out, bias, M, N, K,
                       blocksize, quant_type, nullptr, 0, S(s));
}
void cgemm_4bit_fp32(const float* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit,
                     const float* absmax_code, const float* absmax_offset, float* out, const float* bias, int M, int N,
                     int K, int blocksize, int quant_type, bnb_stream_t s) {
    gemm_4bit_dispatch(0, 0, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, nullptr, out, bias, M, N, K,
                       blocksize, quant_type, nullptr, 0, S(s));
}

// ------------------------------------------------------------------ legacy gemv (m = N, n = 1, k = K)
void cgemm_4bit_inference_naive_fp16(int m, int n, int k, void* A, unsigned char* B, float* absmax, float* datatype,
                                     void* out, int, int, int, int blocksize, bnb_stream_t s) {
    (void)n;
    gemv_4bit_stream(1, A, B, absmax, nullptr, nullptr, nullptr, datatype, out, nullptr, 1, m, k, blocksize, kNF4, S(s));
}
void cgemm_4bit_inference_naive_bf16(int m, int n, int k, void* A, unsigned char* B, float* absmax, float* datatype,
                                     void* out, int, int, int, int blocksize, bnb_stream_t s) {
    (void)n;
    gemv_4bit_stream(2, A, B, absmax, nullptr, nullptr, nullptr, datatype, out, nullptr, 1, m, k, blocksize, kNF4, S(s));
}
void cgemm_4bit_inference_naive_fp32(int m, int n, int k, float* A, unsigned char* B, float* absmax, float* datatype,
                                     float* out, int, int, int, int blocksize, bnb_stream_t s) {
    (void)n;
    gemv_4bit_stream(0, A, B, absmax, nullptr, nullptr, nullptr, datatype, out, nullptr, 1, m, k, blocksize, kNF4, S(s));
}

// ------------------------------------------------------------------ loader symbols
void* get_context(void) {
    static int token = 0x4d493335; // opaque: this path needs no BLAS handle
    return &token;
}
void* cget_managed_ptr(size_t bytes) {
    void* ptr = nullptr;
    BNB_HIP_CHECK(hipMallocManaged(&ptr, bytes, hipMemAttachHost));
    return ptr;
}

// ------------------------------------------------------------------ extensions
void bnb_mi355x_quantize_4bit(const void* A, int dtype, float* absmax, unsigned char* out, int blocksize, long n,
                              int quant_type, bnb_stream_t s) {
    require_quant_type("quantize_4bit", quant_type);
    if (dtype == 0)
        quantize_4bit_f32(static_cast<const float*>(A), absmax, out, blocksize, n, quant_type, S(s));
    else if (dtype == 1)
        quantize_4bit_f16(A, absmax, out, blocksize, n, quant_type, S(s));
    else
        quantize_4bit_bf16(A, absmax, out, blocksize, n, quant_type, S(s));
}
void bnb_mi355x_dequantize_4bit_rows(int dtype, const unsigned char* A, const float* absmax, const void* indices,
                                     int index_bytes, void* out, long rows_out, long num_rows, int row_len,
                                     int blocksize, int quant_type, bnb_stream_t s) {
    dequantize_4bit_rows(dtype, A, absmax, indices, index_bytes, out, rows_out, num_rows, row_len, blocksize,
                         quant_type, S(s));
}
void bnb_mi355x_dequantize_4bit_nested(int dtype, const unsigned char* A, const unsigned char* absmax_8bit, const float* absmax2,
                                       const float* absmax_code, const float* absmax_offset, void* out, int blocksize, long n,
                                       int quant_type, bnb_stream_t s) {
    require_quant_type("dequantize_4bit_nested", quant_type);
    dequantize_4bit_nested(dtype, A, absmax_8bit, absmax2, absmax_code, absmax_offset, out, blocksize, n, quant_type, S(s));
}
void bnb_mi355x_quantize_8bit(const float* code, const void* A, int dtype, float* absmax, unsigned char* out,
                              int blocksize, long n, bnb_stream_t s) {
    if (dtype == 0)
        quantize_8bit_f32(code, static_cast<const float*>(A), absmax, out, blocksize, n, S(s));
    else if (dtype == 1)
        quantize_8bit_f16(code, A, absmax, out, blocksize, n, S(s));
    else
        quantize_8bit_bf16(code, A, absmax, out, blocksize, n, S(s));
}
void bnb_mi355x_quantize_4bit_nested(const void* A, int dtype, long n, int blocksize, int quant_type, unsigned char* out,
                                     float* scratch, const float* code8, unsigned char* absmax_8bit, float* absmax2,
                                     float* offset, bnb_stream_t s) {
    // quantize_4bit(compress_statistics=True) of the reference (bitsandbytes/functional.py:925-951) as ONE call: the 4-bit encoder
    // into scratch[0, blocks), then the statistics (mean, subtract, 8-bit encode in blocks of 256) in two launches
    bnb_mi355x_quantize_4bit(A, dtype, scratch, out, blocksize, n, quant_type, s);
    const long blocks = (n + blocksize - 1) / blocksize;
    quantize_absmax_nested(code8, scratch, blocks, scratch + blocks, offset, absmax_8bit, absmax2, S(s));
}
void bnb_mi355x_gemm_4bit(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax,
                          const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset,
                          const float* code16, void* out, const void* bias, int M, int N, int K, int blocksize,
                          int quant_type, void* workspace, size_t workspace_bytes, bnb_stream_t s) {
    gemm_4bit_dispatch(kernel, dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, code16, out, bias, M, N, K,
                       blocksize, quant_type, workspace, workspace_bytes, S(s));
}
void bnb_mi355x_gemm_4bit_grouped(int dtype, const void* A, int count, const uint8_t* const* B, const float* const* absmax,
                                  const uint8_t* const* absmax_8bit, const float* const* absmax_code,
                                  const float* const* absmax_offset, void* const* out, const void* const* bias, const int* N,
                                  int M, int K, int blocksize, int quant_type, bnb_stream_t s) {
    if (count <= 0 || M <= 0)
        return;
    require_quant_type("gemm_4bit_grouped", quant_type);
    const int route = gemm_4bit_grouped_route(dtype, A, count, B, absmax, absmax_8bit, N, M, K, blocksize);
    if (route == 2 && gemm_4bit_sm_grouped(dtype, A, count, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, N, M, K, blocksize, quant_type, S(s)))
        return;
    if (route == 1 && gemv_4bit_grouped(dtype, A, count, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, N, M, K, blocksize, quant_type, S(s)))
        return;
    // (gemm_4bit_grouped_route has the three cases) matrix by matrix - also a group that its launcher refused: same results
    for (int i = 0; i < count; ++i)
        gemm_4bit_dispatch(0, dtype, A, B[i], absmax[i], absmax_8bit ? absmax_8bit[i] : nullptr,
                           absmax_code ? absmax_code[i] : nullptr, absmax_offset ? absmax_offset[i] : nullptr, nullptr, out[i],
                           bias ? bias[i] : nullptr, M, N[i], K, blocksize, quant_type, nullptr, 0, S(s));
}
int bnb_mi355x_gemm_4bit_grouped_route(int dtype, int count, const int* N, int M, int K, int blocksize) {
    // what bnb_mi355x_gemm_4bit_grouped does with such a group, assuming aligned pointers and members of plain statistics
    const uint8_t* B[8];
    const float* absmax[8];
    for (int i = 0; i < 8; ++i) {
        B[i] = kAlignedDummy8;
        absmax[i] = reinterpret_cast<const float*>(kAlignedDummy);
    }
    return gemm_4bit_grouped_route(dtype, kAlignedDummy, count, B, absmax, nullptr, N, M, K, blocksize);
}
size_t bnb_mi355x_gemm_4bit_workspace_bytes(int kernel, int dtype, int M, int N, int K, int blocksize) {
    // alignment of A/B is unknown here; assume the aligned (fast) case, an unused workspace is harmless
    return gemm_4bit_workspace_bytes(kernel, dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), M, N, K, blocksize);
}
int bnb_mi355x_last_gemm_kernel(void) { return g_last_gemm_kernel; }

// ------------------------------------------------------------------ expert-indexed gemm_4bit (MoE decode)
void bnb_mi355x_gemm_4bit_experts(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax,
                                  const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const void* bias,
                                  const void* ids, int index_bytes, void* out, long P, int slots, int E, int N, int K, int blocksize,
                                  int quant_type, bnb_stream_t s) {
    gemm_4bit_experts(dtype, A, a_slot_stride, B, absmax, absmax_8bit, absmax_code, absmax_offset, bias, ids, index_bytes, out, P, slots,
                      E, N, K, blocksize, quant_type, S(s));
}
int bnb_mi355x_gemm_4bit_experts_supported(int dtype, int E, int N, int K, int blocksize) {
    return gemm_4bit_experts_supported(dtype, E, N, K, blocksize) ? 1 : 0;
}
void bnb_mi355x_gemm_4bit_experts_ffn(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax,
                                      const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const void* bias,
                                      const void* ids, int index_bytes, const void* row_scale, int row_scale_dtype, int gated, void* out,
                                      long P, int slots, int E, int N, int K, int blocksize, int quant_type, bnb_stream_t s) {
    gemm_4bit_experts_ffn(dtype, A, a_slot_stride, B, absmax, absmax_8bit, absmax_code, absmax_offset, bias, ids, index_bytes, row_scale,
                          row_scale_dtype, gated, out, P, slots, E, N, K, blocksize, quant_type, S(s));
}
int bnb_mi355x_gemm_4bit_experts_ffn_supported(int dtype, int E, int N, int K, int blocksize, int gated) {
    return gemm_4bit_experts_ffn_supported(dtype, E, N, K, blocksize, gated) ? 1 : 0;
}

// ------------------------------------------------------------------ gated gemm_4bit (dense FFN: silu(gate) * up as the epilogue)
void bnb_mi355x_gemm_4bit_gated(int dtype, const void* A, const uint8_t* B, const float* absmax, void* out, const void* bias, int M, int N,
                                int K, int blocksize, int quant_type, bnb_stream_t s) {
    require_quant_type("gemm_4bit_gated", quant_type);
    const int family = gemm_4bit_gated_family(dtype, A, B, absmax, M, N, K, blocksize);
    const bool ok = family == kKernelSm       ? gemm_4bit_sm_gated(dtype, A, B, absmax, out, bias, M, N, K, blocksize, quant_type, S(s))
                    : family == kKernelStream ? gemv_4bit_stream_gated(dtype, A, B, absmax, out, bias, M, N, K, blocksize, quant_type, S(s))
                                              : false;
    if (!ok) {
        fprintf(stderr, "bitsandbytes_amd: gemm_4bit_gated: no kernel for dtype %d, M=%d, N=%d, K=%d, blocksize=%d (ask bnb_mi355x_gemm_4bit_gated_supported, align A / B to 16 bytes)\n",
                dtype, M, N, K, blocksize);
        exit(1);
    }
}
int bnb_mi355x_gemm_4bit_gated_supported(int dtype, int M, int N, int K, int blocksize) {
    // (alignment of A / B / absmax is unknown here; the aligned case is assumed, as in the route query)
    return gemm_4bit_gated_family(dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), M, N, K, blocksize) != kKernelNone ? 1 : 0;
}

// ------------------------------------------------------------------ LoRA gemm_4bit (the adapter term as the decode kernels' epilogue)
void bnb_mi355x_gemm_4bit_lora(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit,
                               const float* absmax_code, const float* absmax_offset, void* out, const void* bias, const void* lora_t,
                               const void* lora_b, float scaling, int r, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t s) {
    require_quant_type("gemm_4bit_lora", quant_type);
    const int family = gemm_4bit_lora_family(dtype, A, B, absmax, absmax_8bit, lora_t, lora_b, M, N, K, blocksize, r);
    const bool ok = family == kKernelSm ? gemm_4bit_sm_lora(dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, lora_t, lora_b, scaling, r,
                                                            M, N, K, blocksize, quant_type, S(s))
                    : family == kKernelStream ? gemv_4bit_stream_lora(dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, lora_t, lora_b,
                                                                      scaling, r, M, N, K, blocksize, quant_type, S(s))
                                              : false;
    if (!ok) {
        fprintf(stderr, "bitsandbytes_amd: gemm_4bit_lora: no kernel for dtype %d, M=%d, N=%d, K=%d, blocksize=%d, r=%d (ask bnb_mi355x_gemm_4bit_lora_supported, align A / B / lora_t / lora_b to 16 bytes)\n",
                dtype, M, N, K, blocksize, r);
        exit(1);
    }
}
int bnb_mi355x_gemm_4bit_lora_supported(int dtype, int M, int N, int K, int blocksize, int nested, int r) {
    // (alignment is unknown here; the aligned case is assumed, as in the route query)
    return gemm_4bit_lora_family(dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), nested ? kAlignedDummy8 : nullptr, kAlignedDummy,
                       kAlignedDummy, M, N, K, blocksize, r) != kKernelNone
               ? 1
               : 0;
}

// (mixed-adapter form: lora_b [A_n, N, r], scalings [A_n] fp32 and one adapter id per row on the device; the uniform call's family)
void bnb_mi355x_gemm_4bit_lora_ids(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit,
                                   const float* absmax_code, const float* absmax_offset, void* out, const void* bias, const void* lora_t,
                                   const void* lora_b, const float* scalings, const void* ids, int index_bytes, int A_n, int r, int M, int N, int K,
                                   int blocksize, int quant_type, bnb_stream_t s) {
    require_quant_type("gemm_4bit_lora_ids", quant_type);
    const int family = gemm_4bit_lora_family(dtype, A, B, absmax, absmax_8bit, lora_t, lora_b, M, N, K, blocksize, r);
    const bool ok = family == kKernelSm ? gemm_4bit_sm_lora_ids(dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, lora_t, lora_b,
                                                                scalings, ids, index_bytes, A_n, r, M, N, K, blocksize, quant_type, S(s))
                    : family == kKernelStream ? gemv_4bit_stream_lora_ids(dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, lora_t,
                                                                          lora_b, scalings, ids, index_bytes, A_n, r, M, N, K, blocksize, quant_type, S(s))
                                              : false;
    if (!ok) {
        fprintf(stderr, "bitsandbytes_amd: gemm_4bit_lora_ids: no kernel for dtype %d, M=%d, N=%d, K=%d, blocksize=%d, r=%d, A_n=%d, index_bytes=%d (ask bnb_mi355x_gemm_4bit_lora_ids_supported, align A / B / lora_t / lora_b to 16 bytes)\n",
                dtype, M, N, K, blocksize, r, A_n, index_bytes);
        exit(1);
    }
}
int bnb_mi355x_gemm_4bit_lora_ids_supported(int dtype, int M, int N, int K, int blocksize, int nested, int r, int A_n) {
    // (exactly where the uniform launch is served, for every stack of 1 ... 64 adapters: the streaming MFMA kernel rebases lora_b per
    // adapter, so there is no bound on A_n N r)
    return A_n >= 1 && A_n <= 64 ? bnb_mi355x_gemm_4bit_lora_supported(dtype, M, N, K, blocksize, nested, r) : 0;
}

// ------------------------------------------------------------------ LoRA shrink (t = x lora_A^T, the launch in front of gemm_4bit_lora)
void bnb_mi355x_lora_shrink(int dtype, const void* x, const void* lora_a, void* t, int M, int R, int K, const int* splits, int n_splits, bnb_stream_t s) {
    if (!lora_shrink(dtype, x, lora_a, t, M, R, K, splits, n_splits, S(s))) {
        fprintf(stderr, "bitsandbytes_amd: lora_shrink: no kernel for dtype %d, M=%d, R=%d, K=%d, n_splits=%d (fp16 / bf16, 1 <= M <= 16, K %% 64 == 0, R %% 8 == 0, 8 <= R <= 1024, up to 8 splits of 8 ... 128 rows, each a multiple of 8, that sum to R; x / lora_a / t 16-byte aligned)\n",
                dtype, M, R, K, n_splits);
        exit(1);
    }
}
int bnb_mi355x_lora_shrink_supported(int dtype, int M, int R, int K) { return lora_shrink_supported(dtype, M, R, K) ? 1 : 0; }
// (mixed-adapter form: lora_a [A_n, R, K], one adapter id per row of x on the device)
void bnb_mi355x_lora_shrink_ids(int dtype, const void* x, const void* lora_a, const void* ids, int index_bytes, void* t, int M, int A_n, int R, int K,
                                const int* splits, int n_splits, bnb_stream_t s) {
    if (!lora_shrink_ids(dtype, x, lora_a, ids, index_bytes, t, M, A_n, R, K, splits, n_splits, S(s))) {
        fprintf(stderr, "bitsandbytes_amd: lora_shrink_ids: no kernel for dtype %d, M=%d, A_n=%d, R=%d, K=%d, index_bytes=%d, n_splits=%d (fp16 / bf16, 1 <= M <= 16, 1 <= A_n <= 64, K %% 64 == 0, R %% 8 == 0, 8 <= R <= 1024, ids int32 / int64, up to 8 splits of 8 ... 128 rows, each a multiple of 8, that sum to R; x / lora_a / t 16-byte aligned)\n",
                dtype, M, A_n, R, K, index_bytes, n_splits);
        exit(1);
    }
}
int bnb_mi355x_lora_shrink_ids_supported(int dtype, int M, int A_n, int R, int K) { return lora_shrink_ids_supported(dtype, M, A_n, R, K) ? 1 : 0; }

// ------------------------------------------------------------------ MoE router: scoring + top-k (the launch in front of gemm_4bit_experts)
// Takes an argument block and REFUSES (message, non-zero, nothing launched) instead of ending the process.
int bnb_mi355x_moe_topk(const bnb_mi355x_moe_topk_args* args) {
    if (args == nullptr || args->struct_bytes != sizeof(bnb_mi355x_moe_topk_args)) {
        fprintf(stderr, "bitsandbytes_amd: moe_topk: struct_bytes is %zu, this library's bnb_mi355x_moe_topk_args has %zu\n",
                args == nullptr ? static_cast<size_t>(0) : args->struct_bytes, sizeof(bnb_mi355x_moe_topk_args));
        return 1;
    }
    const MoeTopkCall call = {args->logits_dtype, args->scoring, args->renormalize != 0 ? 1 : 0, args->rows, args->experts, args->top_k,
                              args->scale,        args->logits,  args->select_bias,              args->ids,  args->weights};
    if (!moe_topk(call, S(args->stream))) {
        fprintf(stderr, "bitsandbytes_amd: moe_topk: no kernel for logits_dtype %d, scoring %d, rows=%d, experts=%d, top_k=%d (fp32 / fp16 / bf16 logits, scoring 0 / 1, rows >= 0, 1 <= experts <= 1024, 1 <= top_k <= min(experts, 16); logits / ids / weights not NULL; every pointer aligned to its element)\n",
                args->logits_dtype, args->scoring, args->rows, args->experts, args->top_k);
        return 1;
    }
    return 0;
}
int bnb_mi355x_moe_topk_supported(int logits_dtype, int rows, int experts, int top_k) {
    return moe_topk_supported(logits_dtype, rows, experts, top_k) ? 1 : 0;
}
// (group-limited routing: the same conventions, a block of its own)
int bnb_mi355x_moe_topk_grouped(const bnb_mi355x_moe_topk_grouped_args* args) {
    if (args == nullptr || args->struct_bytes != sizeof(bnb_mi355x_moe_topk_grouped_args)) {
        fprintf(stderr, "bitsandbytes_amd: moe_topk_grouped: struct_bytes is %zu, this library's bnb_mi355x_moe_topk_grouped_args has %zu\n",
                args == nullptr ? static_cast<size_t>(0) : args->struct_bytes, sizeof(bnb_mi355x_moe_topk_grouped_args));
        return 1;
    }
    const MoeTopkGroupedCall call = {{args->logits_dtype, args->scoring, args->renormalize != 0 ? 1 : 0, args->rows, args->experts, args->top_k,
                                      args->scale, args->logits, args->select_bias, args->ids, args->weights},
                                     args->n_group, args->topk_group, args->group_score};
    if (!moe_topk_grouped(call, S(args->stream))) {
        fprintf(stderr, "bitsandbytes_amd: moe_topk_grouped: no kernel for logits_dtype %d, scoring %d, rows=%d, experts=%d, top_k=%d, n_group=%d, topk_group=%d, group_score=%d (fp32 / fp16 / bf16 logits, scoring 0 / 1, rows >= 0, 1 <= experts <= 1024, experts %% n_group == 0, 1 <= topk_group <= n_group <= 64, group_score 0 (max) / 1 (top2sum: experts / n_group >= 2), 1 <= top_k <= min(topk_group * experts / n_group, 16); logits / ids / weights not NULL; every pointer aligned to its element)\n",
                args->logits_dtype, args->scoring, args->rows, args->experts, args->top_k, args->n_group, args->topk_group, args->group_score);
        return 1;
    }
    return 0;
}
int bnb_mi355x_moe_topk_grouped_supported(int logits_dtype, int rows, int experts, int top_k, int n_group, int topk_group, int group_score) {
    return moe_topk_grouped_supported(logits_dtype, rows, experts, top_k, n_group, topk_group, group_score) ? 1 : 0;
}

// ------------------------------------------------------------------ peer chain (the all-gather fused into the gemv launches)
static uint32_t peer_chain_spin_bound() {
    // a re-fetch is s_sleep 4 (256 cycles) + a system-scope load round trip: ~1 us. BNB_MI355X_PEER_WAIT_POLLS as in peer_gather.hip
    static const uint32_t bound = [] {
        const char* e = getenv("BNB_MI355X_PEER_WAIT_POLLS");
        const long long v = e ? atoll(e) : 0;
        return static_cast<uint32_t>(v > 0 && v < 4000000000LL ? v : 30000000LL);
    }();
    return bound;
}
size_t bnb_mi355x_peer_chain_buffer_bytes(long max_values) {
    // header + 64 regions (gemv4_stream.hip: kChainRegions) of max_values / 2 granules of 8 bytes; max_values counts in fours
    // (an even number of granules per region: every region starts 16-byte aligned, which the two-granule stores and fetches need)
    const size_t mv = max_values > 0 ? (static_cast<size_t>(max_values) + 3) & ~static_cast<size_t>(3) : 0;
    return 256 + 64 * 4 * mv;
}
void* bnb_mi355x_peer_chain_alloc(size_t bytes, int fine_grained) {
    // Zeroed device memory for a rank's exchange buffer; exported / mapped / freed with the bnb_mi355x_peer_* functions.
    //   fine_grained != 0: hipDeviceMallocFinegrained - what a chain whose ranks sit on DIFFERENT devices must use. Remote GPUs store
    //     into this buffer while a kernel of the owner polls it; HIP makes coarse-grained memory coherent across devices at kernel
    //     boundaries only, so a line of an ordinary allocation that the owner's L2 holds may never show the remote store.
    //   fine_grained == 0: ordinary (cacheable) hipMalloc memory - enough where every rank runs on ONE device (processes sharing a
    //     GPU, a group of one rank): one L2 hierarchy, nothing crosses a link (profiles/r4_peer_chain.txt, builds 3 and 6).
    void* p = nullptr;
    const hipError_t err = fine_grained ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) : hipMalloc(&p, bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return nullptr;
    }
    return p;
}
int bnb_mi355x_gemv_4bit_peer_serves(int world, int ns, int K, int blocksize, int mode, long max_values, int wg_limit) {
    // the launcher's own shape check (launch geometry included), without launching: 1 = bnb_mi355x_gemv_4bit_peer would accept
    // these shapes (given 16-byte aligned B / A, a valid rank and dtype). Needs the current device (CU count).
    return gemv_4bit_peer_serves(world, ns, K, blocksize, mode, max_values, wg_limit) ? 1 : 0;
}
int bnb_mi355x_gemv_4bit_peer(void* const* bufs, void* epoch_word, int world, int rank, int dtype, const void* A, const uint8_t* B, const float* absmax,
                              const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, const void* bias,
                              void* out_local, int ns, int K, int blocksize, int quant_type, int mode, long max_values, int wg_limit,
                              int epoch_offset, bnb_stream_t s) {
    require_quant_type("gemv_4bit_peer", quant_type);
    return gemv_4bit_peer(bufs, epoch_word, world, rank, dtype, A, B, absmax, absmax_8bit, absmax_code, absmax_offset, bias, out_local, ns, K,
                          blocksize, quant_type, mode, max_values, wg_limit, static_cast<uint32_t>(epoch_offset), peer_chain_spin_bound(), S(s))
               ? 1
               : 0;
}
void bnb_mi355x_peer_chain_read(void* const* bufs, void* epoch_word, int world, int rank, int dtype, void* out, int nvalues, long max_values, int epoch_offset,
                                bnb_stream_t s) {
    if (epoch_word == nullptr || world < 1 || world > 8 || rank < 0 || rank >= world || (dtype != 1 && dtype != 2) || nvalues < 2 || (nvalues & 1) || nvalues > max_values) {
        fprintf(stderr, "bitsandbytes_amd: peer_chain_read: bad arguments (world %d, rank %d, dtype %d, %d values of %ld)\n", world, rank, dtype,
                nvalues, max_values);
        exit(1);
    }
    peer_chain_read(bufs, epoch_word, world, rank, dtype, out, nvalues, max_values, static_cast<uint32_t>(epoch_offset), peer_chain_spin_bound(), S(s));
}
int bnb_mi355x_gemm_4bit_route(int kernel, int dtype, int M, int N, int K, int blocksize) {
    // (alignment of A / B is unknown here; the aligned - fast - case is assumed, as in the workspace query)
    return gemm_4bit_route(kernel, dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), nullptr, nullptr, M, N, K, blocksize).kernel != kKernelStream ? 1 : 0;
}
void bnb_mi355x_gemm_4bit_grad_input(int dtype, const void* grad_out, const uint8_t* B, const float* absmax,
                                     const uint8_t* absmax_8bit, const float* absmax_code, const float* absmax_offset, void* grad_A,
                                     int M, int N, int K, int blocksize, int quant_type, void* workspace, size_t workspace_bytes,
                                     bnb_stream_t s) {
    require_quant_type("gemm_4bit_grad_input", quant_type);
    gemm_4bit_grad_input(dtype, grad_out, B, absmax, absmax_8bit, absmax_code, absmax_offset, grad_A, M, N, K, blocksize,
                         quant_type, workspace, workspace_bytes, S(s));
}
size_t bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(int M, int N, int K) { return gemm_4bit_grad_input_workspace_bytes(M, N, K); }
int bnb_mi355x_gemm_4bit_grad_input_supported(int dtype, int M, int N, int K, int blocksize) {
    return gemm_4bit_grad_input_supported(dtype, kAlignedDummy, kAlignedDummy8, M, N, K, blocksize) ? 1 : 0;
}
void bnb_mi355x_set_tuning(int reserved0, int reserved1, int mfma_knob0, int mfma_knob1) {
    quantize_8bit_set_variant(reserved0); // 1 / 2: force the cell-table / byte-table 8-bit encoder, anything else: by size
    // 3: the one-tile form of the 4-bit quantize kernel everywhere (A/B of the pipelined FP4 form); 4 / 5: round 4's 4 chunks / 8 chunks per
    // workgroup instead of the shipped 2 on large NF4 inputs (A/B, round 5)
    quantize_4bit_set_variant(reserved0 == 3 ? 1 : reserved0 == 4 ? 4 : reserved0 == 5 ? 3 : reserved0 == 8 ? 2 : 0); // (8: 2 chunks forced, FP4 included)
    dequantize_4bit_set_variant(reserved0 >= 10 ? reserved0 - 10 : 0); // 10 + v: tile / lane-mapping variants of dequantize4 (dequantize4.hip)
    gemm_4bit_grad_input_set_slices(reserved1); // N slices of the fused backward (sweeps), 0: built-in
    g_mfma_knob0.store(mfma_knob0, std::memory_order_relaxed);
    g_mfma_knob1.store(mfma_knob1, std::memory_order_relaxed);
}
void bnb_mi355x_set_stream_tuning(int ring_depth, int segments, int rows_per_workgroup, int nontemporal, int waves) {
    gemv_4bit_stream_tuning(ring_depth, segments, rows_per_workgroup, nontemporal, waves);
}
int bnb_mi355x_gemv_4bit_stream_exact(int dtype, int M, int N, int K, int blocksize, int nested) {
    return gemv_4bit_stream_exact(dtype, M, N, K, blocksize, nested != 0) ? 1 : 0;
}
int bnb_mi355x_stream_geometry(int form, int dtype, int M, long rows, int K, int blocksize, int* out8) {
    return gemv_4bit_stream_geometry(form, dtype, M, rows, K, blocksize, out8) ? 1 : 0;
}
void bnb_mi355x_set_cu_count(int cus) { g_cu_count_override.store(cus > 0 ? cus : 0, std::memory_order_relaxed); }
int bnb_mi355x_gemm_4bit_plan(int kernel, int dtype, int M, int N, int K, int blocksize, int nested, int* out16) {
    if (out16 == nullptr || M <= 0 || N <= 0 || K <= 0 || blocksize <= 0 || dtype < 0 || dtype > 2)
        return 0;
    // (bnb_mi355x_gemm_4bit's question, with the aligned pointers of the shape-only queries)
    int v[16];
    if (!gemm_4bit_plan_query(kernel, dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), nested ? kAlignedDummy8 : nullptr, M, N, K,
                              blocksize, v))
        return 0;
    for (int i = 0; i < 16; ++i)
        out16[i] = v[i];
    return 1;
}
int bnb_mi355x_gemm_4bit_sm_form_plan(int form, int dtype, int M, int N, const int* group_N, int K, int blocksize, int nested, int* out16) {
    if (out16 == nullptr || form < 1 || form > 4 || M <= 0 || N <= 0 || K <= 0 || blocksize <= 0)
        return 0;
    const float* const absmax = reinterpret_cast<const float*>(kAlignedDummy);
    int v[16];
    bool ok = false;
    if (form == 1)
        ok = !nested && gemm_4bit_gated_family(dtype, kAlignedDummy, kAlignedDummy8, absmax, M, N, K, blocksize) == kKernelSm && gemm_4bit_sm_plan_query(1, M, N, K, 0, v);
    else if (form <= 3)
        ok = gemm_4bit_lora_family(dtype, kAlignedDummy, kAlignedDummy8, absmax, nested ? kAlignedDummy8 : nullptr, kAlignedDummy, kAlignedDummy, M, N, K, blocksize, 8) == kKernelSm &&
             gemm_4bit_sm_plan_query(form, M, N, K, 0, v);
    else
        ok = group_N != nullptr && bnb_mi355x_gemm_4bit_grouped_route(dtype, N, group_N, M, K, blocksize) == 2 && gemm_4bit_sm_grouped_plan_query(N, group_N, M, K, v);
    if (!ok)
        return 0;
    for (int i = 0; i < 16; ++i)
        out16[i] = v[i];
    return 1;
}
int bnb_mi355x_gemm_4bit_grad_input_plan(int dtype, int M, int N, int K, int blocksize, int* out16) {
    int v[16];
    if (out16 == nullptr || !gemm_4bit_grad_input_plan_query(dtype, M, N, K, blocksize, v))
        return 0;
    for (int i = 0; i < 16; ++i)
        out16[i] = v[i];
    return 1;
}
void bnb_mi355x_set_stamp_buffer(void* device_u64_buffer) {
#ifdef BNB_PROFILING
    g_dbg_buf = static_cast<unsigned long long*>(device_u64_buffer);
#else
    (void)device_u64_buffer; // the product library carries no stamp code: the call is accepted and ignored
#endif
}
const char* bnb_mi355x_version(void) { return "bitsandbytes_amd 0.1.1 gfx950"; }

#pragma GCC visibility pop
} // extern "C"
