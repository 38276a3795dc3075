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

// The alignment of A / B / absmax is unknown to the shape-only queries: they assume the aligned (fast) case and pass this.
const int kAlignedDummy[4] __attribute__((aligned(16))) = {0, 0, 0, 0};
const uint8_t* const kAlignedDummy8 = reinterpret_cast<const uint8_t*>(kAlignedDummy);

// Error convention of the reference ABI (bnb_common.h): an entry point that cannot serve its call prints and terminates.
void require_quant_type(const char* entry, int quant_type) {
    if (quant_type != kFP4 && quant_type != kNF4) {
        fprintf(stderr, "bitsandbytes_amd: %s: quant_type must be 1 (FP4) or 2 (NF4), got %d\n", entry, quant_type);
        exit(1);
    }
}

// M at or below which the streaming dot kernel is used (its activations live in registers: 32 fp32 per row and
// lane); above it the MFMA kernels (when supported). MI355X-specific replacement for the reference's per-arch
// heuristic (bitsandbytes/backends/cuda/ops.py:814-843), calibrated on gfx950 — see DESIGN.md.
constexpr int kStreamMaxM = 4;

// plain_absmax: the call carries fp32 absmax (not the double-quantised form) - what the MFMA route needs to know at blocksize 32,
// where only the register-transposed kernel's BS32 instances (fp32 absmax) exist; the shape-only queries pass true.
bool route_to_mfma(int kernel, int dtype, const void* A, const uint8_t* B, const float* code16, int M, int N, int K, int blocksize, bool plain_absmax) {
    if (kernel == 1 || kernel == 3)
        return false;
    // the streaming MFMA kernel's own reach: 2 ... 16 rows on matrices of >= 128 rows (csrc/gemm4_mfma.hip: sm_selected has the
    // measured exceptions), any K % 64 == 0 (the other MFMA kernels need whole 256-k chunks) - round 6
    const bool sm = gemm_4bit_sm_routes(dtype, M, N, K, blocksize) && gemm_4bit_sm_supported(dtype, A, B, code16, M, N, K, blocksize);
    if (kernel == 2)
        return sm || gemm_4bit_mfma_supported(dtype, A, B, code16, M, N, K, blocksize, plain_absmax);
    // three or four rows: the streaming kernel's FMA count grows with M while the MFMA kernel's does not - on matrices that
    // fill the chip with 16-column workgroups the MFMA kernel is ahead from M = 3 (4096^2 6.5 vs 6.9 us, 4096 x 11008 10.8 vs
    // 26.7), on small ones the streaming kernel's cheaper launch still wins (1376 x 4096 4.9 vs 5.3)
    // round 6: from TWO rows on wherever the streaming MFMA kernel (gemm4_mfma_sm.hip) serves the shape - one decode for all rows,
    // activations once per CU (4096^2 M = 2: 4.44 vs 4.95 us; profiles/r6_sm_v3_ab_full.txt)
    const bool big = static_cast<long>(N) * K >= (12L << 20);
    return sm || ((M > kStreamMaxM || (M >= 3 && big)) && gemm_4bit_mfma_supported(dtype, A, B, code16, M, N, K, blocksize, plain_absmax));
}

void gemm_4bit_dispatch(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax,
                        const uint8_t* absmax8, const float* absmax_code, const float* absmax_offset,
                        const float* code16, void* out, const void* bias, int M, int N, int K, int blocksize,
                        int quant_type, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (M <= 0 || N <= 0)
        return;
    require_quant_type("gemm_4bit", quant_type);
    if (route_to_mfma(kernel, dtype, A, B, code16, M, N, K, blocksize, absmax8 == nullptr && aligned_to(absmax, 16)))
        gemm_4bit_mfma(dtype, A, B, absmax, absmax8, absmax_code, absmax_offset, code16, out, bias, M, N, K, blocksize,
                       quant_type, workspace, workspace_bytes, stream);
    else
        gemv_4bit_stream(dtype, A, B, absmax, absmax8, absmax_code, absmax_offset, code16, out, bias, M, N, K, blocksize,
                         quant_type, stream);
}

// Gated call (bnb_mi355x_gemm_4bit_gated) on the interleaved [N = 2F, K] matrix at M rows: the kernel FAMILY the plain call on the
// same matrix and M runs - so that the gated result is the plain result's silu(gate) * up bit for bit - when that family has a gated
// form: kKernelStream or kKernelSm, else 0 (not supported). 16-bit activations, fp32 absmax, 1 <= M <= 16, blocksize >= 64, whole
// quantization blocks per row, aligned pointers.
int gated_family(int dtype, const void* A, const uint8_t* B, const float* absmax, int M, int N, int K, int blocksize) {
    if ((dtype != 1 && dtype != 2) || M < 1 || M > 16 || N < 2 || (N & 1) || K <= 0 || blocksize < 64 || !is_pow2(blocksize) || (K % blocksize) != 0 ||
        !aligned_to(A, 16) || !aligned_to(B, 16) || !aligned_to(absmax, 4))
        return kKernelNone;
    if (route_to_mfma(0, dtype, A, B, nullptr, M, N, K, blocksize, aligned_to(absmax, 16))) {
        // (gemm_4bit_mfma's order: the tall-tile knob first, then the streaming MFMA kernel; every other MFMA kernel has no gated form)
        if (g_mfma_knob1.load(std::memory_order_relaxed) / 100 == 60)
            return kKernelNone;
        return gemm_4bit_sm_routes(dtype, M, N, K, blocksize) && gemm_4bit_sm_gated_supported(dtype, A, B, M, N, K, blocksize) &&
                       gemm_4bit_sm_serves(absmax, nullptr, blocksize)
                   ? kKernelSm
                   : kKernelNone;
    }
    return gemv_4bit_stream_gated_supported(dtype, M, N, K, blocksize) ? kKernelStream : kKernelNone;
}

// LoRA call (bnb_mi355x_gemm_4bit_lora) at M rows: the kernel FAMILY the plain bnb_mi355x_gemm_4bit call on the same matrix, M and
// statistics runs - the adapter term is an epilogue of that launch, everything in front of it the plain instance's - when that family
// has the epilogue: kKernelStream or kKernelSm, else 0 (not supported). 16-bit activations, 1 <= M <= 16, blocksize >= 64, whole
// quantization blocks per row, r a multiple of 8 in [8, 128], aligned pointers.
int lora_family(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const void* lora_t, const void* lora_b, int M,
                int N, int K, int blocksize, int r) {
    if ((dtype != 1 && dtype != 2) || M < 1 || M > 16 || N < 1 || K <= 0 || blocksize < 64 || !is_pow2(blocksize) || (K % blocksize) != 0 || r < 8 || r > 128 ||
        (r % 8) != 0 || !aligned_to(A, 16) || !aligned_to(B, 16) || !aligned_to(absmax, 4) || !aligned_to(lora_t, 16) || !aligned_to(lora_b, 16))
        return kKernelNone;
    if (route_to_mfma(0, dtype, A, B, nullptr, M, N, K, blocksize, absmax8 == nullptr && aligned_to(absmax, 16))) {
        // (gemm_4bit_mfma's order: the tall-tile knob, the streaming MFMA kernel, the streaming kernel for rows that are not whole
        // 256-k chunks; every other MFMA kernel has no LoRA epilogue)
        if (g_mfma_knob1.load(std::memory_order_relaxed) / 100 == 60)
            return kKernelNone;
        if (gemm_4bit_sm_routes(dtype, M, N, K, blocksize) && gemm_4bit_sm_supported(dtype, A, B, nullptr, M, N, K, blocksize) &&
            gemm_4bit_sm_serves(absmax, absmax8, blocksize))
            return gemm_4bit_sm_lora_supported(dtype, A, B, M, N, K, blocksize, r) ? kKernelSm : kKernelNone;
        if ((K % 256) == 0)
            return kKernelNone;
    }
    return gemv_4bit_stream_lora_supported(dtype, M, N, K, blocksize, r) ? kKernelStream : kKernelNone;
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
// Groups of 17 ... 64 rows as ONE launch of the streaming MFMA kernel - although no member's own route at that many rows is this
// kernel: its 32-row instances multiply two 16-row blocks against every decoded weight fragment (row passes of 32 over grid.y above
// that; small groups: passes of 16 side by side on the CUs they leave idle), and the group shares one boundary, one table build and one
// activation fetch per CU. Measured (profiles/r6_grouped_ab.txt, third table; us per group, grouped launch vs the members one by one):
// 4 x 4096^2 M = 24 / 32 / 48 / 64 17.2 / 17.3 / 29.6 / 30.2 vs 32.9 / 33.4 / 39.4 / 44.4; 4096 + 2 x 1024 (x 4096) 11.0 / 11.3 / 19.7 / 20.0
// vs 19.4 / 20.2 / 21.6 / 22.8; 3 x 512 x 4096 5.9 / 5.9 / 7.9 / 7.9 vs 15.1 / 15.3 / 15.4 / 15.4; 2 x 11008 x 4096 26.8 / 27.0 vs 28.0 / 28.4
// but 47.4 / 48.4 vs 35.0 / 35.5 at 48 / 64 rows; 2 x 14336 x 4096 and 3 x 8192^2 behind (big members keep their own kernels).
// Such a group is NOT bit-identical to separate calls (another kernel family: the oracle's tolerance, like every fused call).
static bool grouped_sm_passes(int dtype, int count, const int* N, int M, int K, int blocksize) {
    if (dtype == 0 || M <= 16 || M > 64 || count < 2 || count > 8 || blocksize < 64 || (K % 64) != 0 || g_mfma_knob0.load(std::memory_order_relaxed) != 0 ||
        g_mfma_knob1.load(std::memory_order_relaxed) != 0)
        return false;
    long long weights = 0;
    for (int i = 0; i < count; ++i)
        weights += static_cast<long long>(N[i]) * K;
    return weights <= (M <= 32 ? (96LL << 20) : (72LL << 20));
}
void bnb_mi355x_gemm_4bit_grouped(int dtype, const void* A, int count, const uint8_t* const* B, const float* const* absmax,
                                  const uint8_t* const* absmax_8bit, const float* const* absmax_code,
                                  const float* const* absmax_offset, void* const* out, const void* const* bias, const int* N,
                                  int M, int K, int blocksize, int quant_type, bnb_stream_t s) {
    if (count <= 0 || M <= 0)
        return;
    require_quant_type("gemm_4bit_grouped", quant_type);
    // Tried in this order (bnb_mi355x_gemm_4bit_grouped_route answers the same question from shapes alone):
    //  * up to 8 members that the single-matrix entry point would ALL route to the streaming MFMA kernel (2 ... 16 rows,
    //    csrc/gemm4_mfma.hip: sm_selected): ONE launch of that kernel over the members' rows - bit-identical to separate calls (the
    //    same kernel family, and its summation order does not depend on the launch geometry);
    //  * a group of 17 ... 64 rows that grouped_sm_passes accepts (above): ONE launch of that kernel as well, in row passes of 32 or
    //    16 - NOT bit-identical to separate calls, whose route at that many rows is another family;
    //  * otherwise, when no member is routed to an MFMA kernel and gemv_4bit_grouped takes the group (M <= 4, up to 8 matrices,
    //    K % 32 == 0, single-phase rows): ONE launch of the streaming kernel, bit-identical to separate calls;
    //  * everything else (mixed routes, more than 8 matrices, a group either launcher refuses): matrix by matrix.
    bool any_mfma = false, all_sm = count <= 8;
    for (int i = 0; i < count; ++i) {
        any_mfma = any_mfma || route_to_mfma(0, dtype, A, B[i], nullptr, M, N[i], K, blocksize,
                                             (absmax_8bit == nullptr || absmax_8bit[i] == nullptr) && aligned_to(absmax[i], 16));
        all_sm = all_sm && gemm_4bit_sm_routes(dtype, M, N[i], K, blocksize);
    }
    if ((all_sm || grouped_sm_passes(dtype, count, N, M, K, blocksize)) &&
        gemm_4bit_sm_grouped(dtype, A, count, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, N, M, K, blocksize, quant_type, S(s)))
        return;
    if (!any_mfma && gemv_4bit_grouped(dtype, A, count, B, absmax, absmax_8bit, absmax_code, absmax_offset, out, bias, N, M, K,
                                       blocksize, quant_type, S(s)))
        return;
    // not a streaming-kernel shape (M > 4, more than 8 matrices, odd K ...): one launch per matrix, same results
    for (int i = 0; i < count; ++i)
        gemm_4bit_dispatch(0, dtype, A, B[i], absmax[i], absmax_8bit ? absmax_8bit[i] : nullptr,
                           absmax_code ? absmax_code[i] : nullptr, absmax_offset ? absmax_offset[i] : nullptr, nullptr, out[i],
                           bias ? bias[i] : nullptr, M, N[i], K, blocksize, quant_type, nullptr, 0, S(s));
}
int bnb_mi355x_gemm_4bit_grouped_route(int dtype, int count, const int* N, int M, int K, int blocksize) {
    // what bnb_mi355x_gemm_4bit_grouped does with such a group, assuming aligned pointers and members of one kind of statistics:
    // 2 = one launch of the streaming MFMA kernel, 1 = one launch of the streaming kernel, 0 = matrix by matrix
    if (count <= 0 || count > 8 || M <= 0 || blocksize <= 0 || K % blocksize != 0)
        return 0;
    bool any_mfma = false, all_sm = true;
    for (int i = 0; i < count; ++i) {
        any_mfma = any_mfma || route_to_mfma(0, dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N[i], K, blocksize, true);
        all_sm = all_sm && gemm_4bit_sm_routes(dtype, M, N[i], K, blocksize) &&
                 gemm_4bit_sm_supported(dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N[i], K, blocksize);
    }
    if (all_sm)
        return 2;
    if (grouped_sm_passes(dtype, count, N, M, K, blocksize)) {
        bool ok = true;
        for (int i = 0; i < count; ++i)
            ok = ok && gemm_4bit_sm_supported(dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N[i], K, blocksize);
        if (ok)
            return 2;
    }
    bool stream_sizes = true; // (gemv_4bit_grouped: every member below 2^32 elements)
    for (int i = 0; i < count; ++i)
        stream_sizes = stream_sizes && gemv_4bit_stream_size_ok(N[i], K);
    return (!any_mfma && M <= 4 && stream_sizes) ? 1 : 0;
}
size_t bnb_mi355x_gemm_4bit_workspace_bytes(int kernel, int dtype, int M, int N, int K, int blocksize) {
    // alignment of A/B is unknown here; assume the aligned (fast) case, an unused workspace is harmless
    if (!route_to_mfma(kernel, dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N, K, blocksize, true))
        return 0;
    return gemm_4bit_mfma_workspace_bytes(M, N, K, blocksize);
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
    const int family = gated_family(dtype, A, B, absmax, M, N, K, blocksize);
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
    return gated_family(dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), M, N, K, blocksize) != kKernelNone ? 1 : 0;
}

// ------------------------------------------------------------------ LoRA gemm_4bit (the adapter term as the decode kernels' epilogue)
void bnb_mi355x_gemm_4bit_lora(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax_8bit,
                               const float* absmax_code, const float* absmax_offset, void* out, const void* bias, const void* lora_t,
                               const void* lora_b, float scaling, int r, int M, int N, int K, int blocksize, int quant_type, bnb_stream_t s) {
    require_quant_type("gemm_4bit_lora", quant_type);
    const int family = lora_family(dtype, A, B, absmax, absmax_8bit, lora_t, lora_b, M, N, K, blocksize, r);
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
    return lora_family(dtype, kAlignedDummy, kAlignedDummy8, reinterpret_cast<const float*>(kAlignedDummy), nested ? kAlignedDummy8 : nullptr, kAlignedDummy,
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
    const int family = lora_family(dtype, A, B, absmax, absmax_8bit, lora_t, lora_b, M, N, K, blocksize, r);
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
    return route_to_mfma(kernel, dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N, K, blocksize, true) ? 1 : 0;
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
    // (gemm_4bit_dispatch's question, with the aligned pointers of the shape-only queries)
    const float* const absmax = reinterpret_cast<const float*>(kAlignedDummy);
    const uint8_t* const absmax8 = nested ? kAlignedDummy8 : nullptr;
    int v[16];
    if (route_to_mfma(kernel, dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N, K, blocksize, !nested) &&
        gemm_4bit_mfma_plan_query(dtype, kAlignedDummy, kAlignedDummy8, absmax, absmax8, M, N, K, blocksize, v)) {
        for (int i = 0; i < 16; ++i)
            out16[i] = v[i];
        return 1;
    }
    if (g_mfma_knob1.load(std::memory_order_relaxed) / 100 == 60 && route_to_mfma(kernel, dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N, K, blocksize, !nested) &&
        gemm_4bit_tall_supported(dtype, kAlignedDummy, kAlignedDummy8, nullptr, M, N, K, blocksize))
        return 0;
    int g[8];
    if (!gemv_4bit_stream_geometry(0, dtype, M, N, K, blocksize, g))
        return 0;
    const int w[16] = {kKernelStream, g[4], (M + g[6] - 1) / g[6], 1, 1, g[3], (K + 2047) / 2048, g[6], g[7], g[6], g[0], g[1], g[5], 2048, g[2], 0};
    for (int i = 0; i < 16; ++i)
        out16[i] = w[i];
    return 1;
}
int bnb_mi355x_gemm_4bit_sm_form_plan(int form, int dtype, int M, int N, const int* group_N, int K, int blocksize, int nested, int* out16) {
    if (out16 == nullptr || form < 1 || form > 4 || M <= 0 || N <= 0 || K <= 0 || blocksize <= 0)
        return 0;
    const float* const absmax = reinterpret_cast<const float*>(kAlignedDummy);
    int v[16];
    bool ok = false;
    if (form == 1)
        ok = !nested && gated_family(dtype, kAlignedDummy, kAlignedDummy8, absmax, M, N, K, blocksize) == kKernelSm && gemm_4bit_sm_plan_query(1, M, N, K, 0, v);
    else if (form <= 3)
        ok = lora_family(dtype, kAlignedDummy, kAlignedDummy8, absmax, nested ? kAlignedDummy8 : nullptr, kAlignedDummy, kAlignedDummy, M, N, K, blocksize, 8) == kKernelSm &&
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
