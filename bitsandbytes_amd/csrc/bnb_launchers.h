// bnb_launchers.h — every function and variable of namespace bnb that one .hip file defines and another one uses, grouped by
// defining file. Internal to the library (the C ABI is include/bnb_mi355x.h). The users include it AND so does every defining
// file: a signature that drifts from its definition is a compile error there, not an undefined symbol when the library loads.
#pragma once

#include "bnb_common.h"

namespace bnb {

// quantize4.hip
void quantize_4bit_set_variant(int variant);
void quantize_4bit_f32(const float* A, float* absmax, uint8_t* out, int blocksize, long n, int quant_type, hipStream_t s);
void quantize_4bit_f16(const void* A, float* absmax, uint8_t* out, int blocksize, long n, int quant_type, hipStream_t s);
void quantize_4bit_bf16(const void* A, float* absmax, uint8_t* out, int blocksize, long n, int quant_type, hipStream_t s);

// dequantize4.hip
void dequantize_4bit_set_variant(int variant);
void dequantize_4bit_f32(const uint8_t* A, const float* absmax, float* out, int blocksize, long n, int qt, hipStream_t s);
void dequantize_4bit_f16(const uint8_t* A, const float* absmax, void* out, int blocksize, long n, int qt, hipStream_t s);
void dequantize_4bit_bf16(const uint8_t* A, const float* absmax, void* out, int blocksize, long n, int qt, hipStream_t s);
void dequantize_4bit_nested(int dtype, const uint8_t* A, const uint8_t* absmax8, const float* absmax2, const float* code2, const float* offset,
                            void* out, int blocksize, long n, int qt, hipStream_t stream);
void dequantize_4bit_rows(int dtype, const uint8_t* A, const float* absmax, const void* idx, int index_bytes, void* out, long rows_out,
                          long num_rows, int row_len, int blocksize, int qt, hipStream_t s);

// blockwise8.hip
void quantize_8bit_set_variant(int variant);
void quantize_absmax_nested(const float* code, const float* absmax, long n, float* partial, float* offset_out, uint8_t* out, float* absmax2,
                            hipStream_t stream);
void quantize_8bit_f32(const float* code, const float* A, float* absmax, uint8_t* out, int bs, long n, hipStream_t s);
void quantize_8bit_f16(const float* code, const void* A, float* absmax, uint8_t* out, int bs, long n, hipStream_t s);
void quantize_8bit_bf16(const float* code, const void* A, float* absmax, uint8_t* out, int bs, long n, hipStream_t s);
void dequantize_8bit_f32(const float* code, const uint8_t* A, const float* absmax, float* out, int bs, long n, hipStream_t s);
void dequantize_8bit_f16(const float* code, const uint8_t* A, const float* absmax, void* out, int bs, long n, hipStream_t s);
void dequantize_8bit_bf16(const float* code, const uint8_t* A, const float* absmax, void* out, int bs, long n, hipStream_t s);

// gemv4_stream.hip (the streaming dot kernel: M <= 4, and what a call outside every MFMA kernel's preconditions runs)
void gemv_4bit_stream(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                      const float* absmax_offset, const float* code16, void* out, const void* bias, int M, int N, int K, int blocksize,
                      int quant_type, hipStream_t stream);
bool gemv_4bit_grouped(int dtype, const void* A, int count, const uint8_t* const* B, const float* const* absmax, const uint8_t* const* absmax8,
                       const float* const* absmax_code, const float* const* absmax_offset, void* const* out, const void* const* bias, const int* N,
                       int M, int K, int blocksize, int quant_type, hipStream_t stream);
void gemv_4bit_stream_tuning(int ns, int sw, int rows_per_wg, int nt, int waves);
bool gemv_4bit_stream_exact(int dtype, int M, int N, int K, int blocksize, bool nested);
bool gemv_4bit_stream_geometry(int form, int dtype, int M, long rows, int K, int blocksize, int* out8);
bool gemv_4bit_stream_size_ok(long N, long K);
bool gemv_4bit_stream_gated_supported(int dtype, int M, int N, int K, int blocksize);
bool gemv_4bit_stream_gated(int dtype, const void* A, const uint8_t* B, const float* absmax, void* out, const void* bias, int M, int N, int K,
                            int blocksize, int quant_type, hipStream_t stream);
bool gemv_4bit_stream_lora_supported(int dtype, int M, int N, int K, int blocksize, int r);
bool gemv_4bit_stream_lora(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                           const float* absmax_offset, void* out, const void* bias, const void* lora_t, const void* lora_b, float scaling, int r,
                           int M, int N, int K, int blocksize, int quant_type, hipStream_t stream);
bool gemv_4bit_stream_lora_ids(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                               const float* absmax_offset, void* out, const void* bias, const void* lora_t, const void* lora_b, const float* scalings,
                               const void* ids, int index_bytes, int A_n, int r, int M, int N, int K, int blocksize, int quant_type, hipStream_t stream);
bool gemv_4bit_peer_serves(int world, int ns, int K, int blocksize, int mode, long max_values, int wg_limit);
bool gemv_4bit_peer(void* const* bufs, void* epoch_word, int world, int rank, int dtype, const void* A, const uint8_t* B, const float* absmax,
                    const uint8_t* absmax8, const float* absmax_code, const float* absmax_offset, const void* bias, void* out_local, int ns, int K,
                    int blocksize, int quant_type, int mode, long max_values, int wg_limit, uint32_t epoch_offset, uint32_t spin_bound,
                    hipStream_t stream);
void peer_chain_read(void* const* bufs, void* epoch_word, int world, int rank, int dtype, void* out, int nvalues, long max_values,
                     uint32_t epoch_offset, uint32_t spin_bound, hipStream_t stream);

// gemm4_mfma.hip (gemm_4bit's route and dispatcher, the slab finalize launch and the library-owned workspace)
extern thread_local TlsKnob g_mfma_knob0, g_mfma_knob1;
void gemm_4bit_finalize(int dtype, const float* ws, const void* bias, void* out, int M, int N, int kslices, hipStream_t stream);
float* gemm_4bit_internal_workspace(size_t bytes, hipStream_t stream);
// The alignment of A / B / absmax is unknown to the shape-only queries: they assume the aligned (fast) case and pass this.
alignas(16) inline const int kAlignedDummy[4] = {0, 0, 0, 0};
inline const uint8_t* const kAlignedDummy8 = reinterpret_cast<const uint8_t*>(kAlignedDummy);
// gemm_4bit_route's answer: the kernel family (kKernelStream / Sm / Kq / Rt / Pc / Tall), the K slices / wavefronts a tuning knob forces
// on it (0 = built-in choice), and the call's one snapshot of the knobs for what the launch passes on (variant, ablation)
struct Gemm4Route {
    int kernel;
    int force_ks, force_waves;
    int knob0, knob1;
};
Gemm4Route gemm_4bit_route(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* code16, int M,
                           int N, int K, int blocksize, bool without_kq = false);
void gemm_4bit(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
               const float* absmax_offset, const float* code16, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type,
               void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t gemm_4bit_workspace_bytes(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax, int M, int N, int K, int blocksize);
bool gemm_4bit_plan_query(int kernel, int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, int M, int N, int K,
                          int blocksize, int* out16);
int gemm_4bit_gated_family(int dtype, const void* A, const uint8_t* B, const float* absmax, int M, int N, int K, int blocksize);
int gemm_4bit_lora_family(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const void* lora_t, const void* lora_b,
                          int M, int N, int K, int blocksize, int r);
int gemm_4bit_grouped_route(int dtype, const void* A, int count, const uint8_t* const* B, const float* const* absmax, const uint8_t* const* absmax8,
                            const int* N, int M, int K, int blocksize);

// gemm4_mfma_rt.hip (the register-transposed kernel for small batches on small / medium matrices)
bool gemm_4bit_rt_supported(int dtype, const void* A, const uint8_t* B, const float* code16, int M, int N, int K, int blocksize);
bool gemm_4bit_rt_serves(const float* absmax, const uint8_t* absmax8, int blocksize);
size_t gemm_4bit_rt_workspace_bytes(int M, int N, int K, int force_ks);
void gemm_4bit_rt(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                  const float* absmax_offset, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, void* workspace,
                  size_t workspace_bytes, int force_ks, int force_waves, int variant, hipStream_t stream);
void gemm_4bit_rt_plan_query(int M, int N, int K, int blocksize, int force_ks, int force_waves, int* out16);

// gemm4_mfma_kq.hip (the K-quarter kernel: 32x32x16 MFMA, shares of a chunk copied to registers, 17 ... 64-row batches)
bool gemm_4bit_kq_supported(int dtype, const void* A, const uint8_t* B, const float* code16, int M, int N, int K, int blocksize);
bool gemm_4bit_kq_serves(const float* absmax, const uint8_t* absmax8, int blocksize, int K);
size_t gemm_4bit_kq_workspace_bytes(int M, int N, int K, int force_ks);
void gemm_4bit_kq(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                  const float* absmax_offset, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, void* workspace,
                  size_t workspace_bytes, int force_ks, int ablate, hipStream_t stream);
void gemm_4bit_kq_plan_query(int M, int N, int K, bool nested, int force_ks, int* out16);

// gemm4_mfma_sm.hip (the streaming MFMA kernel: one persistent workgroup per CU, activations once per CU; 2 ... 16 rows)
bool gemm_4bit_sm_supported(int dtype, const void* A, const uint8_t* B, const float* code16, int M, int N, int K, int blocksize);
bool gemm_4bit_sm_serves(const float* absmax, const uint8_t* absmax8, int blocksize);
void gemm_4bit_sm(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                  const float* absmax_offset, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, int variant,
                  hipStream_t stream);
bool gemm_4bit_sm_gated_supported(int dtype, const void* A, const uint8_t* B, int M, int N, int K, int blocksize);
bool gemm_4bit_sm_gated(int dtype, const void* A, const uint8_t* B, const float* absmax, void* out, const void* bias, int M, int N, int K,
                        int blocksize, int quant_type, hipStream_t stream);
bool gemm_4bit_sm_lora_supported(int dtype, const void* A, const uint8_t* B, int M, int N, int K, int blocksize, int r);
bool gemm_4bit_sm_lora(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                       const float* absmax_offset, void* out, const void* bias, const void* lora_t, const void* lora_b, float scaling, int r,
                       int M, int N, int K, int blocksize, int quant_type, hipStream_t stream);
bool gemm_4bit_sm_lora_ids(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                           const float* absmax_offset, void* out, const void* bias, const void* lora_t, const void* lora_b, const float* scalings,
                           const void* ids, int index_bytes, int A_n, int r, int M, int N, int K, int blocksize, int quant_type, hipStream_t stream);
bool gemm_4bit_sm_grouped(int dtype, const void* A, int count, const uint8_t* const* B, const float* const* absmax, const uint8_t* const* absmax8,
                          const float* const* absmax_code, const float* const* absmax_offset, void* const* out, const void* const* bias,
                          const int* N, int M, int K, int blocksize, int quant_type, hipStream_t stream);
bool gemm_4bit_sm_plan_query(int form, int M, int N, int K, int variant, int* out16);
bool gemm_4bit_sm_grouped_plan_query(int count, const int* N, int M, int K, int* out16);

// gemm4_mfma_tall.hip (128 x 128 tiles, pre-scaled operand decoded once per 128 rows: tall batches)
bool gemm_4bit_tall_supported(int dtype, const void* A, const uint8_t* B, const float* code16, int M, int N, int K, int blocksize);
void gemm_4bit_tall(int dtype, const void* A, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                    const float* absmax_offset, void* out, const void* bias, int M, int N, int K, int blocksize, int quant_type, int ablate,
                    hipStream_t stream);

// gemm4_grad_input.hip
void gemm_4bit_grad_input_set_slices(int ns);
bool gemm_4bit_grad_input_supported(int dtype, const void* G, const uint8_t* B, int M, int N, int K, int blocksize);
size_t gemm_4bit_grad_input_workspace_bytes(int M, int N, int K);
void gemm_4bit_grad_input(int dtype, const void* G, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                          const float* absmax_offset, void* out, int M, int N, int K, int blocksize, int quant_type, void* workspace,
                          size_t workspace_bytes, hipStream_t stream);
bool gemm_4bit_grad_input_plan_query(int dtype, int M, int N, int K, int blocksize, int* out16);

// gemm4_experts.hip
bool gemm_4bit_experts_supported(int dtype, long E, long N, long K, int blocksize);
void gemm_4bit_experts(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax8,
                       const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes, void* out, long P,
                       int S, int E, int N, int K, int blocksize, int quant_type, hipStream_t stream);
bool gemm_4bit_experts_ffn_supported(int dtype, long E, long N, long K, int blocksize, int gated);
void gemm_4bit_experts_ffn(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax8,
                           const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes,
                           const void* row_scale, int row_scale_dtype, int gated, void* out, long P, int S, int E, int N, int K, int blocksize,
                           int quant_type, hipStream_t stream);

// lora_shrink.hip
bool lora_shrink_supported(int dtype, int M, int R, int K);
bool lora_shrink(int dtype, const void* x, const void* lora_a, void* t, int M, int R, int K, const int* splits, int n_splits, hipStream_t stream);
bool lora_shrink_ids_supported(int dtype, int M, int A_n, int R, int K);
bool lora_shrink_ids(int dtype, const void* x, const void* lora_a, const void* ids, int index_bytes, void* t, int M, int A_n, int R, int K,
                     const int* splits, int n_splits, hipStream_t stream);

// moe_route.hip (the router's scoring + top-k launch; the fields of bnb_mi355x_moe_topk_args, include/bnb_mi355x.h)
struct MoeTopkCall {
    int dtype, scoring, renormalize; // logits: 0 fp32, 1 fp16, 2 bf16; 0 softmax, 1 sigmoid
    int rows, experts, top_k;
    float scale;
    const void* logits;       // [rows, experts]
    const float* select_bias; // [experts] or nullptr
    int* ids;                 // [rows, top_k]
    float* weights;           // [rows, top_k]
};
bool moe_topk_supported(int dtype, int rows, int experts, int top_k);
bool moe_topk(const MoeTopkCall& call, hipStream_t stream);
// (group-limited routing: the fields of bnb_mi355x_moe_topk_grouped_args)
struct MoeTopkGroupedCall {
    MoeTopkCall base;
    int n_group, topk_group, group_score; // group_score: 0 "max", 1 "top2sum"
};
bool moe_topk_grouped_supported(int dtype, int rows, int experts, int top_k, int n_group, int topk_group, int group_score);
bool moe_topk_grouped(const MoeTopkGroupedCall& call, hipStream_t stream);

// c_api.hip (g_last_gemm_kernel, defined there as well, is declared in bnb_common.h)
#ifdef BNB_PROFILING
extern unsigned long long* g_dbg_buf; // profiling builds only: device buffer for the kernels' s_memtime stamps
inline unsigned long long* stamp_buffer() { return g_dbg_buf; }
#else
inline unsigned long long* stamp_buffer() { return nullptr; }
#endif

// The mixed-adapter block of a LoRA call (gemv_4bit_stream_lora_ids / gemm_4bit_sm_lora_ids; absent: one adapter for every row):
// lora_b is a stack [A_n, N, r], scalings [A_n] fp32 and ids [M] (int32 / int64) live on the device.
struct LoraIds {
    const float* scalings;
    const void* ids;
    int index_bytes, A_n;
    bool valid() const {
        return A_n >= 1 && A_n <= 64 && (index_bytes == 4 || index_bytes == 8) && ids != nullptr && scalings != nullptr &&
               aligned_to(ids, static_cast<size_t>(index_bytes)) && aligned_to(scalings, 4);
    }
};

} // namespace bnb
