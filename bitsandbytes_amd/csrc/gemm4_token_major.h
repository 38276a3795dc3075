// gemm4_token_major.h — what the two token-major MoE kernels share (gemm4_experts_combine.hip: the down projection with the slot
// sum; gemm4_experts_gate_up.hip: the gate / up projection with gated SiLU): the lane map chosen from K alone, the activations of a
// lane as fp32 registers, the decode table, one weight row's chunks and its sum. The order of every fp32 addition below is a function
// of (K, blocksize) alone - the ledger of both kernels.
#pragma once
#include "bnb_launchers.h"

namespace bnb {
namespace token_major {

constexpr int kChunkK = 32;      // k of one 16-byte load of a lane
constexpr int kLutBytes = 65536; // 256 entries x 32 bank-private copies x 8 B: byte -> (code[hi], code[lo]) fp32
constexpr int kCode2Bytes = 1024;
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kMaxSlots = 16;            // the router's top_k bound
constexpr int kMaxSegs = 16;             // K <= 65536
constexpr int kSegChunks = 128;          // L = 64, Q = 2: the segment of a long row
constexpr size_t kPartBudget = 12 * 1024; // (slot, segment, row) sums; with table and code2 two workgroups fit a CU's 160 KiB

struct CombinePlan {
    int L, Q, SEGS;
};

// The lane map of a row length: the smallest cover L * Q of the row's chunks (ties: fewer lanes per row, so more rows per load);
// rows longer than 192 chunks in segments of 128.
inline CombinePlan combine_plan(int K) {
    const int C = K / kChunkK;
    if (C > 192)
        return {64, 2, (C + kSegChunks - 1) / kSegChunks};
    CombinePlan best{64, 3, 1};
    for (int L = 64; L >= 8; L >>= 1)
        for (int Q = 3; Q >= 2; --Q)
            if (L * Q >= C && L * Q <= best.L * best.Q)
                best = {L, Q, 1};
    return best;
}

template <typename T> __device__ __forceinline__ void load_act32(const T* src, f32x2 (&dst)[16]);
template <> __device__ __forceinline__ void load_act32<bf16>(const bf16* src, f32x2 (&dst)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32x4 v = reinterpret_cast<const u32x4*>(src)[q];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            dst[4 * q + i] = f32x2{__builtin_bit_cast(float, v[i] << 16), __builtin_bit_cast(float, v[i] & 0xFFFF0000u)};
    }
}
template <> __device__ __forceinline__ void load_act32<f16>(const f16* src, f32x2 (&dst)[16]) {
    using h2 = __attribute__((ext_vector_type(2))) f16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32x4 v = reinterpret_cast<const u32x4*>(src)[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const h2 p = __builtin_bit_cast(h2, static_cast<uint32_t>(v[i]));
            dst[4 * q + i] = f32x2{static_cast<float>(p[0]), static_cast<float>(p[1])};
        }
    }
}
template <> __device__ __forceinline__ void load_act32<float>(const float* src, f32x2 (&dst)[16]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 v = reinterpret_cast<const f32x4*>(src)[q];
        dst[2 * q] = f32x2{v[0], v[1]};
        dst[2 * q + 1] = f32x2{v[2], v[3]};
    }
}

// id i of an [T, S] id tensor; the address is workgroup-uniform wherever the kernels call this in their main loops
__device__ __forceinline__ long long token_id(const void* ids, int idx64, long i) {
    return idx64 ? static_cast<const long long*>(ids)[i] : static_cast<long long>(static_cast<const int*>(ids)[i]);
}

// the n-th set bit of mask (n < popcount)
__device__ __forceinline__ int nth_bit(uint32_t mask, int n) {
    for (int i = 0; i < n; ++i)
        mask &= mask - 1;
    return __builtin_ctz(mask);
}

template <int Q> struct Stage {
    u32x4 w[Q]; // the lane's chunk of each round
    float s[Q]; // fp32 absmax of the chunk's block (plain) / the block's 8-bit code as an integer (nested)
    float s2[Q]; // nested: second-level absmax of the block's group of 256
};

// decode table: entry e8 (a packed byte) = 32 copies of (code[e8 >> 4], code[e8 & 15]) in fp32, 256 B per entry, copy c at byte
// 8 c. 16-byte chunk it * 512 + tid holds two copies of entry it * 32 + (tid >> 4): every ds_write_b128 of a wavefront covers 1 KiB.
// Nested: the second-level code behind it. The caller's barrier follows.
template <bool NESTED> __device__ __forceinline__ void build_decode_table(unsigned char* smem, int tid, bool fp4, const float* absmax_code) {
    const float lo = code_literal((tid >> 4) & 15, fp4);
    constexpr int kIters = kLutBytes / 16 / kThreads;
    static_assert(kThreads == 512 && kIters == 8, "chunk -> entry arithmetic below");
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const float hi = (tid >> 8) ? code_literal(2 * it + 1, fp4) : code_literal(2 * it, fp4);
        *reinterpret_cast<f32x4*>(smem + (it * kThreads + tid) * 16) = f32x4{hi, lo, hi, lo};
    }
    if constexpr (NESTED) {
        if (tid < 256)
            reinterpret_cast<float*>(smem + kLutBytes)[tid] = absmax_code[tid];
    }
}

// The lane's Q chunks of the weight row whose first element is row_elem (row * K), at its k offsets kc[], with their statistics.
template <bool NESTED, int Q>
__device__ __forceinline__ Stage<Q> load_row_chunks(const uint8_t* B, const float* absmax, const uint8_t* absmax8, long row_elem,
                                                    const int (&kc)[Q], int bs_shift) {
    Stage<Q> st;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const long elem = row_elem + kc[q];
        st.w[q] = *reinterpret_cast<const u32x4*>(B + (elem >> 1));
        const long blk = elem >> bs_shift;
        if constexpr (NESTED) {
            st.s[q] = __builtin_bit_cast(float, static_cast<uint32_t>(absmax8[blk]));
            st.s2[q] = absmax[blk >> 8];
        } else {
            st.s[q] = absmax[blk];
            st.s2[q] = 0.0f;
        }
    }
    return st;
}

// The sum of one weight row against the lane group's activations: per chunk 32 products in four fp32 FMA chains (even / odd k of two
// alternating bytes), ((c00 + c01) + (c10 + c11)) * block scale; the lane's Q chunk values in ascending round order; an xor butterfly
// over the L lanes of the group (1, 2, 4, 8, 16, 32) - every lane of the group ends with the sum (steps behind L are skipped: uniform).
template <bool NESTED, int Q>
__device__ __forceinline__ float row_sum(const Stage<Q>& st, const f32x2 (&xr)[Q][16], const bool (&k_ok)[Q], const unsigned char* smem,
                                         const float* code2, uint32_t lane_off, float offset, int L) {
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        f32x2 cp[16];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // {lane copy offset, weight byte i, 0, 0}: byte * 256 + copy * 8
                const uint32_t off = __builtin_amdgcn_perm(st.w[q][d], lane_off, 0x0C0C0400u + (i << 8));
                cp[4 * d + i] = *reinterpret_cast<const f32x2*>(smem + off);
            }
        float scale;
        if constexpr (NESTED)
            scale = nested_scale(code2[__builtin_bit_cast(uint32_t, st.s[q])], st.s2[q], offset);
        else
            scale = st.s[q];
        scale = k_ok[q] ? scale : 0.0f;
        // four scalar FMA chains: [byte parity][even k, odd k] (no packed fp32 arithmetic in these kernels, see the Makefile)
        float acc[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            acc[b & 1][0] = fmaf(cp[b][0], xr[q][b][0], acc[b & 1][0]);
            acc[b & 1][1] = fmaf(cp[b][1], xr[q][b][1], acc[b & 1][1]);
        }
        const float cv = rounded_f32(((acc[0][0] + acc[0][1]) + (acc[1][0] + acc[1][1])) * scale);
        v = q == 0 ? cv : v + cv;
    }
    v = dpp_add<0xB1>(v);
    v = dpp_add<0x4E>(v);
    v = dpp_add<0x141>(v);
    if (L >= 16)
        v = dpp_add<0x140>(v);
    if (L >= 32)
        v += __shfl_xor(v, 16, kWave);
    if (L == 64)
        v += __shfl_xor(v, 32, kWave);
    return v;
}

} // namespace token_major
} // namespace bnb
