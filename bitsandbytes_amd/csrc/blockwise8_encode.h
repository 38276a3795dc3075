// blockwise8_encode.h — the device primitives of the 8-bit blockwise encoder, shared by blockwise8.hip (quantize_blockwise) and
// optim8.hip (the fused 8-bit optimizer update, which re-encodes its states with exactly this function). ONE definition of each;
// the rule they implement is described at the top of blockwise8.hip. All are __forceinline__: none leaves a symbol in a code object.
#pragma once

#include "bnb_common.h"

namespace bnb {

__device__ __forceinline__ float bin_value(unsigned u) {
    return -1.0f + (2.0f * static_cast<float>(u)) / 65535.0f; // the reference's expression, IEEE division
}

// T(m) = min{u in [0, 65536] : bin_value(u) > m}  (65536 if none). bin_value is non-decreasing in u, so instead of 17 bisection
// steps (17 correctly rounded divisions on the critical path of every launch) start from the algebraic inverse and walk the
// few steps the roundings can be off; every comparison is made with bin_value itself, so T is the same number.
__device__ __forceinline__ unsigned first_bin_above(float m) {
    if (m < -1.0f)
        return 0u; // bin_value(0) = -1 > m
    if (!(m < 1.0f))
        return 65536u; // bin_value(65535) = 1 is not > m; NaN compares false everywhere (what the bisection returned as well)
    int c = static_cast<int>((m + 1.0f) * 32767.5f);
    c = c < 0 ? 0 : (c > 65535 ? 65535 : c);
    while (c > 0 && bin_value(static_cast<unsigned>(c - 1)) > m)
        --c;
    while (c < 65536 && !(bin_value(static_cast<unsigned>(c)) > m))
        ++c;
    return static_cast<unsigned>(c);
}

__device__ __forceinline__ unsigned bin_of(float x, float inv) {
    float v = x * inv;
    v = fminf(fmaxf(v, -1.0f), 1.0f);
    const float t = (v + 1.0f) * 0.5f;
    const float p = __fmul_rn(t, 65535.0f); // separate rounding, as the un-contracted source reads
    const float r = __fadd_rn(p, 0.5f);     // (fused and un-fused agree on every tested input)
    return static_cast<unsigned>(r) & 0xFFFFu;
}

template <typename T> __device__ __forceinline__ void load4(const T* __restrict__ A, long i, long n, bool vec_ok, float (&x)[4]) {
    if (vec_ok && i + 4 <= n) {
        if constexpr (sizeof(T) == 4) {
            const f32x4 r = stream_load<true>(reinterpret_cast<const f32x4*>(A + i));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                x[j] = r[j];
        } else {
            typedef T v4 __attribute__((ext_vector_type(4)));
            const v4 r = stream_load<true>(reinterpret_cast<const v4*>(A + i));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                x[j] = static_cast<float>(r[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            x[j] = (i + j < n) ? static_cast<float>(A[i + j]) : 0.0f;
    }
}

// The encoder's two tables from the 256-entry code (256-thread workgroup; ends with a barrier). thr[i] = T_i = the first 16-bit bin
// whose value lies above the mid-point of code[i] and code[i + 1] (thr[255] = 65536); cell[c], c = bin >> 6: bits 0-7 thresholds
// below the cell, bits 8-15 thresholds inside it, bits 16-21 offset of the first one inside (what the common single-threshold case
// compares against).
__device__ __forceinline__ void build_cell_tables(const float* __restrict__ code, uint32_t* thr /* [256] LDS */, uint32_t* cell /* [1024] LDS */) {
    // below[c] = #{i < 255 : T_i < 64 c}, c = 0 .. 1024, as a prefix sum: a threshold T counts from cell (T >> 6) + 1 on, so mark it
    // there (LDS atomic: thresholds may share a cell) and scan. (A binary search per cell was 40 dependent LDS reads per thread:
    // ~1.7 us on the critical path of every launch.) cnt[0] stays 0; T = 65536 - no bin above the mid-point - lands in the spare slot.
    __shared__ __attribute__((aligned(16))) uint32_t cnt[1028];
    __shared__ uint32_t wave_tot[4];
    const int tid = threadIdx.x;
    const float lo = code[tid], hi = (tid < 255) ? code[tid + 1] : 0.0f;
#pragma unroll
    for (int c = tid; c < 1028; c += 256)
        cnt[c] = 0u;
    const unsigned t = first_bin_above((tid < 255) ? 0.5f * (lo + hi) : __builtin_inff());
    thr[tid] = t;
    __syncthreads();
    if (tid < 255)
        atomicAdd(&cnt[(t >> 6) + 1u], 1u);
    __syncthreads();
    // thread tid owns c = 4 tid + 1 .. 4 tid + 4
    const u32x4 mine = *reinterpret_cast<const u32x4*>(&cnt[4 * tid]); // cnt[4 tid .. 4 tid + 3]
    const uint32_t last = cnt[4 * tid + 4];
    const unsigned own[4] = {mine[1], mine[2], mine[3], last};
    const unsigned sum = own[0] + own[1] + own[2] + own[3];
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        incl += ((tid & 63) >= off) ? o : 0u;
    }
    if ((tid & 63) == 63)
        wave_tot[tid >> 6] = incl;
    __syncthreads();
    unsigned run = incl - sum; // thresholds below cell 4 tid (= below[4 tid]: cnt[0 .. 4 tid] summed)
#pragma unroll
    for (int w = 0; w < 3; ++w)
        run += (w < (tid >> 6)) ? wave_tot[w] : 0u;
    // cell c = 4 tid + j: below[c] = run + own[0 .. j - 1], inside = below[c + 1] - below[c] = own[j]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned c = 4u * tid + j;
        const unsigned below = run, inside = own[j];
        const unsigned off = (inside > 0u) ? (thr[below] - c * 64u) : 0u;
        cell[c] = below | (inside << 8) | (off << 16);
        run += inside;
    }
    __syncthreads();
}

// The code of 16-bit bin u from the two tables: q = #{i : T_i <= u}. One LDS read and one compare where the bin's cell holds at
// most one threshold; the few cells with several (the dynamic map is dense only around zero) count them by binary search.
__device__ __forceinline__ unsigned cell_count(unsigned u, const uint32_t* thr, const uint32_t* cell) {
    const unsigned ce = cell[u >> 6];
    unsigned q = ce & 0xFFu;
    const unsigned cnt = (ce >> 8) & 0xFFu;
    if (cnt > 1u) { // several thresholds in this cell (the code is dense only around zero): binary search
        unsigned lo = 0;
#pragma unroll
        for (unsigned step = 128; step >= 1; step >>= 1)
            lo += (lo + step - 1 < cnt && thr[q + lo + step - 1] <= u) ? step : 0u;
        q += lo;
    } else {
        q += (cnt == 1u && (u & 63u) >= (ce >> 16)) ? 1u : 0u;
    }
    return q;
}

} // namespace bnb
