// int8_quant.hip — LLM.int8() row-wise quantization (gfx950): q[r, c] = int8(rint(A[r, c] * (127 / absmax_r))), row_stats[r] = absmax_r.
//
// The arithmetic of the reference's default backend (bitsandbytes/backends/default/ops.py:163-167), every operation correctly rounded
// in fp32: the absolute maximum of the row as fp32, ONE IEEE division 127.0f / absmax, one multiplication per element, round to
// nearest even. A row whose absmax is 0 (the reference divides by zero there) writes zeros and the statistic 0.
//
//  * One workgroup of 256 threads per row; two phases (absmax, quantize) around one reduction: across the lanes of a wavefront
//    first, then across the four wavefronts through LDS. No atomics.
//  * Wide instance (cols % 16 == 0, A and q 16-byte aligned): a thread works on groups of 16 consecutive elements - two (16-bit) or four
//    (fp32) 16-byte loads, four int8 packed per dword, ONE 16-byte store. The first kKeep groups of a thread stay in registers across
//    the two phases: rows up to kRegCols = 8192 elements are read once, longer rows re-read what lies behind.
//  * Narrow instance (every other shape: odd cols, tails): one element per thread and step, read in both phases, byte stores.
//  * THRESH (threshold > 0): an element with |a| >= threshold (compared in fp32) takes no part in the absmax and is written as 0; a row
//    of outliers only is an all-zero row. Finding the outlier columns is the caller's business (backends/hip.py).
#include "bnb_launchers.h"

namespace bnb {

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 16;                             // elements per thread and step of the wide instance: one 16-byte store
constexpr int kKeep = 2;                               // groups of a thread that stay in registers
constexpr int kRegCols = kThreads * kKeep * kGroup;    // the longest row that is read once
static_assert(kRegCols == 8192, "tests/test_gpu_int8.py names a row length just above this limit");

template <typename T> struct Group {
    T e[kGroup];
};

template <typename T> __device__ __forceinline__ Group<T> load_group(const T* p) {
    constexpr int kVecs = kGroup * sizeof(T) / 16;
    struct Raw {
        u32x4 v[kVecs];
    } raw;
#pragma unroll
    for (int i = 0; i < kVecs; ++i)
        raw.v[i] = reinterpret_cast<const u32x4*>(p)[i];
    return __builtin_bit_cast(Group<T>, raw);
}

template <typename T, bool WIDE, bool THRESH>
__global__ __launch_bounds__(kThreads) void int8_quant_kernel(const T* A, int8_t* q, float* row_stats, int cols, float threshold) {
    __shared__ float red[kThreads / 64];
    const int tid = threadIdx.x;
    const T* const a = A + static_cast<long>(blockIdx.x) * cols;
    int8_t* const o = q + static_cast<long>(blockIdx.x) * cols;
    // what an element contributes to the absmax
    auto mag = [&](float v) -> float {
        const float m = fabsf(v);
        if constexpr (THRESH)
            return m >= threshold ? 0.0f : m;
        else
            return m;
    };

    const int groups = cols / kGroup;
    Group<T> held[kKeep];
    float mx = 0.0f;
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i) {
            const int gi = tid + i * kThreads;
            if (gi < groups) {
                held[i] = load_group(a + gi * kGroup);
#pragma unroll
                for (int e = 0; e < kGroup; ++e)
                    mx = fmaxf(mx, mag(static_cast<float>(held[i].e[e])));
            }
        }
        for (int gi = tid + kKeep * kThreads; gi < groups; gi += kThreads) {
            const Group<T> x = load_group(a + gi * kGroup);
#pragma unroll
            for (int e = 0; e < kGroup; ++e)
                mx = fmaxf(mx, mag(static_cast<float>(x.e[e])));
        }
    } else {
        for (int c = tid; c < cols; c += kThreads)
            mx = fmaxf(mx, mag(static_cast<float>(a[c])));
    }
    mx = group_max<kWave>(mx);
    if ((tid & 63) == 0)
        red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (tid == 0)
        row_stats[blockIdx.x] = mx;

    const float scale = 127.0f / mx; // (IEEE division: -fhip-fp32-correctly-rounded-divide-sqrt; unused where mx == 0)
    auto quant = [&](float v) -> uint32_t {
        bool zero = mx == 0.0f;
        if constexpr (THRESH)
            zero = zero || fabsf(v) >= threshold;
        const int i = zero ? 0 : static_cast<int>(rintf(v * scale));
        return static_cast<uint32_t>(i) & 0xFFu;
    };
    auto store_group = [&](const Group<T>& x, int gi) {
        u32x4 w;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            w[d] = quant(static_cast<float>(x.e[4 * d])) | (quant(static_cast<float>(x.e[4 * d + 1])) << 8) |
                   (quant(static_cast<float>(x.e[4 * d + 2])) << 16) | (quant(static_cast<float>(x.e[4 * d + 3])) << 24);
        *reinterpret_cast<u32x4*>(o + gi * kGroup) = w;
    };
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i) {
            const int gi = tid + i * kThreads;
            if (gi < groups)
                store_group(held[i], gi);
        }
        for (int gi = tid + kKeep * kThreads; gi < groups; gi += kThreads)
            store_group(load_group(a + gi * kGroup), gi);
    } else {
        for (int c = tid; c < cols; c += kThreads)
            o[c] = static_cast<int8_t>(quant(static_cast<float>(a[c])));
    }
}

template <typename T> void launch(const void* A, int8_t* q, float* row_stats, long rows, int cols, float threshold, hipStream_t stream) {
    const bool wide = cols % kGroup == 0 && aligned_to(A, 16) && aligned_to(q, 16);
    const dim3 grid(static_cast<unsigned>(rows));
    const T* const a = static_cast<const T*>(A);
    if (threshold > 0.0f) {
        if (wide)
            hipLaunchKernelGGL((int8_quant_kernel<T, true, true>), grid, dim3(kThreads), 0, stream, a, q, row_stats, cols, threshold);
        else
            hipLaunchKernelGGL((int8_quant_kernel<T, false, true>), grid, dim3(kThreads), 0, stream, a, q, row_stats, cols, threshold);
    } else {
        if (wide)
            hipLaunchKernelGGL((int8_quant_kernel<T, true, false>), grid, dim3(kThreads), 0, stream, a, q, row_stats, cols, 0.0f);
        else
            hipLaunchKernelGGL((int8_quant_kernel<T, false, false>), grid, dim3(kThreads), 0, stream, a, q, row_stats, cols, 0.0f);
    }
}

} // namespace

// A [rows, cols] of dtype (0 fp32, 1 fp16, 2 bf16), contiguous -> q int8 [rows, cols], row_stats fp32 [rows]; threshold <= 0: none.
int int8_vectorwise_quant(int dtype, const void* A, int8_t* q, float* row_stats, long rows, long cols, float threshold, hipStream_t stream) {
    if (dtype < 0 || dtype > 2 || rows < 0 || cols < 0 || rows >= (1L << 31) || cols >= (1L << 31) || !(threshold == threshold))
        return kInt8Malformed;
    if (rows == 0 || cols == 0)
        return kInt8Ok;
    if (A == nullptr || q == nullptr || row_stats == nullptr)
        return kInt8Malformed;
    const int c = static_cast<int>(cols);
    if (dtype == 0)
        launch<float>(A, q, row_stats, rows, c, threshold, stream);
    else if (dtype == 1)
        launch<f16>(A, q, row_stats, rows, c, threshold, stream);
    else
        launch<bf16>(A, q, row_stats, rows, c, threshold, stream);
    return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
}

} // namespace bnb
