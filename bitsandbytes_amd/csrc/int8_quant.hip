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
//  * MASK (int8_vectorwise_quant_mask: THRESH plus the outlier columns as a bitmask on the device, bit c % 32 of word c / 32, nothing
//    read on the host): three launches in stream order. (1) a small kernel clears the mask (no memset: the sequence is captured in
//    graphs). (2) The quantize kernel ORs its row's outlier bits into the mask while it looks for the absmax - the wide instance per
//    thread (a group of 16 elements is half a mask word), the narrow one per wavefront (one ballot is two mask words) - with a vector
//    atomic for non-zero patterns only: outliers are rare, and an OR across rows does not depend on its order. A is still read once.
//    (3) With more than one row, a second small kernel walks the finished mask and writes zero bytes into the flagged columns of q in
//    every row (with one row the quantize kernel's own zeros are the whole column).
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

template <typename T, bool WIDE, bool THRESH, bool MASK = false>
__global__ __launch_bounds__(kThreads) void int8_quant_kernel(const T* A, int8_t* q, float* row_stats, int cols, float threshold, uint32_t* mask = nullptr) {
    static_assert(THRESH || !MASK, "the mask is the threshold's");
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
    // a group's share of the absmax; MASK: its 16 outlier bits go into their half of mask word gi / 2
    auto scan_group = [&](const Group<T>& x, int gi) {
        uint32_t hit = 0;
#pragma unroll
        for (int e = 0; e < kGroup; ++e) {
            const float v = static_cast<float>(x.e[e]);
            mx = fmaxf(mx, mag(v));
            if constexpr (MASK)
                hit |= (fabsf(v) >= threshold ? 1u : 0u) << e;
        }
        if constexpr (MASK)
            if (hit != 0)
                atomicOr(mask + (gi >> 1), hit << (16 * (gi & 1)));
    };
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < kKeep; ++i) {
            const int gi = tid + i * kThreads;
            if (gi < groups) {
                held[i] = load_group(a + gi * kGroup);
                scan_group(held[i], gi);
            }
        }
        for (int gi = tid + kKeep * kThreads; gi < groups; gi += kThreads)
            scan_group(load_group(a + gi * kGroup), gi);
    } else if constexpr (MASK) {
        // every lane takes every step (the ballot wants the whole wavefront): the 64 columns of a wavefront's step are two mask words
        for (int base = 0; base < cols; base += kThreads) {
            const int c = base + tid;
            const float v = c < cols ? static_cast<float>(a[c]) : 0.0f;
            mx = fmaxf(mx, mag(v));
            const uint64_t hit = __ballot(fabsf(v) >= threshold);
            const uint32_t word = static_cast<uint32_t>((tid & 32) ? hit >> 32 : hit);
            if ((tid & 31) == 0 && word != 0) // (a set bit is a column below cols: the word is inside the mask)
                atomicOr(mask + (c >> 5), word);
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

// MASK, launches (1) and (3)
__global__ __launch_bounds__(kThreads) void int8_mask_clear_kernel(uint32_t* mask, int words) {
    const int w = blockIdx.x * kThreads + threadIdx.x;
    if (w < words)
        mask[w] = 0;
}

// One thread per mask word (grid x), the rows dealt over grid y: a zero byte per (row, flagged column). An empty mask writes nothing.
__global__ __launch_bounds__(kThreads) void int8_zero_masked_columns_kernel(const uint32_t* mask, int8_t* q, long rows, int cols) {
    const int word = blockIdx.x * kThreads + threadIdx.x;
    if (word >= (cols + 31) / 32)
        return;
    for (uint32_t w = mask[word]; w != 0; w &= w - 1) {
        const int c = 32 * word + __builtin_ctz(w);
        if (c < cols)
            for (long r = blockIdx.y; r < rows; r += gridDim.y)
                q[r * cols + c] = 0;
    }
}

template <typename T>
void launch(const void* A, int8_t* q, float* row_stats, uint32_t* mask, long rows, int cols, float threshold, hipStream_t stream) {
    const bool wide = cols % kGroup == 0 && aligned_to(A, 16) && aligned_to(q, 16);
    const dim3 grid(static_cast<unsigned>(rows));
    const T* const a = static_cast<const T*>(A);
    if (mask != nullptr) {
        const int words = (cols + 31) / 32;
        const dim3 word_blocks((words + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(int8_mask_clear_kernel, word_blocks, dim3(kThreads), 0, stream, mask, words);
        if (rows == 0)
            return;
        if (wide)
            hipLaunchKernelGGL((int8_quant_kernel<T, true, true, true>), grid, dim3(kThreads), 0, stream, a, q, row_stats, cols, threshold, mask);
        else
            hipLaunchKernelGGL((int8_quant_kernel<T, false, true, true>), grid, dim3(kThreads), 0, stream, a, q, row_stats, cols, threshold, mask);
        if (rows > 1)
            hipLaunchKernelGGL(int8_zero_masked_columns_kernel, dim3(word_blocks.x, static_cast<unsigned>(rows < 256 ? rows : 256)), dim3(kThreads), 0,
                               stream, mask, q, rows, cols);
    } else if (threshold > 0.0f) {
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
        launch<float>(A, q, row_stats, nullptr, rows, c, threshold, stream);
    else if (dtype == 1)
        launch<f16>(A, q, row_stats, nullptr, rows, c, threshold, stream);
    else
        launch<bf16>(A, q, row_stats, nullptr, rows, c, threshold, stream);
    return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
}

// The same with threshold > 0 and mask uint32 [ceil(cols / 32)]: bit c % 32 of word c / 32 is set iff some row has |A[r, c]| >= threshold;
// bits at and behind cols are zero; q is zero in every flagged column of every row. Nothing is read on the host.
int int8_vectorwise_quant_mask(int dtype, const void* A, int8_t* q, float* row_stats, uint32_t* mask, long rows, long cols, float threshold,
                               hipStream_t stream) {
    if (dtype < 0 || dtype > 2 || rows < 0 || cols < 0 || rows >= (1L << 31) || cols >= (1L << 31) || !(threshold > 0.0f))
        return kInt8Malformed;
    if (cols == 0)
        return kInt8Ok;
    if (mask == nullptr || (rows > 0 && (A == nullptr || q == nullptr || row_stats == nullptr)))
        return kInt8Malformed;
    const int c = static_cast<int>(cols);
    if (dtype == 0)
        launch<float>(A, q, row_stats, mask, rows, c, threshold, stream);
    else if (dtype == 1)
        launch<f16>(A, q, row_stats, mask, rows, c, threshold, stream);
    else
        launch<bf16>(A, q, row_stats, mask, rows, c, threshold, stream);
    return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
}

} // namespace bnb
