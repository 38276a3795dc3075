// int8_outlier.hip — the 16-bit half of the LLM.int8() mixed decomposition (gfx950), in place on the result of the scaled int8 matmul:
//     out[m, n] = T(float(out[m, n]) + sum over flagged c of A[m, c] * Wd[n, c]),   Wd[n, c] = T((float(CB[n, c]) * SCB[n]) * (1 / 127))
// with the flagged columns given as the bitmask int8_vectorwise_quant_mask leaves on the device (bit c % 32 of word c / 32). Their
// number is never known on the host: the grid depends on M and N alone, and every workgroup derives its own work from the mask.
//
//  * Grid: x = 64-column strips of out (one 16-wide N tile per wavefront, four wavefronts), y = 64-row passes over M (four 16-row M
//    tiles per pass; more passes than the grid carries are walked in the launch).
//  * The mask is read in chunks of 256 words (8192 columns), one word per thread. popcount, a prefix sum over the workgroup (shuffles
//    inside a wavefront, the four totals through LDS), and each thread writes the columns of its set bits, as 16-bit offsets from the
//    chunk's first column, into a list in LDS at its prefix: the list is sorted, and its 16 KiB hold a chunk with every bit set. The
//    last group of 32 is padded with a sentinel that reads as zeros.
//  * The list is consumed 32 columns per v_mfma_f32_16x16x32_{f16,bf16} step. Lane (r = lane % 16, g = lane / 16) holds list entries
//    8 g ... 8 g + 7 of the group for both operands. Wavefront j gathers the A fragment of M tile j (row r of the tile, eight 2-byte
//    loads) and leaves it in LDS as the 16 bytes the MFMA takes: the [64 x 32] slice of A is gathered once and read by all four
//    wavefronts. The weight bytes are gathered by the lane that needs them (row n of the wavefront's tile, eight byte loads),
//    converted and scaled in registers with the roundings of the composed path (two fp32 products, then T), and feed four MFMAs.
//    The A slices alternate between two LDS buffers: one barrier per step.
//  * Rows behind M and sentinel columns are zero fragments; a weight row behind N reads the strip's first row and is never stored.
//  * Epilogue: out is read, the fp32 accumulator added, rounded once to T. A workgroup that found no set bit leaves without
//    touching out (adding +0 would turn a -0 into +0).
//
// K % 16 == 0 and K <= 131056 (the int8 matmul's own range: the layer never gets here otherwise); bits at and behind K are ignored.
#include "bnb_launchers.h"

namespace bnb {

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kStrip = 16 * kWaves;           // columns of out per workgroup
constexpr int kPassTiles = 4;                 // 16-row M tiles per pass: wavefront j gathers tile j
constexpr int kPassRows = 16 * kPassTiles;
constexpr int kChunkWords = kThreads;         // mask words per chunk: one per thread
constexpr int kChunkCols = 32 * kChunkWords;  // 8192: a 16-bit list entry holds any offset, and 0xFFFF is free for the sentinel
constexpr int kStep = 32;                     // columns per MFMA step
constexpr uint32_t kSentinel = 0xFFFFu;
constexpr int kMaxPasses = 1024;              // grid y
constexpr long kMaxK = 131056;
static_assert(kPassTiles == kWaves, "wavefront j gathers the A fragment of M tile j");
static_assert(kChunkCols % kStep == 0 && kChunkCols <= 0xFFFF, "the padded list fits its array, and the sentinel is no offset");

struct OutlierArgs {
    const void* A;         // [M, K] of T
    const int8_t* CB;      // [N, K]
    const float* SCB;      // [N]
    const uint32_t* mask;  // [ceil(K / 32)]
    void* out;             // [M, N] of T
    int M, N, K;
};

template <typename T> __global__ __launch_bounds__(kThreads) void int8_outlier_addmm_kernel(const OutlierArgs p) {
    __shared__ __attribute__((aligned(16))) uint16_t list[kChunkCols];
    __shared__ u32x4 afrag[2][kPassTiles][64];
    __shared__ int wave_total[kWaves];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int K = p.K;
    const T* const A = static_cast<const T*>(p.A);
    T* const out = static_cast<T*>(p.out);
    const int words = (K + 31) >> 5;
    const int n0 = blockIdx.x * kStrip;
    const int n = n0 + 16 * wave + r;                                        // the weight row of this lane's B fragment
    const int8_t* const wrow = p.CB + static_cast<long>(n < p.N ? n : n0) * K;
    const float scb = p.SCB[n < p.N ? n : n0];

    for (long m0 = static_cast<long>(blockIdx.y) * kPassRows; m0 < p.M; m0 += static_cast<long>(gridDim.y) * kPassRows) {
        const long tiles_left = (p.M - m0 + 15) >> 4;
        const int mt = tiles_left < kPassTiles ? static_cast<int>(tiles_left) : kPassTiles;
        const long am = m0 + 16 * wave + r;                                  // the row of A this lane gathers
        const T* const arow = A + (am < p.M ? am : m0) * K;
        f32x4 acc[kPassTiles];
#pragma unroll
        for (int j = 0; j < kPassTiles; ++j)
            acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        bool any = false;

        for (int w0 = 0; w0 < words; w0 += kChunkWords) {
            // ---- the chunk's set bits -> a sorted column list in LDS
            uint32_t bits = w0 + tid < words ? p.mask[w0 + tid] : 0u;
            if (32 * (w0 + tid) + 32 > K)                                    // (the last word of a K that is 16 mod 32, or a word behind K)
                bits &= 32 * (w0 + tid) < K ? (1u << (K & 31)) - 1u : 0u;
            const int mine = __builtin_popcount(bits);
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off, kWave);
                incl += lane >= off ? up : 0;
            }
            if (lane == 63)
                wave_total[wave] = incl;
            __syncthreads();
            int at = incl - mine, count = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                at += w < wave ? wave_total[w] : 0;
                count += wave_total[w];
            }
            if (count == 0) {      // (workgroup-uniform)
                __syncthreads();   // wave_total is rewritten by the next chunk
                continue;
            }
            any = true;
            for (uint32_t b = bits; b != 0; b &= b - 1)
                list[at++] = static_cast<uint16_t>(32 * tid + __builtin_ctz(b));
            const int steps = (count + kStep - 1) / kStep;
            if (tid < kStep && count + tid < steps * kStep)
                list[count + tid] = static_cast<uint16_t>(kSentinel);
            __syncthreads();

            // ---- 32 listed columns per MFMA step
            const int cbase = 32 * w0;
            for (int s = 0; s < steps; ++s) {
                const u32x4 packed = *reinterpret_cast<const u32x4*>(list + s * kStep + 8 * g); // entries 8 g ... 8 g + 7
                int col[8];
                bool real[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t e = (packed[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                    real[i] = e != kSentinel;
                    col[i] = real[i] ? cbase + static_cast<int>(e) : 0;
                }
                // the weight fragment of this lane: eight byte loads, in flight under the gather of A
                int8_t wq[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    wq[i] = wrow[col[i]];
                if (wave < mt) {   // (wave-uniform) the A fragment of M tile `wave`
                    T av[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        av[i] = arow[col[i]];
                    u32x4 f;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const uint32_t lo = __builtin_bit_cast(uint16_t, av[2 * d]), hi = __builtin_bit_cast(uint16_t, av[2 * d + 1]);
                        f[d] = (real[2 * d] && am < p.M ? lo : 0u) | ((real[2 * d + 1] && am < p.M ? hi : 0u) << 16);
                    }
                    afrag[s & 1][wave][lane] = f;
                }
                u32x4 wf;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    float v[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float scaled = rounded_f32(rounded_f32(static_cast<float>(wq[2 * d + h]) * scb) * 7.874015718698502e-3f);
                        v[h] = real[2 * d + h] ? scaled : 0.0f;
                    }
                    wf[d] = pack2<T>(v[0], v[1]);
                }
                __syncthreads();   // the slice of this step is in LDS; the buffer of step s - 1 is free again after the NEXT barrier
#pragma unroll
                for (int j = 0; j < kPassTiles; ++j)
                    if (j < mt)    // (workgroup-uniform)
                        acc[j] = Mma16x16x32<T>::run(afrag[s & 1][j][lane], wf, acc[j]);
            }
            __syncthreads();       // the list and both slices are read out before the next chunk rewrites them
        }
        if (!any)
            continue;

        // accumulator layout: lane (r, g) holds rows 4 g ... 4 g + 3 of M tile j, column r of the wavefront's N tile
        if (n < p.N) {
#pragma unroll
            for (int j = 0; j < kPassTiles; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long m = m0 + 16 * j + 4 * g + i;
                    if (j < mt && m < p.M) {
                        T* const o = out + m * p.N + n;
                        *o = static_cast<T>(static_cast<float>(*o) + acc[j][i]);
                    }
                }
        }
    }
}

} // namespace

// dtype 1 fp16 / 2 bf16 (of A and out). Returns kInt8Ok after the launch (M == 0 or N == 0: nothing to launch), kInt8RefusedK for a K
// outside the int8 matmul's range, kInt8Malformed for anything else outside the preconditions; nothing is launched when it refuses.
int int8_outlier_addmm(int dtype, const void* A, const int8_t* CB, const float* SCB, const uint32_t* mask, void* out, long M, long N, long K,
                       hipStream_t stream) {
    if ((dtype != 1 && dtype != 2) || M < 0 || N < 0 || M >= (1L << 31) || N >= (1L << 31))
        return kInt8Malformed;
    if (K <= 0 || K % 16 != 0 || K > kMaxK)
        return kInt8RefusedK;
    if (M == 0 || N == 0)
        return kInt8Ok;
    if (A == nullptr || CB == nullptr || SCB == nullptr || mask == nullptr || out == nullptr || !aligned_to(A, 2) || !aligned_to(out, 2) ||
        !aligned_to(SCB, 4) || !aligned_to(mask, 4))
        return kInt8Malformed;
    const OutlierArgs a{A, CB, SCB, mask, out, static_cast<int>(M), static_cast<int>(N), static_cast<int>(K)};
    const long passes = (M + kPassRows - 1) / kPassRows;
    const dim3 grid(static_cast<unsigned>((N + kStrip - 1) / kStrip), static_cast<unsigned>(passes < kMaxPasses ? passes : kMaxPasses));
    if (dtype == 1)
        hipLaunchKernelGGL(int8_outlier_addmm_kernel<f16>, grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(int8_outlier_addmm_kernel<bf16>, grid, dim3(kThreads), 0, stream, a);
    return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
}

} // namespace bnb
