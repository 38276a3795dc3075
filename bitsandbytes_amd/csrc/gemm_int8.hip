// gemm_int8.hip — the LLM.int8() matmul on the matrix pipe (gfx950): C[m, n] = sum_k A[m, k] * B[n, k], A [M, K] and B [N, K] int8
// row-major, int32 accumulation (v_mfma_i32_16x16x64_i8), with the int32 result or its dequantization as the epilogue; and the
// standalone dequantization kernel of the two-step API.
//
//  * Operand layout: lane (r = lane % 16, g = lane / 16) of an MFMA holds 16 consecutive k bytes of row r - exactly what a row-major
//    [rows, K] int8 matrix holds, for the activations and for the weights alike. No decode table, no transposition, no LDS staging:
//    every operand of every MFMA is ONE 16-byte global load of the lane.
//  * Grid: one workgroup per N tile of 16 TT weight rows (TT <= kMaxTiles from the CU count: gemm_int8_tiles). Its 8 wavefronts split K
//    in chunks of kChunk = 256: wavefront w owns chunks w, w + 8, ... for all TT tiles. Step s (of 4) of a chunk is k
//    [64 s + 16 g, + 16) of the chunk for lane group g: per load instruction a row's 64 bytes are contiguous, over the chunk its 256.
//    Which k a lane's byte j meets inside the MFMA does not matter: both operands are loaded by the same map, and an integer sum
//    does not depend on its order.
//  * Weights stream through a two-stage register ring (the loads of the next (chunk, tile) item fly under the MFMAs of the current
//    one). The activation fragments of a chunk are gathered once per chunk, straight from global memory (L2), and serve every tile.
//  * One weight fragment feeds up to four 16-row M tiles: 64 rows per pass, four MFMAs per weight load; M > 64 runs in row passes
//    inside the launch. Rows of A behind M are zero fragments. A weight row behind N reads the tile's first row, a 16-byte piece
//    behind K the chunk's first piece (both inside the tensor); the piece's activation fragment is zero and the row is never stored.
//  * Combine: the wavefronts leave their int32 partial tiles in LDS; one thread per output element adds them (exact, any order) and
//    applies the epilogue. No workspace, no atomics, no memset.
//
// K % 16 == 0 and K <= 131056 (128 * 128 * K fits int32: no partial sum can overflow); anything else is refused.
#include "bnb_launchers.h"

namespace bnb {

namespace {

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kChunk = 256;    // k per (chunk, tile) item
constexpr int kSteps = 4;      // 64-k MFMA steps per chunk
constexpr int kMaxTiles = 4;   // 16-row weight tiles per workgroup
constexpr int kPassTiles = 4;  // 16-row M tiles per pass
constexpr int kPassRows = 16 * kPassTiles;
constexpr int kMaxK = 131056;
constexpr int kEpiInt32 = 0, kEpiDequant = 1;

struct Int8Args {
    const int8_t* A;
    const int8_t* B;
    void* out;
    const float* row_stats; // [M]
    const float* col_stats; // [N]
    const void* bias;       // [N] or nullptr
    int bias_dtype;
    int M, N, K;
    int TT; // 16-row tiles per workgroup
};

struct Stage {
    i32x4 w[kSteps]; // lane (r, g): k [64 s + 16 g, + 16) of row r of the item's chunk
};

template <int EPI, typename T> __global__ __launch_bounds__(kThreads) void gemm_int8_kernel(const Int8Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* const part = reinterpret_cast<int*>(smem); // [wave][tile][M tile][256]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int K = p.K, TT = p.TT;
    const int n0 = blockIdx.x * 16 * TT;
    const int rows = (p.N - n0) < 16 * TT ? (p.N - n0) : 16 * TT;
    const int tiles = (rows + 15) >> 4;
    const int C = (K + kChunk - 1) / kChunk;
    const int nchunks = wave < C ? (C - wave + kWaves - 1) / kWaves : 0;
    const int nw = C < kWaves ? C : kWaves;

    auto load_stage = [&](int c, int t) -> Stage {
        int rl = 16 * t + r;
        rl = rl < rows ? rl : 0;
        const int tail = K - c * kChunk;
        const int8_t* const src = p.B + static_cast<long>(n0 + rl) * K + c * kChunk;
        Stage st;
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
            const int off = 64 * s + 16 * g;
            st.w[s] = *reinterpret_cast<const i32x4*>(src + (off < tail ? off : 0));
        }
        return st;
    };

    for (int m0 = 0; m0 < p.M; m0 += kPassRows) {
        const int cnt = (p.M - m0) < kPassRows ? (p.M - m0) : kPassRows;
        const int mt = (cnt + 15) >> 4;
        i32x4 acc[kMaxTiles][kPassTiles];
#pragma unroll
        for (int t = 0; t < kMaxTiles; ++t)
#pragma unroll
            for (int j = 0; j < kPassTiles; ++j)
                acc[t][j] = i32x4{0, 0, 0, 0};

        if (nchunks > 0) {
            Stage cur = load_stage(wave, 0);
            for (int ci = 0; ci < nchunks; ++ci) {
                const int c = wave + ci * kWaves;
                const int tail = K - c * kChunk;
                i32x4 af[kPassTiles][kSteps];
#pragma unroll
                for (int j = 0; j < kPassTiles; ++j) {
                    const int m = m0 + 16 * j + r;
#pragma unroll
                    for (int s = 0; s < kSteps; ++s) {
                        af[j][s] = i32x4{0, 0, 0, 0};
                        const int off = 64 * s + 16 * g;
                        if (j < mt && m < p.M && off < tail)
                            af[j][s] = *reinterpret_cast<const i32x4*>(p.A + static_cast<long>(m) * K + c * kChunk + off);
                    }
                }
#pragma unroll
                for (int t = 0; t < kMaxTiles; ++t) {
                    if (t >= tiles) // (wave-uniform)
                        continue;
                    // the next item of the wavefront's list; behind its end the current one again (valid, never used)
                    const bool last_t = t + 1 >= tiles;
                    int nc = last_t ? c + kWaves : c, nt = last_t ? 0 : t + 1;
                    if (nc >= C)
                        nc = c, nt = t;
                    const Stage nxt = load_stage(nc, nt);
#pragma unroll
                    for (int s = 0; s < kSteps; ++s) {
                        if (64 * s >= tail) // (wave-uniform: a step wholly behind the end of the row)
                            continue;
#pragma unroll
                        for (int j = 0; j < kPassTiles; ++j)
                            if (j < mt) // (wave-uniform)
                                acc[t][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[j][s], cur.w[s], acc[t][j], 0, 0, 0);
                    }
                    cur = nxt;
                }
            }
#pragma unroll
            for (int t = 0; t < kMaxTiles; ++t)
#pragma unroll
                for (int j = 0; j < kPassTiles; ++j)
                    if (t < tiles && j < mt)
                        *reinterpret_cast<i32x4*>(part + (((wave * TT + t) * kPassTiles + j) * 256 + lane * 4)) = acc[t][j];
        }
        __syncthreads();

        // one thread per output element. Accumulator layout: lane (ln, lg) holds rows 4 lg ... 4 lg + 3 of the M tile, weight row ln
        for (int idx = tid; idx < cnt * rows; idx += kThreads) {
            const int m = idx / rows, rl = idx - m * rows;
            const int src = ((rl >> 4) * kPassTiles + (m >> 4)) * 256 + ((rl & 15) + 16 * ((m & 15) >> 2)) * 4 + (m & 3);
            int v = part[src];
            for (int w = 1; w < nw; ++w)
                v += part[w * TT * kPassTiles * 256 + src];
            const long n = n0 + rl;
            const long o = static_cast<long>(m0 + m) * p.N + n;
            if constexpr (EPI == kEpiInt32)
                static_cast<int*>(p.out)[o] = v;
            else
                static_cast<T*>(p.out)[o] = static_cast<T>(int8_dequant_f32(v, p.row_stats[m0 + m], p.col_stats[n], p.bias, p.bias_dtype, n));
        }
        __syncthreads();
    }
}

// The two-step API's second step: int32 [M, N] -> T, one thread per element (grid-stride), the epilogue's arithmetic.
template <typename T>
__global__ __launch_bounds__(256) void int8_mm_dequant_kernel(const int* C, const float* row_stats, const float* col_stats, const void* bias,
                                                              int bias_dtype, T* out, long M, int N) {
    const long total = M * N;
    for (long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<long>(gridDim.x) * 256) {
        const long m = i / N, n = i - m * N;
        out[i] = static_cast<T>(int8_dequant_f32(C[i], row_stats[m], col_stats[n], bias, bias_dtype, n));
    }
}

LdsLimit g_lds[4];

template <int EPI, typename T> void launch(const Int8Args& a, int slot, hipStream_t stream) {
    const size_t lds = static_cast<size_t>(kWaves) * a.TT * kPassTiles * 1024;
    ensure_dynamic_lds(g_lds[slot], reinterpret_cast<const void*>(&gemm_int8_kernel<EPI, T>), lds);
    const dim3 grid((a.N + 16 * a.TT - 1) / (16 * a.TT));
    g_last_gemm_kernel = kKernelInt8;
    hipLaunchKernelGGL((gemm_int8_kernel<EPI, T>), grid, dim3(kThreads), lds, stream, a);
}

} // namespace

// 16-row tiles per workgroup: a 4096-row matrix gives every CU one workgroup (MI355X: one tile each), fewer CUs get taller
// tiles up to kMaxTiles, and no more than N holds. The tile selects rows only: no sum depends on it.
int gemm_int8_tiles(int N) {
    const long cus = device_cu_count_or_default();
    long tt = (static_cast<long>(N) + 16 * cus - 1) / (16 * cus);
    tt = tt < 1 ? 1 : tt;
    tt = tt > kMaxTiles ? kMaxTiles : tt;
    const long have = (static_cast<long>(N) + 15) / 16;
    return static_cast<int>(tt < have ? tt : have);
}

bool gemm_int8_k_supported(long K) { return K > 0 && K % 16 == 0 && K <= kMaxK; }

// THE answer to "which kernel does this gemm_int8 call launch": this file's (weight rows over workgroups, K over wavefronts, M in 64-row
// passes: decode) or the LDS-tiled one of gemm_int8_tall.hip (prefill). Tuning knob1 = 100 * cfg: cfg 60 forces this file's kernel, 61 the
// tall one with its built-in tile choice, 62 / 63 its 128 x 128 / 64 x 128 instance; anything else keeps the rule below.
// The rule, measured on MI355X (profiles/int8_bench.txt, us per int8_scaled_mm call, tall vs this file's kernel, spreads <= 0.5 us):
//   M = 64 (tall forced): 4096^2 31.2 vs 14.7, 11008 x 4096 32.9 vs 20.8, 4096 x 11008 80.5 vs 30.8 - behind everywhere;
//   M = 128: 4096^2 31.1 vs 26.2, 4096 x 11008 80.7 vs 56.9 - behind (64 tiles of 64 x 128 on 256 CUs) - but 11008 x 4096 32.8 vs 37.3
//     (172 tiles) ahead;
//   M = 256: 31.1 vs 48.9, 57.5 vs 70.7, 80.7 vs 108.3; M = 512: 32.1 vs 94.4, 75.6 vs 137.3, 87.7 vs 211.6; M = 2048: 79 vs 365, 225 vs
//     539, 191 vs 832 - ahead everywhere.
// M_tall = kTallMinRows = 256 is the smallest benchmarked M at which the tall kernel wins on all three shapes; the one shape that wins at
// 128 differs from the two that lose by its tile count, so 128 ... 255 rows go to the tall kernel where its 64 x 128 tiles give at least
// half of the CUs a workgroup (between 64 and 172 tiles on 256 CUs nothing was measured: the line is drawn at 128).
constexpr long kTallMinRows = 256, kTallMinRowsFilled = 128;
static bool tall_selected(long M, long N) {
    if (M >= kTallMinRows)
        return true;
    return M >= kTallMinRowsFilled && 2 * ((M + 63) / 64) * ((N + 127) / 128) >= device_cu_count_or_default();
}
int gemm_int8_route(long M, long N, long K, int* instance) {
    *instance = 0;
    if (!gemm_int8_k_supported(K))
        return kKernelNone;
    const int cfg = g_mfma_knob1.load(std::memory_order_relaxed) / 100;
    const bool forced_tall = cfg >= 61 && cfg <= 63;
    if (cfg == 60 || (!forced_tall && !tall_selected(M, N)))
        return kKernelInt8;
    const int inst = cfg == 62 ? 1 : cfg == 63 ? 2 : gemm_int8_tall_instance(M, N);
    if (!gemm_int8_tall_serves(inst, M, N)) // (an empty problem, or more tiles than one grid axis carries)
        return kKernelInt8;
    *instance = inst;
    return kKernelInt8Tall;
}

// epilogue 0: out int32 [M, N]; 1: out of out_dtype (0 fp32, 1 fp16, 2 bf16) = dequant(C, row_stats [M], col_stats [N], bias [N] of
// bias_dtype or nullptr). Returns kInt8Ok after the launch (M == 0 or N == 0: nothing to launch), kInt8RefusedK for a K this kernel
// does not serve, kInt8Malformed for anything else outside the preconditions; nothing is launched when it refuses.
int gemm_int8(int epilogue, int out_dtype, const int8_t* A, const int8_t* B, const float* row_stats, const float* col_stats, const void* bias,
              int bias_dtype, void* out, long M, long N, long K, hipStream_t stream) {
    if (M < 0 || N < 0 || M >= (1L << 31) || N >= (1L << 31) || (epilogue != kEpiInt32 && epilogue != kEpiDequant))
        return kInt8Malformed;
    if (!gemm_int8_k_supported(K))
        return kInt8RefusedK;
    if (M == 0 || N == 0)
        return kInt8Ok;
    if (A == nullptr || B == nullptr || out == nullptr || !aligned_to(A, 16) || !aligned_to(B, 16))
        return kInt8Malformed;
    if (epilogue == kEpiDequant && (row_stats == nullptr || col_stats == nullptr || out_dtype < 0 || out_dtype > 2 ||
                                    (bias != nullptr && (bias_dtype < 0 || bias_dtype > 2))))
        return kInt8Malformed;
    int instance = 0;
    if (gemm_int8_route(M, N, K, &instance) == kKernelInt8Tall) {
        gemm_int8_tall(instance, epilogue, out_dtype, A, B, row_stats, col_stats, bias, bias_dtype, out, static_cast<int>(M), static_cast<int>(N),
                       static_cast<int>(K), stream);
        return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
    }
    Int8Args a{};
    a.A = A;
    a.B = B;
    a.out = out;
    a.row_stats = row_stats;
    a.col_stats = col_stats;
    a.bias = bias;
    a.bias_dtype = bias_dtype;
    a.M = static_cast<int>(M);
    a.N = static_cast<int>(N);
    a.K = static_cast<int>(K);
    a.TT = gemm_int8_tiles(a.N);
    if (epilogue == kEpiInt32)
        launch<kEpiInt32, float>(a, 0, stream);
    else if (out_dtype == 0)
        launch<kEpiDequant, float>(a, 1, stream);
    else if (out_dtype == 1)
        launch<kEpiDequant, f16>(a, 2, stream);
    else
        launch<kEpiDequant, bf16>(a, 3, stream);
    return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
}

int int8_mm_dequant(int out_dtype, const int* C, const float* row_stats, const float* col_stats, const void* bias, int bias_dtype, void* out,
                    long M, long N, hipStream_t stream) {
    if (M < 0 || N < 0 || N >= (1L << 31) || out_dtype < 0 || out_dtype > 2 || (bias != nullptr && (bias_dtype < 0 || bias_dtype > 2)))
        return kInt8Malformed;
    if (M == 0 || N == 0)
        return kInt8Ok;
    if (C == nullptr || row_stats == nullptr || col_stats == nullptr || out == nullptr || M > (1L << 40) / N)
        return kInt8Malformed;
    const long blocks = (M * N + 255) / 256;
    const dim3 grid(static_cast<unsigned>(blocks < 16384 ? blocks : 16384));
    const int n = static_cast<int>(N);
    if (out_dtype == 0)
        hipLaunchKernelGGL(int8_mm_dequant_kernel<float>, grid, dim3(256), 0, stream, C, row_stats, col_stats, bias, bias_dtype, static_cast<float*>(out), M, n);
    else if (out_dtype == 1)
        hipLaunchKernelGGL(int8_mm_dequant_kernel<f16>, grid, dim3(256), 0, stream, C, row_stats, col_stats, bias, bias_dtype, static_cast<f16*>(out), M, n);
    else
        hipLaunchKernelGGL(int8_mm_dequant_kernel<bf16>, grid, dim3(256), 0, stream, C, row_stats, col_stats, bias, bias_dtype, static_cast<bf16*>(out), M, n);
    return hipPeekAtLastError() == hipSuccess ? kInt8Ok : kInt8Malformed;
}

} // namespace bnb
