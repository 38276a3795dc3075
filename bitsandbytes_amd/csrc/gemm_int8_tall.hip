// gemm_int8_tall.hip — the LLM.int8() matmul for prefill-sized batches (gfx950): the contract of gemm_int8.hip, C[m, n] = sum_k A[m, k] *
// B[n, k] exact in int32 with the int32 or the dequant epilogue (int8_dequant_f32, the one definition), as a two-dimensional tile with
// both operands shared through LDS. gemm_int8_kernel re-streams its weight rows and re-gathers its activations once per 64-row pass: right
// where the weight stream is the bound (decode), wrong where the arithmetic is (prefill). DESIGN.md §3.18a.
//
//  * Tile: one workgroup of four wavefronts (2 x 2) owns BM x 128 outputs, BM = 128 or 64; wavefront (wm, wn) holds rows
//    [wm BM/2, + BM/2) x columns [64 wn, + 64) as MT x 4 accumulator tiles of 16 x 16 (MT = BM / 32), 64 or 32 int32 registers a lane.
//  * Matrix instruction: v_mfma_i32_16x16x64_i8, the WEIGHT fragment as its first operand: lane (ln, lg) then holds C[m = ln][n = 4 lg + v],
//    v = 0 ... 3 - four consecutive n of one output row, one 16-byte (int32, fp32) or 8-byte (fp16, bf16) store. Operand lane (r, g) holds
//    k [16 g, + 16) of row r of its 16-row subtile, for both operands: 16 consecutive bytes of a row-major row, and the same k-to-lane map on
//    both sides (an integer sum does not depend on its order). 16x16x64 rather than 32x32x32: the same operations per cycle, and the
//    64 x 128 instance's 32 x 64 wavefront block is 2 x 4 tiles, so every fragment read still feeds two (weights) or four (activations)
//    MFMAs; with 32 x 32 tiles it would be 1 x 2 and the weight fragments would feed one.
//  * Operands: global -> LDS by LDS-DMA (lds_dma16) in K tiles of 64 bytes per row, a ring of kStages = 4 stages, three tiles in flight
//    under the MFMAs of the current one. A DMA instruction lands 64 x 16 bytes at consecutive LDS addresses; lane (r, g) of the
//    instruction for subtile t fetches piece g of row 16 t + r. The LDS image of a subtile is therefore its MFMA fragment, lane by lane:
//    lane L reads its fragment with ONE ds_read_b128 at subtile base + 16 L. A wavefront's read covers 1024 consecutive bytes, 16 bytes a
//    lane in lane order - the pattern without bank conflicts whichever way the hardware groups the lanes (any 16 consecutive lanes cover
//    the 64 banks once).
//  * Waits: the DMAs are invisible to the compiler (bnb_common.h), so each wavefront counts its own: (BM + 128) / 64 instructions per
//    stage (LPS). Iteration i waits until at most (kStages - 2) LPS are outstanding (tile i has landed), meets the others at ONE barrier
//    (everybody's share of tile i is in LDS, and everybody is done reading tile i - 1), issues tile i + kStages - 1 into the stage tile
//    i - 1 left, and computes. Tiles past the end of K are issued all the same, with every offset out of range: the count stays uniform.
//  * Edges: a row past M or N and a 16-byte piece past K carry an offset beyond the descriptor's records: zeros land, nothing is
//    fetched. Descriptors start at the workgroup's first row of A and of B (64-bit arithmetic), offsets inside are below 128 * 131056.
//    Stores are guarded per row and per element; vector stores where N % 4 == 0 and `out` is 16-byte aligned.
//  * Order: blockIdx.x walks the M tiles fastest: workgroups that are resident together share a few weight tiles (and, at equal k, the
//    same slices of A) in L2. No split-K, no workspace, no atomics, no memset.
#include "bnb_launchers.h"

namespace bnb {

namespace {

constexpr int kThreads = 256;
constexpr int kBK = 64;    // k (bytes) per row and stage: one MFMA step
constexpr int kStages = 4; // LDS ring
constexpr int kBN = 128;
constexpr int kEpiInt32 = 0;
constexpr uint32_t kOob = 0xFFFFFFF0u; // beyond num_records: zeros, no fetch

struct TallArgs {
    const int8_t* A;
    const int8_t* B;
    void* out;
    const float* row_stats; // [M]
    const float* col_stats; // [N]
    const void* bias;       // [N] or nullptr
    int bias_dtype;
    int M, N, K;
    int tiles_m;
    int vec; // N % 4 == 0 and out 16-byte aligned: one store per accumulator
};

template <int BM, int EPI, typename T> __global__ __launch_bounds__(kThreads) void gemm_int8_tall_kernel(const TallArgs p) {
    constexpr int MT = BM / 32;              // 16-row activation subtiles per wavefront
    constexpr int NT = kBN / 32;             // 16-row weight subtiles per wavefront
    constexpr int SUBS_A = BM / 16;          // subtiles of a stage: activations first, weights behind
    constexpr int SUBS = (BM + kBN) / 16;
    constexpr int LPS = SUBS / 4;            // DMA instructions per wavefront and stage
    constexpr int STAGE = SUBS * 1024;       // bytes
    static_assert(SUBS % 4 == 0 && kStages >= 2, "a stage divides over the four wavefronts");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int M = p.M, N = p.N, K = p.K;
    const int tile_m = blockIdx.x % p.tiles_m, tile_n = blockIdx.x / p.tiles_m;
    const int m0 = tile_m * BM, n0 = tile_n * kBN;
    const int rem_m = M - m0, rem_n = N - n0; // rows and columns from the tile's corner on (>= 1)
    const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));

    // ---- sources: subtiles wave LPS ... + LPS - 1 of every stage are this wavefront's
    const int8_t* const base_a = p.A + static_cast<long>(m0) * K;
    const int8_t* const base_b = p.B + static_cast<long>(n0) * K;
    i32x4 rs[LPS];
    uint32_t voff[LPS];
#pragma unroll
    for (int t = 0; t < LPS; ++t) {
        const int sub = wave * LPS + t;
        const bool is_a = sub < SUBS_A; // (wave-uniform)
        const int row = 16 * (is_a ? sub : sub - SUBS_A) + r;
        const bool valid = row < (is_a ? rem_m : rem_n);
        rs[t] = buffer_rsrc(is_a ? base_a : base_b);
        voff[t] = valid ? static_cast<uint32_t>(row) * static_cast<uint32_t>(K) + static_cast<uint32_t>(16 * g) : kOob;
    }
    auto issue = [&](int i) {
        const int k0 = i * kBK;
        const uint32_t piece = (k0 + 16 * g < K) ? 0u : kOob;
        const uint32_t dst = lds0 + static_cast<uint32_t>((i % kStages) * STAGE + wave * LPS * 1024);
#pragma unroll
        for (int t = 0; t < LPS; ++t)
            lds_dma16(rs[t], dst + static_cast<uint32_t>(t * 1024), voff[t] | piece, static_cast<uint32_t>(k0));
    };

    i32x4 acc[MT][NT];
#pragma unroll
    for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < NT; ++y)
            acc[x][y] = i32x4{0, 0, 0, 0};

    const int ktiles = (K + kBK - 1) / kBK;
#pragma unroll
    for (int s = 0; s < kStages - 1; ++s)
        issue(s);
    for (int i = 0; i < ktiles; ++i) {
        wait_vm<(kStages - 2) * LPS>(); // this wavefront's share of tile i has landed
        __syncthreads();                // everybody's has; everybody is done with tile i - 1
        issue(i + kStages - 1);         // (into the stage of tile i - 1)
        const unsigned char* const st = smem + (i % kStages) * STAGE + lane * 16;
        i32x4 a[MT], b[NT];
#pragma unroll
        for (int x = 0; x < MT; ++x)
            a[x] = *reinterpret_cast<const i32x4*>(st + (wm * MT + x) * 1024);
#pragma unroll
        for (int y = 0; y < NT; ++y)
            b[y] = *reinterpret_cast<const i32x4*>(st + (SUBS_A + wn * NT + y) * 1024);
#pragma unroll
        for (int x = 0; x < MT; ++x)
#pragma unroll
            for (int y = 0; y < NT; ++y)
                acc[x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[y], a[x], acc[x][y], 0, 0, 0);
    }
    wait_vm<0>(); // (the all-out-of-range tail of the ring)
    // The epilogue reads single elements of the accumulators. Seen through, that splits every loop-carried vector into four scalars,
    // and the loop pays ~90 accumulator-register moves per 16 MFMAs to put them together again (seen in the ISA): opaque copies here.
#pragma unroll
    for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < NT; ++y)
            asm volatile("" : "+v"(acc[x][y]));

    // ---- epilogue, straight from the accumulators: lane (r, g) holds C[m0 + mrow + 16 x][n0 + nb + v] of tile (x, y)
    const int mrow = wm * (BM / 2) + r;
    [[maybe_unused]] float rsv[MT];
    if constexpr (EPI != kEpiInt32) {
#pragma unroll
        for (int x = 0; x < MT; ++x)
            rsv[x] = (mrow + 16 * x < rem_m) ? p.row_stats[static_cast<long>(m0) + mrow + 16 * x] : 0.0f;
    }
#pragma unroll
    for (int y = 0; y < NT; ++y) {
        const int nb = wn * (kBN / 2) + 16 * y + 4 * g;
        const long n = static_cast<long>(n0) + nb;
        if (nb >= rem_n)
            continue;
        const bool whole = p.vec != 0 && nb + 3 < rem_n;
        // column statistics and bias: once per lane and tile column, the bias widened to fp32 (exact) in a lane-local table that
        // int8_dequant_f32 reads as an fp32 bias
        [[maybe_unused]] float cs[4], bl[4];
        if constexpr (EPI != kEpiInt32) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const bool in = nb + v < rem_n;
                cs[v] = in ? p.col_stats[n + v] : 0.0f;
                bl[v] = 0.0f;
                if (in && p.bias != nullptr)
                    bl[v] = p.bias_dtype == 0   ? static_cast<const float*>(p.bias)[n + v]
                            : p.bias_dtype == 1 ? static_cast<float>(static_cast<const f16*>(p.bias)[n + v])
                                                : static_cast<float>(static_cast<const bf16*>(p.bias)[n + v]);
            }
        }
#pragma unroll
        for (int x = 0; x < MT; ++x) {
            const int m = mrow + 16 * x;
            if (m >= rem_m)
                continue;
            const long o = (static_cast<long>(m0) + m) * N + n;
            if constexpr (EPI == kEpiInt32) {
                int* const dst = static_cast<int*>(p.out) + o;
                if (whole) {
                    *reinterpret_cast<i32x4*>(dst) = acc[x][y];
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        if (nb + v < rem_n)
                            dst[v] = acc[x][y][v];
                }
            } else {
                float f[4];
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    f[v] = p.bias != nullptr ? int8_dequant_f32(acc[x][y][v], rsv[x], cs[v], bl, 0, v)
                                             : int8_dequant_f32(acc[x][y][v], rsv[x], cs[v], nullptr, 0, 0);
                T* const dst = static_cast<T*>(p.out) + o;
                if (whole) {
                    if constexpr (std::is_same_v<T, float>)
                        *reinterpret_cast<f32x4*>(dst) = f32x4{f[0], f[1], f[2], f[3]};
                    else
                        *reinterpret_cast<u32x2*>(dst) = u32x2{pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3])};
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        if (nb + v < rem_n)
                            dst[v] = static_cast<T>(f[v]);
                }
            }
        }
    }
}

template <int BM, int EPI, typename T> void launch(const TallArgs& a, long tiles, hipStream_t stream) {
    constexpr size_t lds = static_cast<size_t>(kStages) * (BM + kBN) * kBK; // 64 KiB / 48 KiB: two / three workgroups a CU
    static_assert(lds <= 64 * 1024, "inside the default dynamic LDS limit");
    g_last_gemm_kernel = kKernelInt8Tall;
    hipLaunchKernelGGL((gemm_int8_tall_kernel<BM, EPI, T>), dim3(static_cast<unsigned>(tiles)), dim3(kThreads), lds, stream, a);
}

template <int BM> void launch_instance(const TallArgs& a, long tiles, int epilogue, int out_dtype, hipStream_t stream) {
    if (epilogue == kEpiInt32)
        launch<BM, 0, float>(a, tiles, stream);
    else if (out_dtype == 0)
        launch<BM, 1, float>(a, tiles, stream);
    else if (out_dtype == 1)
        launch<BM, 1, f16>(a, tiles, stream);
    else
        launch<BM, 1, bf16>(a, tiles, stream);
}

long tall_tiles(int instance, long M, long N) {
    const long bm = instance == 1 ? 128 : 64;
    return ((M + bm - 1) / bm) * ((N + kBN - 1) / kBN);
}

} // namespace

// The tile instance of a problem: 1 = 128 x 128 where that gives every CU a workgroup, else 2 = 64 x 128 (M = 512 on a 4096-row weight:
// 256 tiles instead of 128). The tile selects rows and columns only: no sum depends on it.
int gemm_int8_tall_instance(long M, long N) { return tall_tiles(1, M, N) >= device_cu_count_or_default() ? 1 : 2; }

// (one grid axis carries every tile)
bool gemm_int8_tall_serves(int instance, long M, long N) { return M >= 1 && N >= 1 && tall_tiles(instance, M, N) <= 0x7FFFFFFFL; }

// gemm_int8's launch for the tall kernel: the caller (gemm_int8, csrc/gemm_int8.hip) has checked the arguments and the route.
void gemm_int8_tall(int instance, int epilogue, int out_dtype, const int8_t* A, const int8_t* B, const float* row_stats, const float* col_stats,
                    const void* bias, int bias_dtype, void* out, int M, int N, int K, hipStream_t stream) {
    TallArgs a{};
    a.A = A;
    a.B = B;
    a.out = out;
    a.row_stats = row_stats;
    a.col_stats = col_stats;
    a.bias = bias;
    a.bias_dtype = bias_dtype;
    a.M = M;
    a.N = N;
    a.K = K;
    const long bm = instance == 1 ? 128 : 64;
    a.tiles_m = static_cast<int>((static_cast<long>(M) + bm - 1) / bm);
    a.vec = (N % 4 == 0 && aligned_to(out, 16)) ? 1 : 0;
    const long tiles = tall_tiles(instance, M, N);
    if (instance == 1)
        launch_instance<128>(a, tiles, epilogue, out_dtype, stream);
    else
        launch_instance<64>(a, tiles, epilogue, out_dtype, stream);
}

} // namespace bnb
