// gemm4_experts_mfma.hip — expert-indexed fused 4-bit matmul on the matrix pipe, for batched MoE decode (gfx950, family 12).
//
//     y[p, :] = x_row(p) @ dequant(W[ids[p]]).T (+ bias[ids[p], :])          p < P = T * S (token, slot) pairs
//
// The operands, the id handling and the three epilogues are those of gemm4_experts.hip (family 9); what differs is how many pairs
// one pass over an expert's weights serves: SIXTEEN, the rows of one v_mfma_f32_16x16x32 batch, instead of four rows of VALU FMAs.
//
//  * Grid (N tile, expert). Every wavefront scans the id list itself (one 64-lane load + ballot per 64 ids, wave-uniform, no LDS, no
//    barrier) and takes its expert's pairs in ascending pair order, 16 per pass: lane (ln, *) keeps pair ln of the pass in a register.
//    A workgroup whose expert nobody selected leaves behind that scan: no weight, absmax or table byte was requested.
//  * K split as in gemm4_mfma_sm.hip: wavefront w of 8 owns the 256-k chunks w, w + 8, ... of K for ALL 16-row weight tiles of the
//    workgroup (up to kMaxTiles) and keeps the chunk's activation fragments (8 MFMA operands, 32 VGPRs) in registers while it walks
//    the tiles. The fragments are gathered straight from the rows x[p / S] or x[p] of the lane's pair: the k order inside a chunk is
//    the kernel's own, so every fragment is one contiguous 16-byte load. Rows behind the pair count repeat the pass's last pair
//    (a valid row; their results are never stored).
//  * Weights: lane 4 r + pp loads 16-byte piece pp of row r's 64 bytes (a lane quad covers 64 contiguous bytes of one row; two loads
//    per chunk), a two-stage register ring (the next item's loads fly under the current item's decode). One 1-KiB tile private to the
//    wavefront transposes the pieces to MFMA shape, v_permlane32_swap regroups them so that every MFMA consumes k from ONE 64-k
//    sub-block, one LDS look-up per packed byte (byte -> two 16-bit code values, 64 lane-private copies, address by v_perm_b32)
//    decodes them. The fp32 partial tile of a sub-block is multiplied by the exact fp32 block scale (plain, or nested_scale over the
//    flat block index) as it is accumulated. A chunk cut short by the end of the row (K % 64 == 0) skips the MFMAs of its missing
//    sub-blocks, wave-uniformly; the loads that would reach behind the row are redirected to the chunk's first piece.
//  * The wavefronts' partial tiles meet once in LDS and are added in ascending wavefront order by one thread per (pair, output
//    column), which applies the epilogue of family 9 in family 9's arithmetic. One output element's sum: per wavefront, its chunks in
//    ascending order, in a chunk the sub-blocks in ascending order (two chained MFMAs from zero, then acc = fma(scale, part, acc)),
//    then wavefront 0 + 1 + ... in order - a function of K alone: not of the pass, the row of the pass, the other pairs, the tile
//    height, the CU count or the ids. No atomics, no workspace, no memset.
//
// Ids outside [0, E) select nothing; the expert-0 workgroups write zeros to those rows.
#include "bnb_launchers.h"

namespace bnb {

namespace {

constexpr int kLut = 65536;  // 256 entries x 64 lane-private copies x 4 B
constexpr int kCode2 = 1024; // nested absmax code (256 floats)
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kPassRows = 16;     // pairs of one expert served by one pass over its weights: the rows of one MFMA batch
constexpr int kChunk = 256;       // k per item: four 64-k sub-blocks, two MFMAs each
constexpr int kMaxTiles = 8;      // 16-row weight tiles per workgroup (their accumulators live in registers)
constexpr int kWaveLds = 1024 + 256; // per wavefront: the transposition tile and the scale tile
constexpr int kPairsLds = 64;     // the pass's pair list for the epilogue
constexpr int kEpiPlain = 0, kEpiGated = 1, kEpiScale = 2;

struct MfmaExpertArgs {
    const void* A;
    const uint8_t* B;
    const float* absmax;
    const uint8_t* absmax8;
    const float* absmax_code;
    const float* absmax_offset;
    const void* bias;
    const void* ids;
    void* out;
    const void* row_scale; // kEpiScale: [P] fp32 (scale_f32) or T
    int scale_f32;
    int up_delta, col_step, n0_shift; // kEpiGated: the local -> global row map of gemm4_experts.hip
    int P, S, E, N, K, bs_shift;
    int a_per_slot; // 1: one activation row per pair, 0: one per token (pair / S)
    int idx64;
    int fp4;
    int TT; // 16-row tiles per workgroup
};

__device__ __forceinline__ long long expert_id(const void* ids, int idx64, int i) {
    return idx64 ? static_cast<const long long*>(ids)[i] : static_cast<long long>(static_cast<const int*>(ids)[i]);
}

// The next up to 16 pairs of expert e at or behind `pos`, in ascending order; `pos` moves behind the last one taken. The count is
// wave-uniform (ballot); pair j of the pass lands in `mine` of the lanes with lane % 16 == j, and the lanes behind the count hold the
// last pair taken. Every wavefront of the workgroup reads the same list: the caller's control flow is uniform over the workgroup.
__device__ __forceinline__ int next_pairs16(const void* ids, int idx64, int P, int e, int lane, int& pos, int& mine) {
    int found = 0;
    while (pos < P && found < kPassRows) {
        const int idx = pos + lane;
        const bool hit = idx < P && expert_id(ids, idx64, idx) == static_cast<long long>(e);
        unsigned long long mask = __ballot(hit);
        int last = pos;
        while (mask != 0 && found < kPassRows) {
            last = pos + __builtin_ctzll(mask);
            mine = (lane & 15) >= found ? last : mine;
            ++found;
            mask &= mask - 1;
        }
        pos = (mask != 0) ? last + 1 : pos + 64;
    }
    pos = __builtin_amdgcn_readfirstlane(pos);
    return __builtin_amdgcn_readfirstlane(found);
}

struct Stage {
    u32x4 w[2];  // lane (r, pp): k [128 h + 32 pp, + 32) of row r of the tile's chunk
    uint32_t s;  // lane (r, pp): the fp32 absmax of 64-k sub-block pp of row r's chunk (nested: its 8-bit code)
    uint32_t s2; // nested: the second-level absmax of that block
};

// One pass: the cnt <= 16 pairs held in `mine` against the workgroup's tile, all K.
template <typename T, bool NESTED, int EPI>
__device__ __forceinline__ void run_pass(const MfmaExpertArgs& p, unsigned char* smem, int mine, int cnt, int e, int n0, int rows, int tid) {
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane >> 2, pp = lane & 3;   // weight-load roles: row r of the 16-row tile, 16-byte piece pp of its 64 bytes
    const int ln = lane & 15, lg = lane >> 4; // MFMA roles: row / column ln, k group lg
    const int K = p.K;
    const int C = (K + kChunk - 1) / kChunk;
    const int nchunks = wave < C ? (C - wave + kWaves - 1) / kWaves : 0;
    const int tiles = (rows + 15) >> 4;
    const float* const code2 = reinterpret_cast<const float*>(smem + kLut);
    unsigned char* const scratch = smem + kLut + kCode2 + wave * kWaveLds;
    u32x4* const tile = reinterpret_cast<u32x4*>(scratch);
    float* const stile = reinterpret_cast<float*>(scratch + 1024);
    int* const pairs = reinterpret_cast<int*>(smem + kLut + kCode2 + kWaves * kWaveLds);
    float* const part = reinterpret_cast<float*>(smem + kLut + kCode2 + kWaves * kWaveLds + kPairsLds); // [wave][tile][256]
    const float offset = NESTED ? p.absmax_offset[0] : 0.0f;
    const long row_base = static_cast<long>(e) * p.N + n0; // first row of the tile in the flat [E * N, K] matrix
    const long gate_base = static_cast<long>(e) * p.N + (n0 >> p.n0_shift);
    // gated: local row rl = 2 c + h is the gate (h = 0) or up (h = 1) row of the tile's output column c (gemm4_experts.hip)
    auto global_row = [&](int rl) -> long {
        if constexpr (EPI == kEpiGated)
            return gate_base + (rl & 1) * p.up_delta + (rl >> 1) * p.col_step;
        else
            return row_base + rl;
    };
    if (wave == 0 && lane < kPassRows)
        pairs[lane] = mine;

    // item (chunk c, tile t): every address is inside the tensors - a tile row behind the workgroup's rows reads its first row, a
    // piece or sub-block behind the end of the row reads the chunk's first one; neither is ever stored or multiplied
    auto load_stage = [&](int c, int t) -> Stage {
        int rl = 16 * t + r;
        rl = rl < rows ? rl : 0;
        const long grow = global_row(rl);
        const int tail = K - c * kChunk;
        const uint8_t* const src = p.B + grow * (K >> 1) + c * (kChunk / 2);
        Stage st;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            st.w[h] = *reinterpret_cast<const u32x4*>(src + (128 * h + 32 * pp < tail ? 64 * h + 16 * pp : 0));
        const long blk = (grow * K + c * kChunk + (64 * pp < tail ? 64 * pp : 0)) >> p.bs_shift;
        if constexpr (NESTED) {
            st.s = p.absmax8[blk];
            st.s2 = __builtin_bit_cast(uint32_t, p.absmax[blk >> 8]);
        } else {
            st.s = __builtin_bit_cast(uint32_t, p.absmax[blk]);
            st.s2 = 0;
        }
        return st;
    };

    // Where lane (r, pp) puts its 16 bytes, and where lane (ln, lg) finds those of lane (r = ln, pp = lg): conflict-free both ways
    // (gemm4_mfma_rt.hip)
    const int wslot = 16 * pp + (r ^ (2 * pp));
    const int rslot = 16 * lg + (ln ^ (2 * lg));
    const uint32_t lane4 = static_cast<uint32_t>(lane) * 4u;

    // nb = 64-k sub-blocks of the item's chunk (4; fewer in the last chunk of a K % 256 != 0 row)
    auto compute = [&](const Stage& s, f32x4& accv, const u32x4 (&af)[8], int nb) {
        float sc;
        if constexpr (NESTED)
            sc = nested_scale(code2[s.s], __builtin_bit_cast(float, s.s2), offset);
        else
            sc = __builtin_bit_cast(float, s.s);
        stile[lane] = sc; // lane 4 r + pp: sub-block pp of row r; lane (ln, lg) reads row ln's four
        u32x4 wt[2];
        tile[wslot] = s.w[0];
        wt[0] = tile[rslot];
        tile[wslot] = s.w[1];
        wt[1] = tile[rslot];
        float scale[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            scale[b] = stile[4 * ln + b];
        // regroup: dwords 0 / 1 (2 / 3) of every lane group belong to sub-block 2 h (2 h + 1); step 4 h + 2 a + b of lane (ln, lg)
        // is then 8 k from 128 h + 64 a + 8 b + 32 (lg & 1) + 16 (lg >> 1) - the order the activation fragments are gathered in
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const auto s02 = __builtin_amdgcn_permlane32_swap(wt[h][0], wt[h][2], false, false);
            const auto s13 = __builtin_amdgcn_permlane32_swap(wt[h][1], wt[h][3], false, false);
            wt[h][0] = s02[0];
            wt[h][2] = s02[1];
            wt[h][1] = s13[0];
            wt[h][3] = s13[1];
        }
        u32x4 bf[8];
#pragma unroll
        for (int sidx = 0; sidx < 8; ++sidx) {
            const uint32_t w = wt[sidx >> 2][sidx & 3];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) // {lane offset, weight byte qq, 0, 0}: byte * 256 + lane * 4
                bf[sidx][qq] = *reinterpret_cast<const uint32_t*>(smem + __builtin_amdgcn_perm(w, lane4, 0x0C0C0400u + (qq << 8)));
        }
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            if (blk >= nb) // (wave-uniform)
                continue;
            f32x4 sub = {0.f, 0.f, 0.f, 0.f};
            sub = Mma16x16x32<T>::run(af[2 * blk], bf[2 * blk], sub);
            sub = Mma16x16x32<T>::run(af[2 * blk + 1], bf[2 * blk + 1], sub);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
                accv[qq] = fmaf(scale[blk], sub[qq], accv[qq]);
        }
    };

    f32x4 acc[kMaxTiles];
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t)
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nchunks > 0) {
        const T* const arow = static_cast<const T*>(p.A) + static_cast<long>(p.a_per_slot ? mine : mine / p.S) * K;
        Stage cur = load_stage(wave, 0);
        for (int ci = 0; ci < nchunks; ++ci) {
            const int c = wave + ci * kWaves;
            const int tail = K - c * kChunk;
            const int nb = tail < kChunk ? tail >> 6 : 4;
            u32x4 af[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                af[s] = u32x4{0u, 0u, 0u, 0u};
                if ((s >> 1) < nb) // (wave-uniform: nothing behind the end of the row is read)
                    af[s] = *reinterpret_cast<const u32x4*>(arow + c * kChunk + 128 * (s >> 2) + 64 * ((s >> 1) & 1) + 8 * (s & 1) + 32 * (lg & 1) + 16 * (lg >> 1));
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
                compute(cur, acc[t], af, nb);
                cur = nxt;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t)
        if (t < tiles)
            *reinterpret_cast<f32x4*>(part + ((wave * p.TT + t) * 256 + lane * 4)) = acc[t];
    __syncthreads();

    // one thread per (pair, output column): the wavefronts' sums in ascending wavefront order, then the epilogue of gemm4_experts.hip.
    // Accumulator layout: lane (ln, lg) holds pass rows 4 lg ... 4 lg + 3 of weight column ln
    const int nw = C < kWaves ? C : kWaves;
    auto total = [&](int m, int rl) -> float {
        const int src = ((rl >> 4) * 256) + ((rl & 15) + 16 * (m >> 2)) * 4 + (m & 3);
        float v = part[src];
        for (int w = 1; w < nw; ++w)
            v += part[w * p.TT * 256 + src];
        return v;
    };
    if constexpr (EPI == kEpiGated) {
        const int cols = rows >> 1;
        for (int idx = tid; idx < cnt * cols; idx += kThreads) {
            const int m = idx / cols, c = idx - m * cols;
            const float ag = total(m, 2 * c), au = total(m, 2 * c + 1);
            const long rg = gate_base + c * p.col_step, ru = rg + p.up_delta;
            const float bg = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[rg]) : 0.0f;
            const float bu = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[ru]) : 0.0f;
            // torch's `F.silu(g) * u` on T-valued g, u (gemm4_experts.hip, gated epilogue)
            const float gf = static_cast<float>(static_cast<T>(rounded_f32(ag + bg)));
            const float uf = static_cast<float>(static_cast<T>(rounded_f32(au + bu)));
            const T st = static_cast<T>(rounded_f32(gf / (1.0f + expf(-gf))));
            static_cast<T*>(p.out)[static_cast<long>(pairs[m]) * (p.N >> 1) + (n0 >> 1) + c] = static_cast<T>(rounded_f32(__fmul_rn(static_cast<float>(st), uf)));
        }
    } else {
        for (int idx = tid; idx < cnt * rows; idx += kThreads) {
            const int m = idx / rows, rl = idx - m * rows;
            const float acc1 = total(m, rl);
            const int pair = pairs[m];
            const float b = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[row_base + rl]) : 0.0f;
            T* const o = static_cast<T*>(p.out) + static_cast<long>(pair) * p.N + n0 + rl;
            if constexpr (EPI == kEpiScale) {
                const float w = p.scale_f32 ? static_cast<const float*>(p.row_scale)[pair] : static_cast<float>(static_cast<const T*>(p.row_scale)[pair]);
                *o = static_cast<T>(rounded_f32(__fmul_rn(__fadd_rn(acc1, b), w)));
            } else
                *o = static_cast<T>(acc1 + b);
        }
    }
    __syncthreads();
}

template <typename T, bool NESTED, int EPI> __global__ __launch_bounds__(kThreads) void gemm4_experts_mfma_kernel(const MfmaExpertArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int e = blockIdx.y;
    const int TN = 16 * p.TT;
    const int n0 = blockIdx.x * TN;
    const int rows = (p.N - n0) < TN ? (p.N - n0) : TN;

    if (e == 0) {
        // rows of ids that name no expert: zeros, no weight read, no bias, no scale (gated: the tile's rows / 2 output columns)
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        constexpr int kSh = EPI == kEpiGated ? 1 : 0;
        for (int q = wave; q < p.P; q += kWaves) {
            const long long id = expert_id(p.ids, p.idx64, q);
            if (id < 0 || id >= p.E) {
                T* const orow = static_cast<T*>(p.out) + static_cast<long>(q) * (p.N >> kSh) + (n0 >> kSh);
                for (int c = lane; c < (rows >> kSh); c += 64)
                    orow[c] = static_cast<T>(0.0f);
            }
        }
    }

    int pos = 0, mine = 0;
    bool table_built = false;
    for (;;) {
        const int cnt = next_pairs16(p.ids, p.idx64, p.P, e, lane, pos, mine);
        if (cnt == 0)
            break;
        if (!table_built) {
            // decode table: entry e8 (a packed byte) = 64 copies of (T(code[e8 >> 4]), T(code[e8 & 15])), 256 B per entry; the two
            // halves of the workgroup write 8 of its 16 16-byte chunks each, in an order rotated by e8 (gemm4_mfma_sm.hip)
            const int cvb = __builtin_bit_cast(int, code_literal(lane & 15, p.fp4 != 0));
            const int e8 = tid & 255;
            const float hi = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((e8 >> 4) & 15) * 4, cvb));
            const float lo = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((e8 & 15) * 4, cvb));
            const uint32_t pr = Mma16x16x32<T>::pack(hi, lo);
            const u32x4 v = {pr, pr, pr, pr};
            u32x4* const dst = reinterpret_cast<u32x4*>(smem + e8 * 256);
            const int half = tid >> 8;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                dst[(8 * half + j + e8) & 15] = v;
            if constexpr (NESTED) {
                if (tid < 256)
                    reinterpret_cast<float*>(smem + kLut)[tid] = p.absmax_code[tid];
            }
            __syncthreads();
            table_built = true;
        }
        run_pass<T, NESTED, EPI>(p, smem, mine, cnt, e, n0, rows, tid);
    }
}

LdsLimit g_lds[2][2][3];

template <typename T, bool NESTED, int EPI> void launch_epi(const MfmaExpertArgs& a, dim3 grid, size_t lds, int di, hipStream_t stream) {
    ensure_dynamic_lds(g_lds[di][NESTED ? 1 : 0][EPI], reinterpret_cast<const void*>(&gemm4_experts_mfma_kernel<T, NESTED, EPI>), lds);
    hipLaunchKernelGGL((gemm4_experts_mfma_kernel<T, NESTED, EPI>), grid, dim3(kThreads), lds, stream, a);
}

template <typename T, bool NESTED> void launch(const MfmaExpertArgs& a, dim3 grid, size_t lds, int di, int epi, hipStream_t stream) {
    if (epi == kEpiGated)
        launch_epi<T, NESTED, kEpiGated>(a, grid, lds, di, stream);
    else if (epi == kEpiScale)
        launch_epi<T, NESTED, kEpiScale>(a, grid, lds, di, stream);
    else
        launch_epi<T, NESTED, kEpiPlain>(a, grid, lds, di, stream);
}

} // namespace

// Pure host logic: 16-bit activations, rows of whole 64-k sub-blocks, blocksize >= 64 (a sub-block never holds two scales), N even
// when gated, and the size limits of the expert-indexed kernel.
bool gemm_4bit_experts_mfma_supported(int dtype, long E, long N, long K, int blocksize, int gated) {
    if ((dtype != 1 && dtype != 2) || blocksize < 64 || K % 64 != 0)
        return false;
    return gemm_4bit_experts_ffn_supported(dtype, E, N, K, blocksize, gated);
}

// 16-row tiles per workgroup: one workgroup per CU when eight experts are selected (a batched call selects that many, or the whole
// of a smaller stack), at least two (the table build stays small beside the tile's weights), at most kMaxTiles and what N holds.
// The tile selects rows only: no sum depends on it.
int gemm_4bit_experts_mfma_tiles(int N) {
    const long cus = device_cu_count_or_default();
    long tt = (8L * N + 16 * cus - 1) / (16 * cus);
    tt = tt < 2 ? 2 : tt;
    tt = tt > kMaxTiles ? kMaxTiles : tt;
    const long have = (static_cast<long>(N) + 15) / 16;
    return static_cast<int>(tt < have ? tt : have);
}

// gated: 0 none, 1 chunked, 2 interleaved (N = 2 I weight rows per expert, out [P, I]); row_scale: [P] fp32 (row_scale_dtype 0) or of
// the activations' dtype, or null. Returns false, with nothing launched, outside the preconditions.
bool gemm_4bit_experts_mfma(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax8,
                            const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes,
                            const void* row_scale, int row_scale_dtype, int gated, void* out, long P, int S, int E, int N, int K,
                            int blocksize, int quant_type, hipStream_t stream) {
    if (P == 0)
        return true;
    if (P < 0 || !gemm_4bit_experts_mfma_supported(dtype, E, N, K, blocksize, gated) || (gated != 0 && row_scale != nullptr) ||
        (row_scale != nullptr && row_scale_dtype != 0 && row_scale_dtype != dtype) || (quant_type != kFP4 && quant_type != kNF4) || S <= 0 ||
        (a_slot_stride != 0 && a_slot_stride != K) || (index_bytes != 4 && index_bytes != 8) || P > (1L << 30) || A == nullptr ||
        B == nullptr || absmax == nullptr || ids == nullptr || out == nullptr ||
        (absmax8 != nullptr && (absmax_code == nullptr || absmax_offset == nullptr)) || !aligned_to(A, 16) || !aligned_to(B, 16))
        return false;
    MfmaExpertArgs a{};
    a.A = A;
    a.B = B;
    a.absmax = absmax;
    a.absmax8 = absmax8;
    a.absmax_code = absmax_code;
    a.absmax_offset = absmax_offset;
    a.bias = bias;
    a.ids = ids;
    a.out = out;
    a.row_scale = row_scale;
    a.scale_f32 = row_scale_dtype == 0;
    a.up_delta = gated == 2 ? 1 : N / 2;
    a.col_step = gated == 2 ? 2 : 1;
    a.n0_shift = gated == 2 ? 0 : 1;
    a.P = static_cast<int>(P);
    a.S = S;
    a.E = E;
    a.N = N;
    a.K = K;
    a.bs_shift = ilog2(blocksize);
    a.a_per_slot = a_slot_stride != 0;
    a.idx64 = index_bytes == 8;
    a.fp4 = quant_type == kFP4;
    a.TT = gemm_4bit_experts_mfma_tiles(N);
    const size_t lds = kLut + kCode2 + kWaves * kWaveLds + kPairsLds + static_cast<size_t>(kWaves) * a.TT * 1024;
    const dim3 grid((N + 16 * a.TT - 1) / (16 * a.TT), E);
    const bool nested = absmax8 != nullptr;
    const int epi = gated != 0 ? kEpiGated : (row_scale != nullptr ? kEpiScale : kEpiPlain);
    if (dtype == 1)
        nested ? launch<f16, true>(a, grid, lds, 0, epi, stream) : launch<f16, false>(a, grid, lds, 0, epi, stream);
    else
        nested ? launch<bf16, true>(a, grid, lds, 1, epi, stream) : launch<bf16, false>(a, grid, lds, 1, epi, stream);
    if (hipPeekAtLastError() != hipSuccess)
        return false;
    g_last_gemm_kernel = kKernelExpertsMfma;
    return true;
}

} // namespace bnb
