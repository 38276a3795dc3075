// gemm4_experts_combine.hip — token-major MoE down projection with the routing-weighted slot sum in the launch (gfx950).
//
//     y[t, n] = T( sum over the valid slots s of token t, ascending:  w[t, s] * ( h[t, s, :] . dequant(W[ids[t, s]])[n, :] + bias[ids[t, s], n] ) )
//
// W is ONE quantize_4bit result over a contiguous [E, N, K] tensor, h is [T, S, K] (one activation row per (token, slot) pair), ids and
// w are [T, S] on the DEVICE and read by the kernel only: no host synchronisation, no workspace, no memset, no atomics - the call can
// be captured in a hipGraph and replayed with other ids and weights in the same buffers.
//
// The grid is (N tile, token), not (N tile, expert) as in gemm4_experts.hip: every workgroup has work, nobody scans an id list, and
// all S slots of an output element meet in one workgroup, so the slot sum is the epilogue (fp32, ascending slot order, ONE rounding).
//
// Lane map, chosen from K alone (combine_plan; gemm4_token_major.h holds what the gate / up kernel shares): a lane owns 16 packed bytes (a CHUNK: 32 k, inside one quantization block since
// blocksize >= 32) per round; L = 8 / 16 / 32 / 64 neighbouring lanes cover L consecutive chunks of ONE weight row, Q = 2 / 3 rounds
// L chunks apart, and the 64 / L lane groups of a wavefront take 64 / L neighbouring rows of the tile. K = 768 (24 chunks) runs as
// L = 8, Q = 3: every lane of every load is live and one wavefront-wide load fetches 128 contiguous bytes of each of 8 rows, where a
// 2048-k lane map leaves 40 of 64 lanes idle. K > 6144 runs L = 64, Q = 2 over SEGS = ceil(K / 4096) segments.
//
// Work of a workgroup: UNITS (valid slot, segment), each with the tile's row groups. With at least as many units as wavefronts a
// wavefront takes units wave, wave + 8, ... whole (S = 8, short rows: one wavefront per slot); with fewer, 8 / units wavefronts share
// the row groups of a unit (S = 2, K = 14336: 8 units). The activations of a unit are register-resident fp32 for all its row groups.
//
// Sum of one output element - a function of (K, blocksize) alone, whatever T, S, the ids, the tile and the other slots' validity:
//   chunk:   32 products in four fp32 FMA chains (even / odd k of two alternating bytes), ((c00 + c01) + (c10 + c11)) * block scale
//   lane:    its Q chunk values added in ascending round order
//   row:     xor butterfly over the L lanes of the group (1, 2, 4, 8, 16, 32), the value of (slot, segment, row) goes to the LDS
//   slot:    the segments in ascending order, v_s = __fmul_rn(__fadd_rn(acc_s, bias), w_s) - the row-scale epilogue's arithmetic
//   output:  ((v_s0 + v_s1) + ...) over the valid slots in ascending slot order, one rounding to T
// A slot whose id is outside [0, E) is skipped before anything of it is read - its weight is never multiplied in; a token without a
// valid slot gets zeros, written here. Lanes behind the end of a row and row groups behind the end of the tile read in-bounds
// addresses (chunk 0, the tile's last row) and contribute 0 / are not stored.
#include "gemm4_token_major.h"

namespace bnb {

namespace {

using namespace token_major; // the lane map, the decode table, a row's chunks and its sum

constexpr int kMaxTileRows = 64;

struct CombineArgs {
    const void* h;
    const uint8_t* B;
    const float* absmax;
    const uint8_t* absmax8;
    const float* absmax_code;
    const float* absmax_offset;
    const void* bias;
    const void* ids;
    const void* w;
    void* out;
    int w_f32, idx64, fp4;
    int t0; // first token of this launch (grid.y holds at most 65535)
    int S, E, N, K, bs_shift;
    int TN;      // rows per workgroup, a multiple of 64 / L
    int L_shift; // log2 L
    int SEGS;
};

// id of pair i; the address is workgroup-uniform wherever this is called
__device__ __forceinline__ long long pair_id(const CombineArgs& p, long i) {
    return token_id(p.ids, p.idx64, i);
}

template <typename T, bool NESTED, int Q> __global__ __launch_bounds__(kThreads) void gemm4_experts_combine_kernel(const CombineArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kDepth = Q == 2 ? 2 : 1; // row groups in flight per wavefront (and as many again prefetched)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long t = static_cast<long>(p.t0) + blockIdx.y;
    const int n0 = blockIdx.x * p.TN;
    const int rows = (p.N - n0) < p.TN ? (p.N - n0) : p.TN;
    T* const orow = static_cast<T*>(p.out) + t * p.N + n0;

    // the token's valid slots: S uniform loads, a bit per slot
    uint32_t valid = 0;
    for (int s = 0; s < p.S; ++s) {
        const long long id = pair_id(p, t * p.S + s);
        valid |= (id >= 0 && id < p.E) ? (1u << s) : 0u;
    }
    valid = __builtin_amdgcn_readfirstlane(valid);
    const int nv = __builtin_popcount(valid);
    if (nv == 0) { // (workgroup-uniform: nobody waits at a barrier below)
        for (int rl = tid; rl < rows; rl += kThreads)
            orow[rl] = static_cast<T>(0.0f);
        return;
    }

    build_decode_table<NESTED>(smem, tid, p.fp4 != 0, p.absmax_code);
    __syncthreads();
    const float* const code2 = reinterpret_cast<const float*>(smem + kLutBytes);
    float* const part = reinterpret_cast<float*>(smem + kLutBytes + kCode2Bytes); // [valid slot][segment][TN]

    const int L = 1 << p.L_shift;
    const int R = 64 >> p.L_shift;          // rows per wavefront-wide load
    const int j = lane & (L - 1);           // the lane's chunk column in its group
    const int r = lane >> p.L_shift;        // the lane group's row in the row group
    const int C = p.K / kChunkK;
    const int RG = (rows + R - 1) / R;      // row groups of the tile
    const int U = nv * p.SEGS;              // units
    const int G = U >= kWaves ? 1 : kWaves / U; // wavefronts sharing a unit's row groups
    const int g = G == 1 ? 0 : wave % G;
    const uint32_t lane_off = static_cast<uint32_t>(lane & 31) * 8u;
    const float offset = NESTED ? p.absmax_offset[0] : 0.0f;

    for (int u = G == 1 ? wave : wave / G; u < U; u += kWaves) { // (G > 1: u + 8 >= U, one unit per wavefront)
        const int sv = u / p.SEGS, seg = u - sv * p.SEGS;
        const int s = nth_bit(valid, sv);
        const long pair = t * p.S + s;
        const int e = static_cast<int>(pair_id(p, pair));
        const long row_base = static_cast<long>(e) * p.N + n0;

        // the unit's activations, fp32 in registers: xr[q][b] = (h[2 b], h[2 b + 1]) of the lane's chunk of round q
        f32x2 xr[Q][16];
        int kc[Q];     // the chunk's first k (0 behind the end of the row)
        bool k_ok[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c = (seg * Q + q) * L + j;
            k_ok[q] = c < C;
            kc[q] = k_ok[q] ? c * kChunkK : 0;
            load_act32<T>(static_cast<const T*>(p.h) + pair * p.K + kc[q], xr[q]);
            if (!k_ok[q]) {
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    xr[q][b] = f32x2{0.0f, 0.0f};
            }
        }

        auto load_stage = [&](int rg) -> Stage<Q> {
            int rl = rg * R + r;
            rl = rl < rows ? rl : rows - 1; // (behind the tile: the tile's last row again, never stored)
            return load_row_chunks<NESTED, Q>(p.B, p.absmax, p.absmax8, (row_base + rl) * p.K, kc, p.bs_shift);
        };

        auto compute = [&](const Stage<Q>& st, int rg) {
            const float v = row_sum<NESTED, Q>(st, xr, k_ok, smem, code2, lane_off, offset, L);
            const int rl = rg * R + r;
            if (j == 0 && rl < rows)
                part[(sv * p.SEGS + seg) * p.TN + rl] = v;
        };

        Stage<Q> cur[kDepth], nxt[kDepth];
#pragma unroll
        for (int d = 0; d < kDepth; ++d)
            cur[d] = load_stage(g + d * G);
        for (int rg = g; rg < RG; rg += kDepth * G) {
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                nxt[d] = load_stage(rg + (kDepth + d) * G);
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                if (rg + d * G < RG) // (uniform)
                    compute(cur[d], rg + d * G);
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                cur[d] = nxt[d];
        }
    }
    __syncthreads();

    // epilogue: per slot the segments ascending, bias, routing weight; the slots ascending; one rounding
    for (int rl = tid; rl < rows; rl += kThreads) {
        float y = 0.0f;
        for (int sv = 0; sv < nv; ++sv) {
            const int s = nth_bit(valid, sv);
            const long pair = t * p.S + s;
            const long e = static_cast<long>(pair_id(p, pair));
            const float w = p.w_f32 ? static_cast<const float*>(p.w)[pair] : static_cast<float>(static_cast<const T*>(p.w)[pair]);
            float acc = 0.0f;
            for (int seg = 0; seg < p.SEGS; ++seg)
                acc += part[(sv * p.SEGS + seg) * p.TN + rl];
            const float b = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[e * p.N + n0 + rl]) : 0.0f;
            const float v = rounded_f32(__fmul_rn(__fadd_rn(acc, b), w));
            y = sv == 0 ? v : y + v;
        }
        orow[rl] = static_cast<T>(rounded_f32(y));
    }
}

LdsLimit g_lds[3][2][2];

template <typename T, bool NESTED, int Q> void launch_q(const CombineArgs& a, dim3 grid, size_t lds, int di, hipStream_t stream) {
    ensure_dynamic_lds(g_lds[di][NESTED ? 1 : 0][Q - 2], reinterpret_cast<const void*>(&gemm4_experts_combine_kernel<T, NESTED, Q>), lds);
    hipLaunchKernelGGL((gemm4_experts_combine_kernel<T, NESTED, Q>), grid, dim3(kThreads), lds, stream, a);
    BNB_CHECK_LAUNCH();
}

template <typename T> void launch(const CombineArgs& a, dim3 grid, size_t lds, int di, bool nested, int Q, hipStream_t stream) {
    if (nested)
        Q == 2 ? launch_q<T, true, 2>(a, grid, lds, di, stream) : launch_q<T, true, 3>(a, grid, lds, di, stream);
    else
        Q == 2 ? launch_q<T, false, 2>(a, grid, lds, di, stream) : launch_q<T, false, 3>(a, grid, lds, di, stream);
}

} // namespace

// Pure host logic: the geometries the kernel serves (pointer alignment - 16 bytes for h and B - is the caller's).
bool gemm_4bit_experts_combine_supported(int dtype, long E, long N, long K, int blocksize, int S) {
    if (dtype < 0 || dtype > 2 || E <= 0 || N <= 0 || K <= 0 || S < 1 || S > kMaxSlots)
        return false;
    if (!is_pow2(blocksize) || blocksize < kChunkK || K % blocksize != 0)
        return false;
    // (the (slot, segment, row) sums need no clause of their own: one row group takes at most 16 slots x 16 segments x 1 row, or
    // 16 x 1 x 8, floats - 1 KiB of kPartBudget; combine_tile_rows bounds the tile by the rest)
    return N <= (1L << 30) && K <= static_cast<long>(kMaxSegs) * kSegChunks * kChunkK && E * N < (1L << 31);
}

// Rows per workgroup: about two workgroups per CU over the whole call (T = 1 fills every CU down to N = CUs * 64 / L rows), whole row
// groups, at most kMaxTileRows and what kPartBudget holds of (slot, segment, row) sums. The tile selects rows only: no sum depends
// on it. (The budget is below kMaxTileRows rows only for S * SEGS > 48, where rows run in segments and a row group is one row;
// kMaxTileRows is a multiple of every other row group: rounding up to whole row groups never passes the cap.)
static int combine_tile_rows(const CombinePlan& plan, long T, int S, int N) {
    const int R = 64 / plan.L;
    const long cus = device_cu_count_or_default();
    long tn = (static_cast<long>(N) * T + 2 * cus - 1) / (2 * cus);
    long cap = static_cast<long>(kPartBudget / (static_cast<size_t>(S) * plan.SEGS * sizeof(float)));
    cap = cap < kMaxTileRows ? cap : kMaxTileRows;
    tn = tn < cap ? tn : cap;
    return static_cast<int>((tn + R - 1) / R * R);
}

// Debug / test query, pure host logic plus the CU count (or its override): out4 = {L, Q, SEGS, TN} of a supported call.
bool gemm_4bit_experts_combine_plan(long T, int S, int N, int K, int* out4) {
    if (T < 1 || S < 1 || S > kMaxSlots || N < 1 || K < kChunkK || K % kChunkK != 0 || K > kMaxSegs * kSegChunks * kChunkK || out4 == nullptr)
        return false;
    const CombinePlan plan = combine_plan(K);
    out4[0] = plan.L, out4[1] = plan.Q, out4[2] = plan.SEGS, out4[3] = combine_tile_rows(plan, T, S, N);
    return true;
}

// w: [T, S] fp32 (w_dtype 0) or of the activations' dtype (w_dtype == dtype). out: [T, N]. false: outside the preconditions, nothing launched.
bool gemm_4bit_experts_combine(int dtype, const void* h, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                               const float* absmax_offset, const void* bias, const void* ids, int index_bytes, const void* w, int w_dtype,
                               void* out, long T, int S, int E, int N, int K, int blocksize, int quant_type, hipStream_t stream) {
    if (T == 0)
        return true;
    if (T < 0 || !gemm_4bit_experts_combine_supported(dtype, E, N, K, blocksize, S) || w == nullptr || ids == nullptr ||
        (w_dtype != 0 && w_dtype != dtype) || (quant_type != kFP4 && quant_type != kNF4) || (index_bytes != 4 && index_bytes != 8) ||
        T > (1L << 30) / S || !aligned_to(h, 16) || !aligned_to(B, 16) ||
        h == nullptr || B == nullptr || absmax == nullptr || out == nullptr ||
        (absmax8 != nullptr && (absmax_code == nullptr || absmax_offset == nullptr)))
        return false;
    const CombinePlan plan = combine_plan(K);
    CombineArgs a{};
    a.h = h;
    a.B = B;
    a.absmax = absmax;
    a.absmax8 = absmax8;
    a.absmax_code = absmax_code;
    a.absmax_offset = absmax_offset;
    a.bias = bias;
    a.ids = ids;
    a.w = w;
    a.out = out;
    a.w_f32 = w_dtype == 0;
    a.idx64 = index_bytes == 8;
    a.fp4 = quant_type == kFP4;
    a.S = S;
    a.E = E;
    a.N = N;
    a.K = K;
    a.bs_shift = ilog2(blocksize);
    a.L_shift = ilog2(plan.L);
    a.SEGS = plan.SEGS;
    a.TN = combine_tile_rows(plan, T, S, N);
    const size_t lds = kLutBytes + kCode2Bytes + static_cast<size_t>(S) * plan.SEGS * a.TN * sizeof(float);
    const bool nested = absmax8 != nullptr;
    for (long t0 = 0; t0 < T; t0 += 65535) {
        a.t0 = static_cast<int>(t0);
        const dim3 grid((N + a.TN - 1) / a.TN, static_cast<unsigned>(T - t0 < 65535 ? T - t0 : 65535));
        if (dtype == 0)
            launch<float>(a, grid, lds, 0, nested, plan.Q, stream);
        else if (dtype == 1)
            launch<f16>(a, grid, lds, 1, nested, plan.Q, stream);
        else
            launch<bf16>(a, grid, lds, 2, nested, plan.Q, stream);
    }
    g_last_gemm_kernel = kKernelExpertsCombine;
    return true;
}

} // namespace bnb
