// gemm4_experts_gate_up.hip — token-major MoE gate / up projection with gated SiLU in the launch (gfx950).
//
//     h[t, s, i] = T( float(T(silu(g))) * float(u) ),   g = T( x[t, :] . dequant(W[e])[gate row i, :] + bias[e, gate row i] ),
//                                                       u = T( x[t, :] . dequant(W[e])[up row i, :]   + bias[e, up row i] ),   e = ids[t, s]
//
// W is ONE quantize_4bit result over a contiguous [E, 2 I, K] tensor - chunked: gate rows [0, I), up rows [I, 2 I) of every expert;
// interleaved: gate row 2 i, up row 2 i + 1 -, x is [T, K] (ONE activation row per token, shared by its S slots), ids is [T, S] on the
// DEVICE and read by the kernel only: no host synchronisation, no workspace, no memset, no atomics - the call can be captured in a
// hipGraph and replayed with other ids in the same buffer. The output is [T, S, I]; the row of a slot whose id is outside [0, E) is
// zeros, written here, and nothing of such a slot is read.
//
// The counterpart of gemm4_experts_combine.hip, whose lane map, decode table and row sum it shares (gemm4_token_major.h). The grid is
// (column tile, token), not (row tile, expert) as in gemm4_experts.hip: every workgroup has work and nobody scans an id list. What
// differs from the down projection:
//   * x[t] is the activation row of every slot. The units of a workgroup, (segment, valid slot) in that order, are dealt to the
//     wavefronts in contiguous runs, so a wavefront reloads and reconverts its Q * 32 fp32 activations only where its segment changes:
//     with one segment (K <= 6144) once for the life of the workgroup, at 2 segments x 8 slots once as well (two slots of one segment
//     per wavefront). With fewer units than wavefronts 8 / units wavefronts share the row groups of a unit, as in the down kernel.
//   * A tile of TC output columns has 2 TC local weight rows. Chunked: local row lr < cols is the gate row n0 + lr, the others the up
//     row I + n0 + lr - cols (two contiguous runs of the expert's matrix); interleaved: row 2 n0 + lr (one run).
//   * The partial sums of a workgroup are [valid slot][segment][2 TC]; after ONE barrier a thread per (valid slot, column) adds the
//     segments of its gate and of its up row in ascending order, the biases, applies the gated arithmetic of gemm4_experts.hip -
//     silu in fp32 with expf and IEEE division, rounded to T; __fmul_rn; rounded to T - and makes one store.
//
// Sum of one g or u - a function of (K, blocksize) alone, whatever T, S, the ids, the tile and the CU count: the chunk, the lane's
// rounds, the xor butterfly (row_sum, gemm4_token_major.h), then the segments in ascending order from the LDS.
// Lanes behind the end of a row and row groups behind the end of the tile read in-bounds addresses (chunk 0, the tile's last row)
// and contribute 0 / are not stored.
#include "gemm4_token_major.h"

namespace bnb {

namespace {

using namespace token_major;

constexpr int kMaxTileCols = 32; // 64 weight rows

struct GateUpArgs {
    const void* x;
    const uint8_t* B;
    const float* absmax;
    const uint8_t* absmax8;
    const float* absmax_code;
    const float* absmax_offset;
    const void* bias;
    const void* ids;
    void* out;
    int idx64, fp4, interleaved;
    int t0; // first token of this launch (grid.y holds at most 65535)
    int S, E, I, K, bs_shift;
    int TC;      // output columns per workgroup; 2 TC is a multiple of 64 / L
    int L_shift; // log2 L
    int SEGS;
};

template <typename T, bool NESTED, int Q> __global__ __launch_bounds__(kThreads) void gemm4_experts_gate_up_kernel(const GateUpArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kDepth = Q == 2 ? 2 : 1; // row groups in flight per wavefront (and as many again prefetched)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long t = static_cast<long>(p.t0) + blockIdx.y;
    const int n0 = blockIdx.x * p.TC;
    const int cols = (p.I - n0) < p.TC ? (p.I - n0) : p.TC;
    const int rows = 2 * cols; // local weight rows
    T* const otok = static_cast<T*>(p.out) + t * p.S * p.I + n0; // slot s at + s * I

    // the token's valid slots: S uniform loads, a bit per slot
    uint32_t valid = 0;
    for (int s = 0; s < p.S; ++s) {
        const long long id = token_id(p.ids, p.idx64, t * p.S + s);
        valid |= (id >= 0 && id < p.E) ? (1u << s) : 0u;
    }
    valid = __builtin_amdgcn_readfirstlane(valid);
    const int nv = __builtin_popcount(valid);
    if (nv < p.S) { // the tile's columns of every dropped slot: zeros
        for (int i = tid; i < p.S * cols; i += kThreads) {
            const int s = i / cols, c = i - s * cols;
            if (!((valid >> s) & 1u))
                otok[static_cast<long>(s) * p.I + c] = static_cast<T>(0.0f);
        }
        if (nv == 0) // (workgroup-uniform: nobody waits at a barrier below)
            return;
    }

    build_decode_table<NESTED>(smem, tid, p.fp4 != 0, p.absmax_code);
    __syncthreads();
    const float* const code2 = reinterpret_cast<const float*>(smem + kLutBytes);
    float* const part = reinterpret_cast<float*>(smem + kLutBytes + kCode2Bytes); // [valid slot][segment][2 TC]
    const int PR = 2 * p.TC;

    const int L = 1 << p.L_shift;
    const int R = 64 >> p.L_shift;          // weight rows per wavefront-wide load
    const int j = lane & (L - 1);           // the lane's chunk column in its group
    const int r = lane >> p.L_shift;        // the lane group's row in the row group
    const int C = p.K / kChunkK;
    const int N = 2 * p.I;
    const int RG = (rows + R - 1) / R;      // row groups of the tile
    const int U = nv * p.SEGS;              // units, segment-major: u = seg * nv + sv
    // at least as many units as wavefronts: wavefront w takes the run [w U / 8, (w + 1) U / 8) whole; fewer: 8 / U wavefronts share
    // the row groups of unit w / G (wavefronts behind U * G have none)
    const int G = U >= kWaves ? 1 : kWaves / U;
    const int g = G == 1 ? 0 : wave % G;
    const int u_begin = G == 1 ? wave * U / kWaves : wave / G;
    const int u_end = G == 1 ? (wave + 1) * U / kWaves : (u_begin < U ? u_begin + 1 : u_begin);
    const uint32_t lane_off = static_cast<uint32_t>(lane & 31) * 8u;
    const float offset = NESTED ? p.absmax_offset[0] : 0.0f;

    // the activations of the wavefront's segment, fp32 in registers: xr[q][b] = (x[2 b], x[2 b + 1]) of the lane's chunk of round q
    f32x2 xr[Q][16];
    int kc[Q];     // the chunk's first k (0 behind the end of the row)
    bool k_ok[Q];
    int have_seg = -1;
    for (int u = u_begin; u < u_end; ++u) {
        const int seg = u / nv, sv = u - seg * nv;
        if (seg != have_seg) { // (uniform)
            have_seg = seg;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int c = (seg * Q + q) * L + j;
                k_ok[q] = c < C;
                kc[q] = k_ok[q] ? c * kChunkK : 0;
                load_act32<T>(static_cast<const T*>(p.x) + t * p.K + kc[q], xr[q]);
                if (!k_ok[q]) {
#pragma unroll
                    for (int b = 0; b < 16; ++b)
                        xr[q][b] = f32x2{0.0f, 0.0f};
                }
            }
        }
        const int s = nth_bit(valid, sv);
        const int e = static_cast<int>(token_id(p.ids, p.idx64, t * p.S + s));
        const long expert_row = static_cast<long>(e) * N;

        auto load_stage = [&](int rg) -> Stage<Q> {
            int rl = rg * R + r;
            rl = rl < rows ? rl : rows - 1; // (behind the tile: the tile's last row again, never stored)
            const int row = p.interleaved ? 2 * n0 + rl : (rl < cols ? n0 + rl : p.I + n0 + rl - cols);
            return load_row_chunks<NESTED, Q>(p.B, p.absmax, p.absmax8, (expert_row + row) * p.K, kc, p.bs_shift);
        };

        auto compute = [&](const Stage<Q>& st, int rg) {
            const float v = row_sum<NESTED, Q>(st, xr, k_ok, smem, code2, lane_off, offset, L);
            const int rl = rg * R + r;
            if (j == 0 && rl < rows)
                part[(sv * p.SEGS + seg) * PR + rl] = v;
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

    // epilogue: a thread per (valid slot, column) - the segments of the gate and of the up row ascending, the biases, the gated
    // arithmetic of gemm4_experts.hip (torch's `F.silu(g) * u` on T-valued g, u), one store
    for (int i = tid; i < nv * cols; i += kThreads) {
        const int sv = i / cols, c = i - sv * cols;
        const int s = nth_bit(valid, sv);
        const long e = static_cast<long>(token_id(p.ids, p.idx64, t * p.S + s));
        const float* const ps = part + sv * p.SEGS * PR;
        const int lg = p.interleaved ? 2 * c : c, lu = p.interleaved ? 2 * c + 1 : cols + c;
        float ag = 0.0f, au = 0.0f;
        for (int seg = 0; seg < p.SEGS; ++seg)
            ag += ps[seg * PR + lg];
        for (int seg = 0; seg < p.SEGS; ++seg)
            au += ps[seg * PR + lu];
        const long rg = e * N + (p.interleaved ? 2 * (n0 + c) : n0 + c), ru = rg + (p.interleaved ? 1 : p.I);
        const float bg = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[rg]) : 0.0f;
        const float bu = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[ru]) : 0.0f;
        const float gf = static_cast<float>(static_cast<T>(rounded_f32(ag + bg)));
        const float uf = static_cast<float>(static_cast<T>(rounded_f32(au + bu)));
        const T st = static_cast<T>(rounded_f32(gf / (1.0f + expf(-gf))));
        otok[static_cast<long>(s) * p.I + c] = static_cast<T>(rounded_f32(__fmul_rn(static_cast<float>(st), uf)));
    }
}

LdsLimit g_lds[3][2][2];

template <typename T, bool NESTED, int Q> void launch_q(const GateUpArgs& a, dim3 grid, size_t lds, int di, hipStream_t stream) {
    ensure_dynamic_lds(g_lds[di][NESTED ? 1 : 0][Q - 2], reinterpret_cast<const void*>(&gemm4_experts_gate_up_kernel<T, NESTED, Q>), lds);
    hipLaunchKernelGGL((gemm4_experts_gate_up_kernel<T, NESTED, Q>), grid, dim3(kThreads), lds, stream, a);
    BNB_CHECK_LAUNCH();
}

template <typename T> void launch(const GateUpArgs& a, dim3 grid, size_t lds, int di, bool nested, int Q, hipStream_t stream) {
    if (nested)
        Q == 2 ? launch_q<T, true, 2>(a, grid, lds, di, stream) : launch_q<T, true, 3>(a, grid, lds, di, stream);
    else
        Q == 2 ? launch_q<T, false, 2>(a, grid, lds, di, stream) : launch_q<T, false, 3>(a, grid, lds, di, stream);
}

// Output columns per workgroup: about two workgroups per CU over the whole call, whole row groups (2 TC a multiple of 64 / L), at most
// kMaxTileCols and what kPartBudget holds of (slot, segment, 2 TC) sums. The tile selects rows only: no sum depends on it. (The
// budget is below kMaxTileCols only for S * SEGS > 48, where rows run in segments and a row group is one row; kMaxTileCols is a
// multiple of every other half row group, so rounding up to whole row groups never passes the cap; the cap is at least 6.)
int gate_up_tile_cols(const CombinePlan& plan, long T, int S, int I) {
    const int half = plan.L >= 32 ? 1 : 32 / plan.L; // columns of one row group: R / 2, at least 1
    const long cus = device_cu_count_or_default();
    long tc = (static_cast<long>(I) * T + 2 * cus - 1) / (2 * cus);
    long cap = static_cast<long>(kPartBudget / (static_cast<size_t>(S) * plan.SEGS * 2 * sizeof(float)));
    cap = cap < kMaxTileCols ? cap : kMaxTileCols;
    tc = tc < cap ? tc : cap;
    return static_cast<int>((tc + half - 1) / half * half);
}

} // namespace

// Pure host logic: the geometries the kernel serves (pointer alignment - 16 bytes for x and B - is the caller's). N = 2 I weight rows
// per expert; gated: 1 chunked, 2 interleaved.
bool gemm_4bit_experts_gate_up_supported(int dtype, long E, long N, long K, int blocksize, int S, int gated) {
    if (dtype < 0 || dtype > 2 || E <= 0 || N <= 0 || N % 2 != 0 || K <= 0 || S < 1 || S > kMaxSlots || (gated != 1 && gated != 2))
        return false;
    if (!is_pow2(blocksize) || blocksize < kChunkK || K % blocksize != 0)
        return false;
    return N <= (1L << 30) && K <= static_cast<long>(kMaxSegs) * kSegChunks * kChunkK && E * N < (1L << 31);
}

// Debug / test query, pure host logic plus the CU count (or its override): out4 = {L, Q, SEGS, TC} of a supported call.
bool gemm_4bit_experts_gate_up_plan(long T, int S, int N, int K, int* out4) {
    if (T < 1 || S < 1 || S > kMaxSlots || N < 2 || N % 2 != 0 || K < kChunkK || K % kChunkK != 0 || K > kMaxSegs * kSegChunks * kChunkK ||
        out4 == nullptr)
        return false;
    const CombinePlan plan = combine_plan(K);
    out4[0] = plan.L, out4[1] = plan.Q, out4[2] = plan.SEGS, out4[3] = gate_up_tile_cols(plan, T, S, N / 2);
    return true;
}

// x: [T, K]; out: [T, S, N / 2]. false: outside the preconditions, nothing launched.
bool gemm_4bit_experts_gate_up(int dtype, const void* x, const uint8_t* B, const float* absmax, const uint8_t* absmax8, const float* absmax_code,
                               const float* absmax_offset, const void* bias, const void* ids, int index_bytes, int gated, void* out, long T, int S,
                               int E, int N, int K, int blocksize, int quant_type, hipStream_t stream) {
    if (T == 0)
        return true;
    if (T < 0 || !gemm_4bit_experts_gate_up_supported(dtype, E, N, K, blocksize, S, gated) || ids == nullptr ||
        (quant_type != kFP4 && quant_type != kNF4) || (index_bytes != 4 && index_bytes != 8) || T > (1L << 30) / S || !aligned_to(x, 16) ||
        !aligned_to(B, 16) || x == nullptr || B == nullptr || absmax == nullptr || out == nullptr ||
        (absmax8 != nullptr && (absmax_code == nullptr || absmax_offset == nullptr)))
        return false;
    const CombinePlan plan = combine_plan(K);
    GateUpArgs a{};
    a.x = x;
    a.B = B;
    a.absmax = absmax;
    a.absmax8 = absmax8;
    a.absmax_code = absmax_code;
    a.absmax_offset = absmax_offset;
    a.bias = bias;
    a.ids = ids;
    a.out = out;
    a.idx64 = index_bytes == 8;
    a.fp4 = quant_type == kFP4;
    a.interleaved = gated == 2;
    a.S = S;
    a.E = E;
    a.I = N / 2;
    a.K = K;
    a.bs_shift = ilog2(blocksize);
    a.L_shift = ilog2(plan.L);
    a.SEGS = plan.SEGS;
    a.TC = gate_up_tile_cols(plan, T, S, a.I);
    const size_t lds = kLutBytes + kCode2Bytes + static_cast<size_t>(S) * plan.SEGS * 2 * a.TC * sizeof(float);
    const bool nested = absmax8 != nullptr;
    for (long t0 = 0; t0 < T; t0 += 65535) {
        a.t0 = static_cast<int>(t0);
        const dim3 grid((a.I + a.TC - 1) / a.TC, static_cast<unsigned>(T - t0 < 65535 ? T - t0 : 65535));
        if (dtype == 0)
            launch<float>(a, grid, lds, 0, nested, plan.Q, stream);
        else if (dtype == 1)
            launch<f16>(a, grid, lds, 1, nested, plan.Q, stream);
        else
            launch<bf16>(a, grid, lds, 2, nested, plan.Q, stream);
    }
    g_last_gemm_kernel = kKernelExpertsGateUp;
    return true;
}

} // namespace bnb
