// gemm4_experts.hip — expert-indexed fused 4-bit matmul for mixture-of-experts decode (gfx950).
//
//     y[p, :] = x_row(p) @ dequant(W[ids[p]]).T (+ bias[ids[p], :])          p < P = T * S (token, slot) pairs
//
// W is ONE quantize_4bit result over a contiguous [E, N, K] tensor; ids live on the DEVICE and are read by the kernel only, so
// the call needs no host synchronisation and can be captured in a hipGraph and replayed with new ids in the same buffer.
//
// One launch for any id pattern: the grid is (N tile, expert). Every wavefront of a workgroup scans the id list itself (P ids:
// a few hundred bytes, one 64-lane load + ballot per 64 ids, the result wave-uniform - no LDS, no barrier), so the workgroups
// of an expert nobody selected leave after that scan without requesting one weight or absmax byte. A workgroup of a selected
// expert takes the expert's pairs in ascending pair order, kPassRows at a time, as the rows of one small-M product: the tile's
// weights are streamed once per pass (once per launch for up to kPassRows pairs per expert).
//
// The decode is the one of gemv4_stream.hip in its simplest arrangement: a lane owns 16 packed bytes (32 k) of a 2048-k row
// segment, the byte -> (code[hi], code[lo]) fp32 pair table sits in the LDS (32 bank-private copies, built from literals),
// the activations of the wavefront's segment are register-resident fp32, the products are fp32 FMAs, the block scale is
// applied to the lane's sum of 32 products, and a row's segment sums are combined in ascending segment order from the LDS.
// Every step of one output element's sum is therefore independent of which other pairs are in the call and of the slot a pair
// lands in: deterministic, order-free, no atomics.
//
// Ids outside [0, E) (a router's "dropped" slot) select nothing; the expert-0 workgroups write zeros to those rows.
//
// Two more epilogues, compile-time variants (EPI) of the same kernel - the plain form's code is what it was:
//   * gated: an expert's matrix is [2 I, K], (gate, up) rows chunked (gate [0, I), up [I, 2 I)) or interleaved (gate 2 i, up 2 i + 1);
//     the output is [P, I], out = T(float(T(silu(g))) * float(u)) with g = T(acc_g + bias_g), u = T(acc_u + bias_u) - the bits of
//     torch's `F.silu(g) * u` on the plain call's T-valued output. A workgroup keeps its TN (even) WEIGHT rows: local row 2 c is
//     the gate row and 2 c + 1 the up row of the tile's output column c, so only the local -> global row map (wave-uniform
//     scalars) and the epilogue differ; every row's sum is formed exactly as in the plain form.
//   * row scale: out[p, n] = T((acc + bias) * w[p]), w fp32 or T as it is in memory (the routing weight of the down projection).
#include "bnb_launchers.h"

namespace bnb {

namespace {

constexpr int kSegK = 2048;      // k covered by one wavefront-wide 16-byte load
constexpr int kLutBytes = 65536; // 256 entries x 32 copies x 8 B
constexpr int kCode2Bytes = 1024;
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kPassRows = 4; // pairs of one expert served by one pass over its weights
constexpr int kMaxSegs = 64; // K <= 131072
constexpr size_t kPartBudget = 12 * 1024;
constexpr int kEpiPlain = 0, kEpiGated = 1, kEpiScale = 2;

struct ExpertArgs {
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
    int up_delta, col_step, n0_shift; // kEpiGated: up row = gate row + up_delta, next column's gate row + col_step (chunked: N / 2, 1;
                            // interleaved: 1, 2); the tile's first gate row is n0 >> n0_shift (chunked: n0 / 2, interleaved: n0)
    int P, S, E, N, K, bs_shift;
    int a_per_slot; // 1: one activation row per pair, 0: one per token (pair / S)
    int idx64;
    int fp4;
    int TN;   // rows per workgroup
    int SEGS; // ceil(K / 2048)
    int SW, G; // wavefront (sw, g): segment column sw, row group g
    int PH;    // phases = ceil(SEGS / SW)
};

template <typename T> __device__ __forceinline__ void load_x32(const T* src, f32x2 (&dst)[16]);
template <> __device__ __forceinline__ void load_x32<bf16>(const bf16* src, f32x2 (&dst)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32x4 v = reinterpret_cast<const u32x4*>(src)[q];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            dst[4 * q + i] = f32x2{__builtin_bit_cast(float, v[i] << 16), __builtin_bit_cast(float, v[i] & 0xFFFF0000u)};
    }
}
template <> __device__ __forceinline__ void load_x32<f16>(const f16* src, f32x2 (&dst)[16]) {
    using h2 = __attribute__((ext_vector_type(2))) f16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32x4 v = reinterpret_cast<const u32x4*>(src)[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t e = v[i];
            const h2 h = __builtin_bit_cast(h2, e);
            dst[4 * q + i] = f32x2{static_cast<float>(h[0]), static_cast<float>(h[1])};
        }
    }
}
template <> __device__ __forceinline__ void load_x32<float>(const float* src, f32x2 (&dst)[16]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 v = reinterpret_cast<const f32x4*>(src)[q];
        dst[2 * q] = f32x2{v[0], v[1]};
        dst[2 * q + 1] = f32x2{v[2], v[3]};
    }
}

__device__ __forceinline__ long long load_id(const void* ids, int idx64, int i) {
    return idx64 ? static_cast<const long long*>(ids)[i] : static_cast<long long>(static_cast<const int*>(ids)[i]);
}

// The next up to kPassRows pairs of expert e at or behind `pos`, in ascending order; `pos` moves behind the last one taken.
// Every lane returns the same values (ballot), so the caller's control flow is uniform over the wavefront - and, because every
// wavefront of the workgroup reads the same list, over the workgroup.
__device__ __forceinline__ int next_pairs(const void* ids, int idx64, int P, int e, int lane, int& pos, int (&pr)[kPassRows]) {
    int found = 0;
#pragma unroll
    for (int j = 0; j < kPassRows; ++j)
        pr[j] = 0;
    while (pos < P && found < kPassRows) {
        const int idx = pos + lane;
        const bool hit = idx < P && load_id(ids, idx64, idx) == static_cast<long long>(e);
        unsigned long long mask = __ballot(hit);
        int last = pos;
        while (mask != 0 && found < kPassRows) {
            const int b = __builtin_ctzll(mask);
            last = pos + b;
#pragma unroll
            for (int j = 0; j < kPassRows; ++j)
                pr[j] = (found == j) ? last : pr[j];
            ++found;
            mask &= mask - 1;
        }
        pos = (mask != 0) ? last + 1 : pos + 64;
    }
#pragma unroll
    for (int j = 0; j < kPassRows; ++j)
        pr[j] = __builtin_amdgcn_readfirstlane(pr[j]);
    pos = __builtin_amdgcn_readfirstlane(pos);
    return __builtin_amdgcn_readfirstlane(found);
}

struct Stage {
    u32x4 w;  // the lane's 16 packed bytes of the row segment
    float s;  // fp32 absmax of the lane's block (plain) / the block's 8-bit code as an integer (nested)
    float s2; // nested: second-level absmax of the block's group of 256
};

// One pass: MB pairs of expert e against the workgroup's tile, all K.
template <typename T, bool NESTED, int MB, int EPI>
__device__ __forceinline__ void run_pass(const ExpertArgs& p, unsigned char* smem, const int (&pr)[kPassRows], int e, int n0, int rows, int tid) {
    // weight rows in flight per wavefront (and as many again prefetched): fewer beside the 96 ... 128 activation registers of 3 / 4 rows
    constexpr int kDepth = MB >= 3 ? 2 : 4;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sw = wave / p.G, g = wave % p.G;
    const bool wave_active = sw < p.SW;
    const float* const code2 = reinterpret_cast<const float*>(smem + kLutBytes);
    float* const part = reinterpret_cast<float*>(smem + kLutBytes + kCode2Bytes);
    const uint32_t lane_off = static_cast<uint32_t>(lane & 31) * 8u;
    const float offset = NESTED ? p.absmax_offset[0] : 0.0f;
    const long row_base = static_cast<long>(e) * p.N + n0; // first row of the tile in the flat [E * N, K] matrix
    const int items = (wave_active && g < rows) ? (rows - g + p.G - 1) / p.G : 0;
    // gated: local row rl = 2 c + h is the gate (h = 0) or up (h = 1) row of the tile's output column c (n0 and rows are even)
    // chunked: gate row (n0 >> 1) + c, up row N / 2 + that; interleaved: gate row n0 + 2 c, up row that + 1. One base beside the
    // launch's two constants (up_delta, col_step): nothing more stays live across the item loop than in the plain form
    const long gate_base = static_cast<long>(e) * p.N + (n0 >> p.n0_shift);
    auto global_row = [&](int rl) -> long {
        if constexpr (EPI == kEpiGated)
            return gate_base + (rl & 1) * p.up_delta + (rl >> 1) * p.col_step;
        else
            return row_base + rl;
    };

    for (int ph = 0; ph < p.PH; ++ph) {
        const int seg = ph * p.SW + sw;
        if (!wave_active || seg >= p.SEGS || items == 0)
            continue; // (wave-uniform; barriers are outside this loop)
        const int k0 = seg * kSegK + lane * 32;
        const bool k_ok = k0 < p.K;
        const int k0c = k_ok ? k0 : 0; // lanes behind the end of the row read the row's first bytes and contribute 0

        // activations of this segment, fp32 in registers: xr[m][b] = (x[2 b], x[2 b + 1]) of the lane's 32 k
        f32x2 xr[MB][16];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const long arow = p.a_per_slot ? pr[m] : pr[m] / p.S;
            load_x32<T>(static_cast<const T*>(p.A) + arow * p.K + k0c, xr[m]);
            if (!k_ok) {
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    xr[m][b] = f32x2{0.0f, 0.0f};
            }
        }

        auto load_stage = [&](int item) -> Stage {
            const int it = item < items ? item : items - 1; // (clamped: the prefetch behind the last row re-reads it)
            const int rl = g + it * p.G;
            const long elem = global_row(rl) * p.K + k0c;
            Stage st;
            st.w = *reinterpret_cast<const u32x4*>(p.B + (elem >> 1));
            const long blk = elem >> p.bs_shift;
            if constexpr (NESTED) {
                st.s = __builtin_bit_cast(float, static_cast<uint32_t>(p.absmax8[blk]));
                st.s2 = p.absmax[blk >> 8];
            } else {
                st.s = p.absmax[blk];
                st.s2 = 0.0f;
            }
            return st;
        };

        auto compute = [&](const Stage& st, int item) {
            f32x2 cp[16];
            float c2v = 0.0f;
            if constexpr (NESTED)
                c2v = code2[__builtin_bit_cast(uint32_t, st.s)];
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // {lane copy offset, weight byte j, 0, 0}: byte * 256 + copy * 8
                    const uint32_t off = __builtin_amdgcn_perm(st.w[d], lane_off, 0x0C0C0400u + (j << 8));
                    cp[4 * d + j] = *reinterpret_cast<const f32x2*>(smem + off);
                }
            float scale;
            if constexpr (NESTED)
                scale = nested_scale(c2v, st.s2, offset);
            else
                scale = st.s;
            scale = k_ok ? scale : 0.0f;
            // two independent chains of packed FMAs per row: [chain][even k, odd k]
            f32x2 acc[MB][2];
#pragma unroll
            for (int m = 0; m < MB; ++m)
                acc[m][0] = acc[m][1] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int b = 0; b < 16; ++b)
#pragma unroll
                for (int m = 0; m < MB; ++m)
                    acc[m][b & 1] = __builtin_elementwise_fma(cp[b], xr[m][b], acc[m][b & 1]);
            float v[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m)
                v[m] = ((acc[m][0][0] + acc[m][0][1]) + (acc[m][1][0] + acc[m][1][1])) * scale;
            wave_sum_n<MB>(v);
            const int rl = g + item * p.G;
            if (lane == 0 && item < items) {
#pragma unroll
                for (int m = 0; m < MB; ++m)
                    part[(rl * p.SEGS + seg) * kPassRows + m] = v[m];
            }
        };

        Stage cur[kDepth], nxt[kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u)
            cur[u] = load_stage(u);
        for (int it = 0; it < items; it += kDepth) {
#pragma unroll
            for (int u = 0; u < kDepth; ++u)
                nxt[u] = load_stage(it + kDepth + u);
#pragma unroll
            for (int u = 0; u < kDepth; ++u)
                compute(cur[u], it + u);
#pragma unroll
            for (int u = 0; u < kDepth; ++u)
                cur[u] = nxt[u];
        }
    }
    __syncthreads();
    // a row's segment sums in ascending segment order, bias, one rounding
    if constexpr (EPI == kEpiGated) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            T* const orow = static_cast<T*>(p.out) + static_cast<long>(pr[m]) * (p.N >> 1) + (n0 >> 1);
            for (int c = tid; c < (rows >> 1); c += kThreads) {
                float ag = 0.0f, au = 0.0f;
                for (int s = 0; s < p.SEGS; ++s)
                    ag += part[((2 * c) * p.SEGS + s) * kPassRows + m];
                for (int s = 0; s < p.SEGS; ++s)
                    au += part[((2 * c + 1) * p.SEGS + s) * kPassRows + m];
                const long rg = gate_base + c * p.col_step, ru = rg + p.up_delta;
                const float bg = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[rg]) : 0.0f;
                const float bu = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[ru]) : 0.0f;
                // torch's `F.silu(g) * u` on T-valued g, u: silu in fp32 (exact expf, IEEE division) rounded to T, the product
                // in fp32 rounded to T (csrc/gemv4_stream.hip, gated production)
                const float gf = static_cast<float>(static_cast<T>(rounded_f32(ag + bg)));
                const float uf = static_cast<float>(static_cast<T>(rounded_f32(au + bu)));
                const T st = static_cast<T>(rounded_f32(gf / (1.0f + expf(-gf))));
                orow[c] = static_cast<T>(rounded_f32(__fmul_rn(static_cast<float>(st), uf)));
            }
        }
        __syncthreads();
        return;
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        T* const orow = static_cast<T*>(p.out) + static_cast<long>(pr[m]) * p.N + n0;
        [[maybe_unused]] float w = 1.0f; // the pair's routing weight: one fp32 multiply in front of the single rounding
        if constexpr (EPI == kEpiScale)
            w = p.scale_f32 ? static_cast<const float*>(p.row_scale)[pr[m]] : static_cast<float>(static_cast<const T*>(p.row_scale)[pr[m]]);
        for (int rl = tid; rl < rows; rl += kThreads) {
            float acc = 0.0f;
            for (int s = 0; s < p.SEGS; ++s)
                acc += part[(rl * p.SEGS + s) * kPassRows + m];
            const float b = p.bias ? static_cast<float>(static_cast<const T*>(p.bias)[row_base + rl]) : 0.0f;
            if constexpr (EPI == kEpiScale)
                orow[rl] = static_cast<T>(rounded_f32(__fmul_rn(__fadd_rn(acc, b), w)));
            else
                orow[rl] = static_cast<T>(acc + b);
        }
    }
    __syncthreads();
}

template <typename T, bool NESTED, int EPI = kEpiPlain> __global__ __launch_bounds__(kThreads) void gemm4_experts_kernel(const ExpertArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int e = blockIdx.y;
    const int n0 = blockIdx.x * p.TN;
    const int rows = (p.N - n0) < p.TN ? (p.N - n0) : p.TN;

    if (e == 0) {
        // rows of ids that name no expert: zeros, no weight read, no bias, no scale (gated: the tile's rows / 2 output columns)
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        constexpr int kSh = EPI == kEpiGated ? 1 : 0;
        for (int q = wave; q < p.P; q += kWaves) {
            const long long id = load_id(p.ids, p.idx64, q);
            if (id < 0 || id >= p.E) {
                T* const orow = static_cast<T*>(p.out) + static_cast<long>(q) * (p.N >> kSh) + (n0 >> kSh);
                for (int c = lane; c < (rows >> kSh); c += 64)
                    orow[c] = static_cast<T>(0.0f);
            }
        }
    }

    int pos = 0;
    int pr[kPassRows];
    bool table_built = false;
    for (;;) {
        const int cnt = next_pairs(p.ids, p.idx64, p.P, e, lane, pos, pr);
        if (cnt == 0)
            break;
        if (!table_built) {
            // decode table: entry e8 (a packed byte) = 32 copies of (code[e8 >> 4], code[e8 & 15]) in fp32, 256 B per entry, copy c
            // at byte 8 c. 16-byte chunk c16 = it * 512 + tid holds two copies of entry it * 32 + (tid >> 4): the high code is
            // a literal of the pass, the low one a per-thread constant; every ds_write_b128 of a wavefront covers 1 KiB.
            const float lo = code_literal((tid >> 4) & 15, p.fp4 != 0);
            constexpr int kIters = kLutBytes / 16 / kThreads;
            static_assert(kThreads == 512 && kIters == 8, "chunk -> entry arithmetic below");
#pragma unroll
            for (int it = 0; it < kIters; ++it) {
                const float hi = (tid >> 8) ? code_literal(2 * it + 1, p.fp4 != 0) : code_literal(2 * it, p.fp4 != 0);
                *reinterpret_cast<f32x4*>(smem + (it * kThreads + tid) * 16) = f32x4{hi, lo, hi, lo};
            }
            if constexpr (NESTED) {
                if (tid < 256)
                    reinterpret_cast<float*>(smem + kLutBytes)[tid] = p.absmax_code[tid];
            }
            __syncthreads();
            table_built = true;
        }
        if (cnt == 1)
            run_pass<T, NESTED, 1, EPI>(p, smem, pr, e, n0, rows, tid);
        else if (cnt == 2)
            run_pass<T, NESTED, 2, EPI>(p, smem, pr, e, n0, rows, tid);
        else if (cnt == 3)
            run_pass<T, NESTED, 3, EPI>(p, smem, pr, e, n0, rows, tid);
        else
            run_pass<T, NESTED, 4, EPI>(p, smem, pr, e, n0, rows, tid);
    }
}

LdsLimit g_lds[3][2][3];

template <typename T, bool NESTED, int EPI> void launch_epi(const ExpertArgs& a, dim3 grid, size_t lds, int di, hipStream_t stream) {
    ensure_dynamic_lds(g_lds[di][NESTED ? 1 : 0][EPI], reinterpret_cast<const void*>(&gemm4_experts_kernel<T, NESTED, EPI>), lds);
    hipLaunchKernelGGL((gemm4_experts_kernel<T, NESTED, EPI>), grid, dim3(kThreads), lds, stream, a);
    BNB_CHECK_LAUNCH();
}

template <typename T, bool NESTED> void launch(const ExpertArgs& a, dim3 grid, size_t lds, int di, int epi, hipStream_t stream) {
    if (epi == kEpiGated)
        launch_epi<T, NESTED, kEpiGated>(a, grid, lds, di, stream);
    else if (epi == kEpiScale)
        launch_epi<T, NESTED, kEpiScale>(a, grid, lds, di, stream);
    else
        launch_epi<T, NESTED, kEpiPlain>(a, grid, lds, di, stream);
}

} // namespace

// Pure host logic: the geometries the kernel serves (pointer alignment - 16 bytes for A, B and out rows - is the caller's).
bool gemm_4bit_experts_supported(int dtype, long E, long N, long K, int blocksize) {
    if (dtype < 0 || dtype > 2 || E <= 0 || N <= 0 || K <= 0)
        return false;
    if (!is_pow2(blocksize) || blocksize < 32 || K % blocksize != 0)
        return false;
    if (E > 65535 || N > (1L << 30) || K > static_cast<long>(kMaxSegs) * kSegK)
        return false;
    return E * N < (1L << 31);
}

// The geometries of the FFN entry point: the plain predicate, and an even number of weight rows (gate + up) in a gated call.
bool gemm_4bit_experts_ffn_supported(int dtype, long E, long N, long K, int blocksize, int gated) {
    if (gated < 0 || gated > 2 || (gated != 0 && N % 2 != 0))
        return false;
    return gemm_4bit_experts_supported(dtype, E, N, K, blocksize);
}

// gated: 0 none, 1 chunked, 2 interleaved (N = 2 I weight rows per expert, out [P, I]); row_scale: [P] fp32 (row_scale_dtype 0) or
// of the activations' dtype (row_scale_dtype == dtype), or null. Not both.
void gemm_4bit_experts_ffn(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax8,
                           const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes,
                           const void* row_scale, int row_scale_dtype, int gated, void* out, long P, int S, int E, int N, int K,
                           int blocksize, int quant_type, hipStream_t stream) {
    if (P <= 0)
        return;
    if (!gemm_4bit_experts_ffn_supported(dtype, E, N, K, blocksize, gated) || (gated != 0 && row_scale != nullptr) ||
        (row_scale != nullptr && row_scale_dtype != 0 && row_scale_dtype != dtype) ||
        (quant_type != kFP4 && quant_type != kNF4) || S <= 0 ||
        (a_slot_stride != 0 && a_slot_stride != K) || (index_bytes != 4 && index_bytes != 8) || P > (1L << 30) ||
        !aligned_to(A, 16) || !aligned_to(B, 16)) {
        fprintf(stderr,
                "bitsandbytes_amd: gemm_4bit_experts: unsupported call (dtype %d, E %d, N %d, K %d, blocksize %d, quant_type %d, "
                "a_slot_stride %ld, index_bytes %d, gated %d, row_scale %s of dtype %d; A and B must be 16-byte aligned, gated and "
                "row_scale exclude each other)\n",
                dtype, E, N, K, blocksize, quant_type, a_slot_stride, index_bytes, gated, row_scale ? "given" : "null", row_scale_dtype);
        exit(1);
    }
    ExpertArgs a{};
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
    a.SEGS = (K + kSegK - 1) / kSegK;
    a.SW = a.SEGS < kWaves ? a.SEGS : kWaves;
    a.G = kWaves / a.SW;
    a.PH = (a.SEGS + a.SW - 1) / a.SW;
    // rows per workgroup: two workgroups per CU when two experts are selected (the decode regime), at least 32 rows so that
    // the 64 KiB table build stays small beside the weights of the tile, bounded by the LDS of the segment sums
    int tn = (N + 255) / 256;
    if (tn < 32)
        tn = 32;
    const int tn_cap = static_cast<int>(kPartBudget / (static_cast<size_t>(a.SEGS) * kPassRows * sizeof(float)));
    if (tn > tn_cap)
        tn = tn_cap;
    if (gated != 0)
        tn &= ~1; // (gate, up) row pairs: TN / 2 output columns (tn >= 12 here)
    a.TN = tn;
    const size_t lds = kLutBytes + kCode2Bytes + static_cast<size_t>(tn) * a.SEGS * kPassRows * sizeof(float);
    const dim3 grid((N + tn - 1) / tn, E);
    const bool nested = absmax8 != nullptr;
    const int epi = gated != 0 ? kEpiGated : (row_scale != nullptr ? kEpiScale : kEpiPlain);
    if (dtype == 0)
        nested ? launch<float, true>(a, grid, lds, 0, epi, stream) : launch<float, false>(a, grid, lds, 0, epi, stream);
    else if (dtype == 1)
        nested ? launch<f16, true>(a, grid, lds, 1, epi, stream) : launch<f16, false>(a, grid, lds, 1, epi, stream);
    else
        nested ? launch<bf16, true>(a, grid, lds, 2, epi, stream) : launch<bf16, false>(a, grid, lds, 2, epi, stream);
    g_last_gemm_kernel = kKernelExperts;
}

void gemm_4bit_experts(int dtype, const void* A, long a_slot_stride, const uint8_t* B, const float* absmax, const uint8_t* absmax8,
                       const float* absmax_code, const float* absmax_offset, const void* bias, const void* ids, int index_bytes,
                       void* out, long P, int S, int E, int N, int K, int blocksize, int quant_type, hipStream_t stream) {
    gemm_4bit_experts_ffn(dtype, A, a_slot_stride, B, absmax, absmax8, absmax_code, absmax_offset, bias, ids, index_bytes, nullptr, 0, 0,
                          out, P, S, E, N, K, blocksize, quant_type, stream);
}

} // namespace bnb
