// lora_shrink.hip — the LoRA "shrink" matmul of a decode step, t = x · lora_A^T, as a kernel of this library (gfx950, wave64).
//
//     t[m, j] = T( sum_{k < K} float(x[m, k]) * float(A[j, k]) )          fp32 sum, ONE rounding to T
//
// x [M, K] and A [R, K] row-major, T = fp16 / bf16, 1 <= M <= 16, K % 64 == 0, R % 8 == 0, 8 <= R <= 1024. A is PEFT's lora_A.weight
// as stored, or up to eight of them concatenated along dim 0 (`splits`): part i of the output is then a CONTIGUOUS [M, r_i] matrix
// at element offset M * (r_0 + ... + r_{i-1}) of the one output buffer, which is what bnb_mi355x_gemm_4bit_lora takes as lora_t.
//
// Decomposition. One workgroup of 16 wavefronts owns EIGHT adapter rows and the whole of K: grid = R / 8, no workspace, no traffic
// between workgroups, nothing to wait for. R % 8 == 0 and r_i % 8 == 0, so a tile is always full and never straddles two parts.
// The dot products run on the matrix pipe: v_mfma_f32_16x16x32 with the rows of x as the A operand (row m = lane % 16, rows >= M are
// zeros) and the eight adapter rows as the B operand (column j = lane % 16, columns >= 8 are zeros); both operands of lane group
// g = lane / 16 hold k = 32 s + 8 g ... + 7 of step s - one 16-byte load each, straight from global memory into the operand registers.
// Eight rows, not sixteen, because the work is latency- and per-CU-bandwidth-bound and nowhere near the matrix pipe: the half-empty
// B operand costs nothing, twice the workgroups halve every workgroup's stream (arithmetic in DESIGN.md §3.14).
//
// Summation order - a function of K alone. K is cut into steps of 32 k; wavefront w of the 16 takes steps w, w + 16, w + 32, ... in
// ascending order into ONE fp32 accumulator tile that starts at zero (a step is one MFMA: the hardware's fixed 32-term order); the
// sixteen tiles meet in LDS and one thread per output adds them in ascending w, ((p0 + p1) + p2) + ... + p15 (wavefronts without a
// step contribute their zero), and rounds once. Every column of an MFMA is computed independently of the others, so t[m, j] does not
// depend on R, on where row j sits in A, on the splits, or on the grid; it does not depend on M either (one family for M = 1 ... 16).
//
// Mixed-adapter form (lora_shrink_ids_kernel): A is a stack [A_n, R, K], every row of x names its adapter by an id
// on the device, the grid gets a second dimension (adapter), and the tile body below runs with the rows of other adapters masked
// out of the x operand - same steps, same order, so a row has the bits of the uniform kernel's call with its adapter.
#include "bnb_launchers.h"

namespace bnb {
namespace {

constexpr int kShrinkWaves = 16;    // wavefronts per workgroup = the K interleave of the summation order
constexpr int kShrinkTile = 8;      // adapter rows per workgroup
constexpr int kShrinkBatch = 8;     // steps of a wavefront whose loads are issued together (16 x 16 bytes in flight per lane)
constexpr int kShrinkMaxSplits = 8; // the grouped call's member cap
constexpr int kShrinkMaxRows = 16, kShrinkMaxRank = 1024, kShrinkMaxPart = 128;
constexpr int kShrinkMaxAdapters = 64; // the mixed-adapter form: adapters in a stack (the grid's second dimension)
constexpr int kShrinkShortK = 4096, kShrinkLongK = 14336; // the K buckets of the predicate (measured at their upper ends)

// the split table, by value in the kernarg segment: r[i] rows in part i, zero behind the last part (no splits: r[0] = R)
struct ShrinkSplits {
    int r[kShrinkMaxSplits];
};

// One workgroup's tile: adapter rows j0 ... j0 + 7 of A against the rows of x. IDS (lora_shrink_ids_kernel): `sel` has bit m set for
// the rows of x that carry this workgroup's adapter, `none` for the rows that this workgroup writes as zeros. The operand lanes of a
// row outside `sel` hold the literal zero and never load; the MFMAs run as before, and a row of an MFMA does not depend on the other
// rows, so a selected row's sum is the uniform kernel's, bit for bit. Only rows in `sel` or `none` are stored.
template <typename T, bool IDS>
__device__ __forceinline__ void shrink_tile(const T* __restrict__ x, const T* __restrict__ A, T* __restrict__ t, int M, int K, const ShrinkSplits& sp,
                                            [[maybe_unused]] uint32_t sel, [[maybe_unused]] uint32_t none) {
    __shared__ __attribute__((aligned(16))) float part[kShrinkWaves][kShrinkTile][16]; // [wavefront][column j][row m]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 15, lg = lane >> 4; // MFMA roles: row of x / adapter row ln, k group lg
    const int j0 = blockIdx.x * kShrinkTile;
    int steps = K >> 5;
    bool x_lane = ln < M;
    if constexpr (IDS) {
        x_lane = ((sel >> ln) & 1u) != 0; // (sel has no bit at or above M)
        if (sel == 0)
            steps = 0; // only rows without an adapter to write: no load at all
    }
    const bool a_lane = ln < kShrinkTile;
    // 16-byte pieces: step s of a row is pieces 4 s ... 4 s + 3, this lane's is 4 s + lg (idle lanes point at row 0 and never load)
    const u32x4* xp = reinterpret_cast<const u32x4*>(x + static_cast<size_t>(x_lane ? ln : 0) * K) + lg;
    const u32x4* ap = reinterpret_cast<const u32x4*>(A + static_cast<size_t>(j0 + (a_lane ? ln : 0)) * K) + lg;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = wave; s0 < steps; s0 += kShrinkWaves * kShrinkBatch) {
        u32x4 xv[kShrinkBatch], av[kShrinkBatch];
#pragma unroll
        for (int u = 0; u < kShrinkBatch; ++u) {
            const int s = s0 + u * kShrinkWaves;
            const bool live = s < steps; // (uniform over the wavefront)
            xv[u] = (live && x_lane) ? xp[s * 4] : zero;
            av[u] = (live && a_lane) ? ap[s * 4] : zero;
        }
#pragma unroll
        for (int u = 0; u < kShrinkBatch; ++u)
            if (s0 + u * kShrinkWaves < steps)
                acc = Mma16x16x32<T>::run(xv[u], av[u], acc);
    }
    // accumulator layout: lane (ln, lg) holds rows m = 4 lg ... 4 lg + 3 of column ln
    if (a_lane)
        *reinterpret_cast<f32x4*>(&part[wave][ln][lg * 4]) = acc;
    __syncthreads();
    if (tid < M * kShrinkTile) {
        const int m = tid >> 3, j = tid & 7;
        if constexpr (IDS) {
            if ((((sel | none) >> m) & 1u) == 0)
                return; // another adapter's row: its workgroups write it
        }
        float sum = part[0][j][m];
#pragma unroll
        for (int w = 1; w < kShrinkWaves; ++w)
            sum += part[w][j][m];
        if constexpr (IDS) {
            if (((sel >> m) & 1u) == 0)
                sum = 0.f; // a row without an adapter
        }
        // the part that holds this tile: rows [base, base + rr) of A, stored as a contiguous [M, rr] matrix at element M * base
        int base = 0, rr = sp.r[0], pre = 0;
#pragma unroll
        for (int i = 0; i < kShrinkMaxSplits; ++i) {
            const int ri = sp.r[i];
            if (j0 >= pre && j0 < pre + ri) {
                base = pre;
                rr = ri;
            }
            pre += ri;
        }
        t[static_cast<size_t>(M) * base + static_cast<size_t>(m) * rr + (j0 + j - base)] = from_f32<T>(sum);
    }
}

template <typename T>
__global__ __launch_bounds__(kShrinkWaves * 64) void lora_shrink_kernel(const T* __restrict__ x, const T* __restrict__ A, T* __restrict__ t, int M,
                                                                        int K, const ShrinkSplits sp) {
    shrink_tile<T, false>(x, A, t, M, K, sp, 0u, 0u);
}

// Mixed-adapter form (bnb_mi355x_lora_shrink_ids): A is [A_n, R, K], ids holds one adapter id per row of x on the DEVICE, and
//     t[m, :] = the uniform kernel's row m for adapter ids[m]        0 <= ids[m] < A_n
//     t[m, :] = 0                                                    otherwise (the row has no adapter)
// Grid (tile of 8 adapter rows, adapter). Every wavefront reads the <= 16 ids itself - one load, two ballots, the result wave-uniform:
// no LDS list, no barrier - and a workgroup whose adapter no row names returns before it requests a byte of A or x. Rows without an
// adapter are written as zeros by the workgroups of adapter 0, so every element of t is written exactly once and a captured graph
// needs no memset node. An id is only ever COMPARED (as a 64-bit value: 2^32 + 1 is out of range, not adapter 1); every address is
// formed from blockIdx.y < A_n.
template <typename T>
__global__ __launch_bounds__(kShrinkWaves * 64) void lora_shrink_ids_kernel(const T* __restrict__ x, const T* __restrict__ A, T* __restrict__ t,
                                                                            const void* __restrict__ ids, int idx64, int M, int R, int K, int A_n,
                                                                            const ShrinkSplits sp) {
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.y;
    long long id = -1;
    if (lane < M)
        id = idx64 ? static_cast<const long long*>(ids)[lane] : static_cast<long long>(static_cast<const int*>(ids)[lane]);
    const bool in_range = id >= 0 && id < static_cast<long long>(A_n);
    const uint32_t sel = static_cast<uint32_t>(__builtin_amdgcn_ballot_w64(lane < M && id == static_cast<long long>(a)));
    const uint32_t none = a == 0 ? static_cast<uint32_t>(__builtin_amdgcn_ballot_w64(lane < M && !in_range)) : 0u;
    if ((sel | none) == 0)
        return; // (uniform over the workgroup: every wavefront computed the same masks)
    shrink_tile<T, true>(x, A + static_cast<size_t>(a) * R * K, t, M, K, sp, sel, none);
}

bool shrink_shape_ok(int dtype, int M, int R, int K) {
    return (dtype == 1 || dtype == 2) && M >= 1 && M <= kShrinkMaxRows && R >= 8 && R <= kShrinkMaxRank && (R % 8) == 0 && K >= 64 && (K % 64) == 0;
}

} // namespace

// Whether bnb_mi355x_lora_shrink serves the shape: the preconditions, minus the classes that the measurements exclude
// (profiles/lora_shrink_bench.txt). Pure host logic.
bool lora_shrink_supported(int dtype, int M, int R, int K) {
    if (!shrink_shape_ok(dtype, M, R, K))
        return false;
    // Measured classes (K bucket x M range; every rank bucket of a class measured alike). K <= 4096: ahead of F.linear in every cell,
    // M = 1 ... 16, and the kernel's time falls with K while the BLAS call stays at its floor. 4096 < K <= 14336: ahead at 2 ... 4
    // rows only - at one row the BLAS gemv is as fast, from 5 rows on a workgroup's stream of x (M K 2 bytes each) outweighs it.
    // Longer rows are not measured.
    if (K <= kShrinkShortK)
        return true;
    return K <= kShrinkLongK && M >= 2 && M <= 4;
}

// the split table of a call (false: not a table the kernel takes)
static bool shrink_split_table(int R, const int* splits, int n_splits, ShrinkSplits& sp) {
    if (n_splits < 0 || n_splits > kShrinkMaxSplits || (n_splits > 0 && splits == nullptr))
        return false;
    sp = {};
    if (n_splits == 0) {
        sp.r[0] = R;
        return true;
    }
    int total = 0;
    for (int i = 0; i < n_splits; ++i) {
        if (splits[i] < 8 || splits[i] > kShrinkMaxPart || (splits[i] % 8) != 0)
            return false;
        sp.r[i] = splits[i];
        total += splits[i];
    }
    return total == R;
}

// One launch; false (nothing launched) outside the preconditions. The predicate above is NOT consulted: an excluded class still
// computes the documented result, it is only not worth a launch of its own.
bool lora_shrink(int dtype, const void* x, const void* lora_a, void* t, int M, int R, int K, const int* splits, int n_splits, hipStream_t stream) {
    ShrinkSplits sp;
    if (!shrink_shape_ok(dtype, M, R, K) || x == nullptr || lora_a == nullptr || t == nullptr || !aligned_to(x, 16) || !aligned_to(lora_a, 16) ||
        !aligned_to(t, 16) || !shrink_split_table(R, splits, n_splits, sp))
        return false;
    const dim3 grid(R / kShrinkTile), block(kShrinkWaves * 64);
    if (dtype == 1)
        hipLaunchKernelGGL(lora_shrink_kernel<f16>, grid, block, 0, stream, static_cast<const f16*>(x), static_cast<const f16*>(lora_a), static_cast<f16*>(t), M,
                           K, sp);
    else
        hipLaunchKernelGGL(lora_shrink_kernel<bf16>, grid, block, 0, stream, static_cast<const bf16*>(x), static_cast<const bf16*>(lora_a),
                           static_cast<bf16*>(t), M, K, sp);
    BNB_CHECK_LAUNCH();
    return true;
}

// Whether bnb_mi355x_lora_shrink_ids serves the shape: the preconditions, minus the classes that the measurements exclude
// (profiles/lora_multi_bench.txt). Pure host logic.
bool lora_shrink_ids_supported(int dtype, int M, int A_n, int R, int K) {
    return shrink_shape_ok(dtype, M, R, K) && A_n >= 1 && A_n <= kShrinkMaxAdapters;
}

// The mixed-adapter launch: lora_a [A_n, R, K], ids [M] on the device (int32 / int64: index_bytes 4 / 8). false (nothing launched)
// outside the preconditions; the predicate above is not consulted.
bool lora_shrink_ids(int dtype, const void* x, const void* lora_a, const void* ids, int index_bytes, void* t, int M, int A_n, int R, int K,
                     const int* splits, int n_splits, hipStream_t stream) {
    ShrinkSplits sp;
    if (!shrink_shape_ok(dtype, M, R, K) || A_n < 1 || A_n > kShrinkMaxAdapters || (index_bytes != 4 && index_bytes != 8) || x == nullptr ||
        lora_a == nullptr || ids == nullptr || t == nullptr || !aligned_to(x, 16) || !aligned_to(lora_a, 16) || !aligned_to(t, 16) ||
        !aligned_to(ids, static_cast<size_t>(index_bytes)) || !shrink_split_table(R, splits, n_splits, sp))
        return false;
    const dim3 grid(R / kShrinkTile, A_n), block(kShrinkWaves * 64);
    if (dtype == 1)
        hipLaunchKernelGGL(lora_shrink_ids_kernel<f16>, grid, block, 0, stream, static_cast<const f16*>(x), static_cast<const f16*>(lora_a),
                           static_cast<f16*>(t), ids, index_bytes == 8 ? 1 : 0, M, R, K, A_n, sp);
    else
        hipLaunchKernelGGL(lora_shrink_ids_kernel<bf16>, grid, block, 0, stream, static_cast<const bf16*>(x), static_cast<const bf16*>(lora_a),
                           static_cast<bf16*>(t), ids, index_bytes == 8 ? 1 : 0, M, R, K, A_n, sp);
    BNB_CHECK_LAUNCH();
    return true;
}

} // namespace bnb
