// moe_route.hip — the scoring and top-k half of a mixture-of-experts router as ONE launch (gfx950, wave64): the step between the
// router matmul (logits = x · Wr^T, a launch of its own: lora_shrink.hip serves its shape class) and the expert FFN
// (gemm4_experts.hip), which takes this kernel's two outputs as they are.
//
//     p_j   = softmax(l)_j  or  sigmoid(l_j)                         the score,          fp32
//     c_j   = p_j (+ select_bias[j])                                 the selection key,  fp32
//     ids   = the S experts of largest key, best first               int32 [T, S]
//     w_s   = p_{ids[s]} (/ (w_0 + w_1 + ... + w_{S-1})) * scale     fp32  [T, S]        (always the UNBIASED score)
//
// Decomposition. One wavefront owns one token row; four wavefronts share a workgroup and nothing else (no LDS, no barrier, no
// workspace): grid = ceil(T / 4), any T. Lane l holds experts j = l + 64 i, i < NI = ceil(E / 64) rounded up to a power of two
// (<= 16: E <= 1024), in registers; slots with j >= E never take part. Loads are element loads, coalesced over the lanes: the only
// alignment a pointer needs is its element's.
//
// Arithmetic - a function of the row alone (not of T, of the row's place, or of the grid):
//   softmax   m = max_j l_j;  e_j = expf(l_j - m);  Z = sum e_j, lane-local in ascending i, then the xor butterfly 32, 16, ... 1
//             (every lane ends with the same bits: an fp32 add commutes);  p_j = e_j / Z, IEEE division.
//   sigmoid   p_j = 1 / (1 + expf(-l_j)).
//   top-k     S rounds: every lane's best live key, a butterfly on the pair (key, index), the winner leaves. a beats b when
//             c_a > c_b, or c_a == c_b and a < b; a NaN key beats nothing and loses to every other key; among NaN keys the lower
//             index goes first. This is a strict total order on the live experts, so the ids of a row are distinct and in [0, E)
//             whatever the logits hold, and every lane of the butterfly ends with the same winner.
//   weights   sum = w_0 + w_1 + ... in slot order; no epsilon: a zero sum gives what IEEE gives (inf or NaN).
#include "bnb_launchers.h"

#include <climits>

namespace bnb {
namespace {

constexpr int kRouteWaves = 4;          // token rows per workgroup
constexpr int kRouteMaxExperts = 1024;  // 16 register slots per lane
constexpr int kRouteMaxTopK = 16;

// the order of the selection (file head); a dead candidate is (NaN, INT_MAX): it loses to every live one
__device__ __forceinline__ bool route_beats(float ka, int ia, float kb, int ib) {
    const bool na = ka != ka, nb = kb != kb;
    if (na || nb)
        return na == nb ? ia < ib : nb;
    return ka > kb || (ka == kb && ia < ib);
}

template <typename T, int NI>
__global__ __launch_bounds__(kRouteWaves * 64) void moe_topk_kernel(const T* __restrict__ logits, const float* __restrict__ select_bias,
                                                                   int* __restrict__ ids, float* __restrict__ weights, int rows, int E, int S,
                                                                   int sigmoid, int renormalize, float scale) {
    const int lane = threadIdx.x & 63;
    // (unsigned: the last workgroup's rows reach past INT_MAX when `rows` is within three of it)
    const uint32_t row = blockIdx.x * kRouteWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= static_cast<uint32_t>(rows))
        return; // (the whole wavefront: nothing below waits for another one)
    const T* lrow = logits + static_cast<size_t>(row) * E;
    const float nan = __builtin_nanf("");
    float p[NI], c[NI];
    uint32_t live = 0; // bit i: slot i holds an expert that has not been taken
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        p[i] = -__builtin_inff();
        if (j < E) {
            p[i] = to_f32(lrow[j]);
            live |= 1u << i;
        }
    }
    if (sigmoid) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
            p[i] = 1.0f / (1.0f + expf(-p[i]));
    } else {
        float m = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < NI; ++i)
            m = fmaxf(m, p[i]); // (idle slots hold -inf)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            m = fmaxf(m, __shfl_xor(m, d, 64));
        float z = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            p[i] = ((live >> i) & 1u) ? expf(p[i] - m) : 0.f;
            z += p[i];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            z += __shfl_xor(z, d, 64);
#pragma unroll
        for (int i = 0; i < NI; ++i)
            p[i] = p[i] / z;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        c[i] = (select_bias != nullptr && j < E) ? p[i] + select_bias[j] : p[i];
    }
    // lane s keeps slot s of the result; the sum of the chosen scores runs on every lane alike
    int my_id = 0;
    float my_w = 0.f, sum = 0.f;
    for (int s = 0; s < S; ++s) {
        float bk = nan;
        int bi = INT_MAX;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = lane + 64 * i;
            if (((live >> i) & 1u) && route_beats(c[i], j, bk, bi)) {
                bk = c[i];
                bi = j;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ko = __shfl_xor(bk, d, 64);
            const int io = __shfl_xor(bi, d, 64);
            if (route_beats(ko, io, bk, bi)) {
                bk = ko;
                bi = io;
            }
        }
        // bi: the winner on every lane (S <= E: a live expert exists in every round); its lane hands out the score and retires it
        float pw = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (bi == lane + 64 * i) {
                pw = p[i];
                live &= ~(1u << i);
            }
        }
        pw = __shfl(pw, bi & 63, 64);
        sum = s == 0 ? pw : sum + pw;
        if (lane == s) {
            my_id = bi;
            my_w = pw;
        }
    }
    if (lane < S) {
        if (renormalize)
            my_w = my_w / sum;
        my_w = my_w * scale;
        ids[static_cast<size_t>(row) * S + lane] = my_id;
        weights[static_cast<size_t>(row) * S + lane] = my_w;
    }
}

template <typename T>
void moe_topk_launch(const MoeTopkCall& a, hipStream_t stream) {
    const int per_lane = (a.experts + 63) / 64;
    const dim3 grid(static_cast<uint32_t>((static_cast<long long>(a.rows) + kRouteWaves - 1) / kRouteWaves)), block(kRouteWaves * 64);
    const T* logits = static_cast<const T*>(a.logits);
#define BNB_ROUTE_LAUNCH(NI)                                                                                                                    \
    hipLaunchKernelGGL((moe_topk_kernel<T, NI>), grid, block, 0, stream, logits, a.select_bias, a.ids, a.weights, a.rows, a.experts, a.top_k, \
                       a.scoring, a.renormalize, a.scale)
    if (per_lane <= 1)
        BNB_ROUTE_LAUNCH(1);
    else if (per_lane <= 2)
        BNB_ROUTE_LAUNCH(2);
    else if (per_lane <= 4)
        BNB_ROUTE_LAUNCH(4);
    else if (per_lane <= 8)
        BNB_ROUTE_LAUNCH(8);
    else
        BNB_ROUTE_LAUNCH(16);
#undef BNB_ROUTE_LAUNCH
}

// the shape preconditions of bnb_mi355x_moe_topk
bool moe_topk_shape_ok(int dtype, int rows, int experts, int top_k) {
    return dtype >= 0 && dtype <= 2 && rows >= 0 && experts >= 1 && experts <= kRouteMaxExperts && top_k >= 1 && top_k <= kRouteMaxTopK &&
           top_k <= experts;
}

} // namespace

// Whether bnb_mi355x_moe_topk serves the class: the preconditions, minus the classes in which the launch measured behind the torch
// composition it replaces (profiles/moe_route.txt). Pure host logic.
bool moe_topk_supported(int dtype, int rows, int experts, int top_k) { return rows >= 1 && moe_topk_shape_ok(dtype, rows, experts, top_k); }

// One launch (none for rows == 0); false (nothing launched) outside the preconditions. The predicate above is not consulted.
bool moe_topk(const MoeTopkCall& a, hipStream_t stream) {
    if (!moe_topk_shape_ok(a.dtype, a.rows, a.experts, a.top_k) || (a.scoring != 0 && a.scoring != 1))
        return false;
    if (a.rows == 0)
        return true;
    const size_t elt = a.dtype == 0 ? 4 : 2;
    if (a.logits == nullptr || a.ids == nullptr || a.weights == nullptr || !aligned_to(a.logits, elt) || !aligned_to(a.ids, 4) ||
        !aligned_to(a.weights, 4) || !aligned_to(a.select_bias, 4))
        return false;
    if (a.dtype == 0)
        moe_topk_launch<float>(a, stream);
    else if (a.dtype == 1)
        moe_topk_launch<f16>(a, stream);
    else
        moe_topk_launch<bf16>(a, stream);
    BNB_CHECK_LAUNCH();
    return true;
}

} // namespace bnb
