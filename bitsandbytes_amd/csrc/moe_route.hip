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
//
// Group-limited routing (moe_topk_grouped_kernel: DeepSeek-V2 / -V3, GLM): the experts are n_group contiguous groups of G = E / n_group;
// a group's score is its first key in the order above ("max") or first + second key, one fp32 add ("top2sum"); the topk_group groups
// first in the same order on (score, group index) stay, and the S rounds run over their experts only - an expert of a dropped group
// is not live, which is not the same as a key of 0. Scoring, selection and weights are the code above, shared (route_scores,
// route_select); with topk_group == n_group the group stage is skipped and the bits are moe_topk_kernel's.
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

// Scoring (file head): p and c of the lane's experts j = lane + 64 i; returns the live mask (bit i: j < E).
template <typename T, int NI>
__device__ __forceinline__ uint32_t route_scores(const T* __restrict__ lrow, const float* __restrict__ select_bias, int lane, int E, int sigmoid,
                                                 float (&p)[NI], float (&c)[NI]) {
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
    return live;
}

// The S rounds of the selection over the live experts, the weights, and the two stores of the row.
template <int NI>
__device__ __forceinline__ void route_select(const float (&p)[NI], const float (&c)[NI], uint32_t live, int lane, uint32_t row, int S,
                                             int renormalize, float scale, int* __restrict__ ids, float* __restrict__ weights) {
    const float nan = __builtin_nanf("");
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
        // bi: the winner on every lane (a live expert exists in every round: S <= E, and S <= topk_group * G behind the group
        // stage); its lane hands out the score and retires it
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

template <typename T, int NI>
__global__ __launch_bounds__(kRouteWaves * 64) void moe_topk_kernel(const T* __restrict__ logits, const float* __restrict__ select_bias,
                                                                   int* __restrict__ ids, float* __restrict__ weights, int rows, int E, int S,
                                                                   int sigmoid, int renormalize, float scale) {
    const int lane = threadIdx.x & 63;
    // (unsigned: the last workgroup's rows reach past INT_MAX when `rows` is within three of it)
    const uint32_t row = blockIdx.x * kRouteWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= static_cast<uint32_t>(rows))
        return; // (the whole wavefront: nothing below waits for another one)
    float p[NI], c[NI];
    const uint32_t live = route_scores<T, NI>(logits + static_cast<size_t>(row) * E, select_bias, lane, E, sigmoid, p, c);
    route_select<NI>(p, c, live, lane, row, S, renormalize, scale, ids, weights);
}

// ---------------------------------------------------------------------------------------------------------------- the group stage
// x goes before y in the order of the selection as far as the VALUES go (equal keys are one value, whichever index holds it)
__device__ __forceinline__ bool route_value_before(float x, float y) { return y != y ? x == x : x > y; }

// (a1, a2) <- the first two of {a1, a2, b1, b2} in that order; both pairs arrive ordered. The two pairs always stand for DISJOINT
// sets of experts, so a key is never counted twice.
__device__ __forceinline__ void route_merge2(float& a1, float& a2, float b1, float b2) {
    if (route_value_before(b1, a1)) {
        a2 = route_value_before(b2, a1) ? b2 : a1;
        a1 = b1;
    } else {
        a2 = route_value_before(b1, a2) ? b1 : a2;
    }
}

// The groups that stay: bit g of the result, the same on every lane. Group g = experts [g G, (g + 1) G), any G >= 1 (a group may
// straddle lanes and register slots). Per register slot, a segmented Hillis-Steele scan over the lanes (distances 1, 2, ... 32: a lane
// takes from lane - d only inside its own group) leaves, in the last lane a group has in that slot, the best two keys of the group's
// experts there; lane g then fetches group g's piece of every slot it reaches into and merges them. The group score (first key, or
// first + second: one fp32 add) lives in lane g; a group's rank is the number of groups that beat it under route_beats on
// (score, g) - a strict total order, so the ranks are 0 ... n_group - 1 - counted over a loop of wave-uniform lane reads.
template <int NI>
__device__ __forceinline__ uint64_t route_keep_groups(const float (&c)[NI], int lane, int E, int G, int n_group, int topk_group, int top2) {
    const float nan = __builtin_nanf("");
    const int step_r = 64 % G;     // (wave-uniform) how an expert's place in its group moves from one slot to the next
    int r = lane % G;              // the place of expert lane + 64 i in its group
    const int hi = lane * G + G - 1; // lane g: the last expert of group g
    float a1 = nan, a2 = nan;      // lane g: the best two keys of group g (a dead candidate is NaN: it goes behind every key)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (64 * i < E) { // (wave-uniform)
            float k1 = lane + 64 * i < E ? c[i] : nan, k2 = nan;
            const int reach = r < lane ? r : lane; // lanes lane - reach ... lane hold this lane's group in this slot
#pragma unroll
            for (int d = 1; d <= 32; d <<= 1) {
                const float o1 = __shfl_up(k1, d, 64), o2 = __shfl_up(k2, d, 64);
                if (d <= reach)
                    route_merge2(k1, k2, o1, o2);
            }
            const int e = hi - 64 * i; // group g's last lane in this slot (past 63: the group goes on in the next slot)
            const bool hit = lane < n_group && e >= 0 && lane * G <= 64 * i + 63;
            const int src = e < 0 ? 0 : (e > 63 ? 63 : e);
            const float o1 = __shfl(k1, src, 64), o2 = __shfl(k2, src, 64);
            if (hit)
                route_merge2(a1, a2, o1, o2);
            r += step_r;
            r = r >= G ? r - G : r;
        }
    }
    const float score = top2 ? a1 + a2 : a1;
    int rank = 0;
    for (int h = 0; h < n_group; ++h) {
        const float sh = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(score), h));
        rank += route_beats(sh, h, score, lane) ? 1 : 0;
    }
    return __ballot(lane < n_group && rank < topk_group);
}

// moe_topk_kernel with the group stage between the scoring and the selection: the experts of a dropped group leave the live mask.
template <typename T, int NI>
__global__ __launch_bounds__(kRouteWaves * 64) void moe_topk_grouped_kernel(const T* __restrict__ logits, const float* __restrict__ select_bias,
                                                                           int* __restrict__ ids, float* __restrict__ weights, int rows, int E,
                                                                           int S, int sigmoid, int renormalize, float scale, int n_group,
                                                                           int topk_group, int top2) {
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * kRouteWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= static_cast<uint32_t>(rows))
        return;
    float p[NI], c[NI];
    uint32_t live = route_scores<T, NI>(logits + static_cast<size_t>(row) * E, select_bias, lane, E, sigmoid, p, c);
    if (topk_group < n_group) { // (wave-uniform; every group stays otherwise: the bits of moe_topk_kernel)
        const int G = E / n_group;
        const uint64_t keep = route_keep_groups<NI>(c, lane, E, G, n_group, topk_group, top2);
        const int step_q = 64 / G, step_r = 64 % G;
        int q = lane / G, r = lane % G; // expert lane + 64 i: its group and its place in it
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!((keep >> (q & 63)) & 1ull)) // (q >= n_group only where j >= E: not live anyway)
                live &= ~(1u << i);
            q += step_q;
            r += step_r;
            if (r >= G) {
                r -= G;
                ++q;
            }
        }
    }
    route_select<NI>(p, c, live, lane, row, S, renormalize, scale, ids, weights);
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

template <typename T>
void moe_topk_grouped_launch(const MoeTopkGroupedCall& g, hipStream_t stream) {
    const MoeTopkCall& a = g.base;
    const int per_lane = (a.experts + 63) / 64;
    const dim3 grid(static_cast<uint32_t>((static_cast<long long>(a.rows) + kRouteWaves - 1) / kRouteWaves)), block(kRouteWaves * 64);
    const T* logits = static_cast<const T*>(a.logits);
#define BNB_ROUTE_LAUNCH(NI)                                                                                                                 \
    hipLaunchKernelGGL((moe_topk_grouped_kernel<T, NI>), grid, block, 0, stream, logits, a.select_bias, a.ids, a.weights, a.rows, a.experts, \
                       a.top_k, a.scoring, a.renormalize, a.scale, g.n_group, g.topk_group, g.group_score)
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

// the shape preconditions of bnb_mi355x_moe_topk_grouped (group_score: 0 "max", 1 "top2sum")
bool moe_topk_grouped_shape_ok(int dtype, int rows, int experts, int top_k, int n_group, int topk_group, int group_score) {
    if (dtype < 0 || dtype > 2 || rows < 0 || experts < 1 || experts > kRouteMaxExperts || n_group < 1 || n_group > 64 ||
        experts % n_group != 0 || topk_group < 1 || topk_group > n_group || (group_score != 0 && group_score != 1))
        return false;
    const int G = experts / n_group;
    if (group_score == 1 && G < 2)
        return false;
    return top_k >= 1 && top_k <= kRouteMaxTopK && top_k <= topk_group * G; // (topk_group * G <= experts <= 1024)
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

// Whether bnb_mi355x_moe_topk_grouped serves the class: its preconditions, minus the classes in which the launch measured behind the
// torch composition it replaces (profiles/moe_route_grouped.txt). Pure host logic.
bool moe_topk_grouped_supported(int dtype, int rows, int experts, int top_k, int n_group, int topk_group, int group_score) {
    return rows >= 1 && moe_topk_grouped_shape_ok(dtype, rows, experts, top_k, n_group, topk_group, group_score);
}

// One launch (none for rows == 0); false (nothing launched) outside the preconditions. The predicate above is not consulted.
bool moe_topk_grouped(const MoeTopkGroupedCall& g, hipStream_t stream) {
    const MoeTopkCall& a = g.base;
    if (!moe_topk_grouped_shape_ok(a.dtype, a.rows, a.experts, a.top_k, g.n_group, g.topk_group, g.group_score) ||
        (a.scoring != 0 && a.scoring != 1))
        return false;
    if (a.rows == 0)
        return true;
    const size_t elt = a.dtype == 0 ? 4 : 2;
    if (a.logits == nullptr || a.ids == nullptr || a.weights == nullptr || !aligned_to(a.logits, elt) || !aligned_to(a.ids, 4) ||
        !aligned_to(a.weights, 4) || !aligned_to(a.select_bias, 4))
        return false;
    if (a.dtype == 0)
        moe_topk_grouped_launch<float>(g, stream);
    else if (a.dtype == 1)
        moe_topk_grouped_launch<f16>(g, stream);
    else
        moe_topk_grouped_launch<bf16>(g, stream);
    BNB_CHECK_LAUNCH();
    return true;
}

} // namespace bnb
