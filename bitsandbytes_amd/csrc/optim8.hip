// optim8.hip — the 8-bit blockwise optimizers: ONE launch updates one parameter tensor in place (p, state1 + absmax1, and for
// Adam state2 + absmax2). Parity target: the reference CPU backend (bitsandbytes/backends/cpu/ops.py
// _optimizer_update_8bit_blockwise_cpu): dequantize_blockwise, the update in fp32, quantize_blockwise - with the encoder of
// blockwise8.hip (blockwise8_encode.h), so the stored codes and absmax equal quantize_blockwise(new fp32 state) bit for bit.
//
// Split: a wavefront owns one 256-element quantization block, a lane 4 consecutive elements: g and p travel as one 8- / 16-byte load
// and store, the codes of a state as one dword. All loads of a block (g, p, the codes, the old absmax values) are requested before
// the first table look-up, and the loads of the wavefront's NEXT block before this one is computed. The new absmax of a block is a
// wavefront reduction (group_max): no LDS slot, no barrier.
//
// Tables: per workgroup (4 wavefronts), built once - per state the 256-float decode table and the encoder's thr[256] + cell[1024]:
// 6 KiB per state, 12 KiB for Adam, plus the 4 KiB prefix-sum scratch of the build. The grid is persistent - at most
// kOptim8WorkgroupsPerCu workgroups per compute unit, workgroup w's wavefront v takes blocks 4 w + v, + 4 grid, ... - so the table build
// is paid once per workgroup, not once per 1024 elements. No barrier after the build, no workspace, no atomics on global memory.
//
// Arithmetic: fp32, every operation rounded on its own (rounded_f32 makes a result opaque: no product is contracted into the add
// behind it, no sum into the conversion to T), IEEE division and square root (-fhip-fp32-correctly-rounded-divide-sqrt). The
// scalars that depend on step, lr or the betas arrive as fp32 values the host computed in double. The ledger of every optimizer
// is DESIGN.md §3.19; tests/test_gpu_optim8.py restates it with separate torch ops.
//
// STATE = float: fp32 states, no tables, no absmax - the same load / update / store path; serves optimizer_update_32bit.
#include "blockwise8_encode.h"
#include "bnb_launchers.h"

#pragma clang fp contract(off)

namespace bnb {

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return rounded_f32(a * b); }
__device__ __forceinline__ float add_rn(float a, float b) { return rounded_f32(a + b); }
__device__ __forceinline__ float div_rn(float a, float b) { return rounded_f32(a / b); }
__device__ __forceinline__ float sqrt_rn(float a) { return rounded_f32(__builtin_sqrtf(a)); }

// One element of the ledger. s2 is touched by Adam only.
template <int OPT> __device__ __forceinline__ void optim_step(float g, float& p, float& s1, float& s2, const OptimScalars& k) {
    g = mul_rn(g, k.gnorm_scale);
    const bool decay = k.weight_decay > 0.0f;
    if constexpr (OPT == kOptAdam) {
        s1 = add_rn(mul_rn(s1, k.beta1), mul_rn(g, k.one_minus_beta1));
        s2 = add_rn(mul_rn(s2, k.beta2), mul_rn(mul_rn(g, g), k.one_minus_beta2));
        const float d = add_rn(div_rn(sqrt_rn(s2), k.sqrt_correction2), k.eps);
        if (decay)
            p = mul_rn(p, k.decay);
        p = add_rn(p, mul_rn(div_rn(s1, d), k.step_scale));
    } else if constexpr (OPT == kOptLion) {
        if (decay)
            p = mul_rn(p, k.decay);
        const float u = add_rn(mul_rn(s1, k.beta1), mul_rn(g, k.one_minus_beta1));
        const float sgn = (u > 0.0f ? 1.0f : 0.0f) - (u < 0.0f ? 1.0f : 0.0f);
        p = add_rn(p, mul_rn(sgn, k.neg_lr));
        s1 = add_rn(mul_rn(s1, k.beta2), mul_rn(g, k.one_minus_beta2));
    } else {
        if (decay) // L2: the decay enters the gradient
            g = add_rn(g, mul_rn(p, k.weight_decay));
        if constexpr (OPT == kOptMomentum) {
            s1 = (k.step == 1) ? g : add_rn(mul_rn(s1, k.beta1), g);
            p = add_rn(p, mul_rn(s1, k.neg_lr));
        } else {
            if constexpr (OPT == kOptRmsprop)
                s1 = add_rn(mul_rn(s1, k.beta1), mul_rn(mul_rn(g, g), k.one_minus_beta1));
            else // adagrad
                s1 = add_rn(s1, mul_rn(g, g));
            const float d = add_rn(sqrt_rn(s1), k.eps);
            p = add_rn(p, mul_rn(div_rn(g, d), k.neg_lr));
        }
    }
}

// What a lane holds of one block between the loads and the first use: the raw vectors (converting at the load would wait for it).
template <typename T, typename STATE, bool TWO> struct BlockRegs {
    typedef T TV __attribute__((ext_vector_type(4)));
    using SV = std::conditional_t<std::is_same_v<STATE, uint8_t>, uint32_t, f32x4>;
    TV g, p;
    SV s1, s2;
    float absmax1, absmax2;
};

template <typename STATE> __device__ __forceinline__ auto load_state4(const STATE* __restrict__ s, long i, long n, bool vec) {
    if constexpr (std::is_same_v<STATE, uint8_t>) {
        if (vec)
            return stream_load<true>(reinterpret_cast<const uint32_t*>(s + i));
        uint32_t w = 0; // the unaligned / partial form: scalar, as load4 does it
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w |= (i + j < n) ? static_cast<uint32_t>(s[i + j]) << (8 * j) : 0u;
        return w;
    } else {
        if (vec)
            return stream_load<true>(reinterpret_cast<const f32x4*>(s + i));
        f32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = (i + j < n) ? s[i + j] : 0.0f;
        return w;
    }
}

template <typename T, typename STATE, bool TWO>
__device__ __forceinline__ void load_block(BlockRegs<T, STATE, TWO>& b, const OptimUpdateCall& a, long blk, int lane, bool vec_ok) {
    using TV = typename BlockRegs<T, STATE, TWO>::TV;
    const long i = blk * 256 + lane * 4;
    const bool vec = vec_ok && i + 4 <= a.n;
    const T* const g = static_cast<const T*>(a.g);
    const T* const p = static_cast<const T*>(a.p);
    if (vec) {
        b.g = stream_load<true>(reinterpret_cast<const TV*>(g + i));
        b.p = *reinterpret_cast<const TV*>(p + i);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b.g[j] = (i + j < a.n) ? g[i + j] : static_cast<T>(0.0f);
            b.p[j] = (i + j < a.n) ? p[i + j] : static_cast<T>(0.0f);
        }
    }
    b.s1 = load_state4(static_cast<const STATE*>(a.state1), i, a.n, vec);
    if constexpr (TWO)
        b.s2 = load_state4(static_cast<const STATE*>(a.state2), i, a.n, vec);
    if constexpr (std::is_same_v<STATE, uint8_t>) {
        b.absmax1 = a.absmax1[blk];
        if constexpr (TWO)
            b.absmax2 = a.absmax2[blk];
    }
}

// The new fp32 state of a block -> its absmax (written by lane 0) and the lane's four codes, with quantize_blockwise's function:
// inv = 1 / absmax, the 16-bit bin, the count of thresholds at or below it; an all-zero block gives codes 0 and absmax 0.
__device__ __forceinline__ uint32_t encode_block(const float (&s)[4], const uint32_t* thr, const uint32_t* cell, float* absmax_out, int lane) {
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        m = fmaxf(m, fabsf(s[j]));
    m = group_max<64>(m);
    if (lane == 0)
        *absmax_out = m;
    const float inv = 1.0f / m; // m == 0: inf; the codes are forced to 0 below
    uint32_t q4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned q = cell_count(bin_of(s[j], inv), thr, cell); // (bin_of clamps: a NaN or inf state indexes inside the tables)
        q = (m == 0.0f) ? 0u : q;
        q4 |= q << (8 * j);
    }
    return q4;
}

template <typename STATE, typename SV> __device__ __forceinline__ void store_state4(STATE* __restrict__ s, long i, long n, bool vec, SV v) {
    if (vec) {
        stream_store<true>(v, reinterpret_cast<SV*>(s + i));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < n) {
                if constexpr (std::is_same_v<STATE, uint8_t>)
                    s[i + j] = static_cast<uint8_t>(v >> (8 * j));
                else
                    s[i + j] = v[j];
            }
    }
}

constexpr int kSetWords = 256 + 256 + 1024; // per 8-bit state, in LDS: the decode table, thr, cell

template <typename T, int OPT, typename STATE>
__global__ __launch_bounds__(256) void optim8_update_kernel(const OptimUpdateCall a, const int vec_ok) {
    constexpr bool TWO = OPT == kOptAdam;
    constexpr bool Q8 = std::is_same_v<STATE, uint8_t>;
    using Regs = BlockRegs<T, STATE, TWO>;
    const int tid = threadIdx.x, lane = tid & 63;
    const long blocks = (a.n + 255) / 256;
    const long stride = static_cast<long>(gridDim.x) * 4;
    long blk = static_cast<long>(blockIdx.x) * 4 + (tid >> 6);

    // the first block's loads go out before the tables are built: the build hides their latency
    Regs next;
    if (blk < blocks)
        load_block<T, STATE, TWO>(next, a, blk, lane, vec_ok != 0);

    __shared__ __attribute__((aligned(16))) uint32_t tables[Q8 ? (TWO ? 2 : 1) * kSetWords : 1];
    if constexpr (Q8) {
        reinterpret_cast<float*>(tables)[tid] = a.qmap1[tid];
        if constexpr (TWO)
            reinterpret_cast<float*>(tables + kSetWords)[tid] = a.qmap2[tid];
        build_cell_tables(a.qmap1, tables + 256, tables + 512); // (ends with a barrier: the decode tables are visible as well)
        if constexpr (TWO)
            build_cell_tables(a.qmap2, tables + kSetWords + 256, tables + kSetWords + 512);
    }
    const float* const dec1 = reinterpret_cast<const float*>(tables);
    const float* const dec2 = reinterpret_cast<const float*>(tables + (Q8 && TWO ? kSetWords : 0));

    for (; blk < blocks; blk += stride) { // (wavefront-uniform: group_max sees all 64 lanes)
        const Regs cur = next;
        if (blk + stride < blocks)
            load_block<T, STATE, TWO>(next, a, blk + stride, lane, vec_ok != 0);
        const long i = blk * 256 + lane * 4;
        const bool vec = vec_ok && i + 4 <= a.n;
        float s1[4], s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        typename Regs::TV p_out;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (Q8) { // dequantize_blockwise: fp32(code[c] * absmax), one rounding
                s1[j] = mul_rn(dec1[(cur.s1 >> (8 * j)) & 0xFFu], cur.absmax1);
                if constexpr (TWO)
                    s2[j] = mul_rn(dec2[(cur.s2 >> (8 * j)) & 0xFFu], cur.absmax2);
            } else {
                s1[j] = cur.s1[j];
                if constexpr (TWO)
                    s2[j] = cur.s2[j];
            }
            float p = static_cast<float>(cur.p[j]);
            optim_step<OPT>(static_cast<float>(cur.g[j]), p, s1[j], s2[j], a.k);
            p_out[j] = static_cast<T>(p);
            if (!(i + j < a.n)) { // past the end: nothing may enter the block's absmax
                s1[j] = 0.0f;
                s2[j] = 0.0f;
            }
        }
        T* const p = static_cast<T*>(a.p);
        if (vec) {
            *reinterpret_cast<typename Regs::TV*>(p + i) = p_out;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < a.n)
                    p[i + j] = p_out[j];
        }
        if constexpr (Q8) {
            const uint32_t q1 = encode_block(s1, tables + 256, tables + 512, a.absmax1 + blk, lane);
            store_state4(static_cast<uint8_t*>(a.state1), i, a.n, vec, q1);
            if constexpr (TWO) {
                const uint32_t q2 = encode_block(s2, tables + kSetWords + 256, tables + kSetWords + 512, a.absmax2 + blk, lane);
                store_state4(static_cast<uint8_t*>(a.state2), i, a.n, vec, q2);
            }
        } else {
            store_state4(static_cast<float*>(a.state1), i, a.n, vec, f32x4{s1[0], s1[1], s1[2], s1[3]});
            if constexpr (TWO)
                store_state4(static_cast<float*>(a.state2), i, a.n, vec, f32x4{s2[0], s2[1], s2[2], s2[3]});
        }
    }
}

template <typename T, int OPT, typename STATE> void launch_optim8(const OptimUpdateCall& a, hipStream_t stream) {
    const bool two = OPT == kOptAdam;
    const size_t state_align = std::is_same_v<STATE, uint8_t> ? 4 : 16;
    const int vec_ok = aligned_to(a.g, 4 * sizeof(T)) && aligned_to(a.p, 4 * sizeof(T)) && aligned_to(a.state1, state_align) &&
                       (!two || aligned_to(a.state2, state_align));
    const long grid = optimizer_update_grid(a.n);
    hipLaunchKernelGGL((optim8_update_kernel<T, OPT, STATE>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream, a, vec_ok);
}

template <typename T, typename STATE> int launch_by_optimizer(const OptimUpdateCall& a, hipStream_t stream) {
    switch (a.optimizer) {
    case kOptAdam:
        launch_optim8<T, kOptAdam, STATE>(a, stream);
        break;
    case kOptMomentum:
        launch_optim8<T, kOptMomentum, STATE>(a, stream);
        break;
    case kOptRmsprop:
        launch_optim8<T, kOptRmsprop, STATE>(a, stream);
        break;
    case kOptAdagrad:
        launch_optim8<T, kOptAdagrad, STATE>(a, stream);
        break;
    case kOptLion:
        launch_optim8<T, kOptLion, STATE>(a, stream);
        break;
    default:
        return kOptimRefusedOptimizer;
    }
    BNB_CHECK_LAUNCH();
    return kOptimOk;
}

template <typename STATE> int launch_by_dtype(const OptimUpdateCall& a, hipStream_t stream) {
    switch (a.dtype) {
    case 0:
        return launch_by_optimizer<float, STATE>(a, stream);
    case 1:
        return launch_by_optimizer<f16, STATE>(a, stream);
    case 2:
        return launch_by_optimizer<bf16, STATE>(a, stream);
    default:
        return kOptimRefusedDtype;
    }
}

} // namespace

// The persistent grid: 4 blocks of 256 elements per workgroup and pass, at most kOptim8WorkgroupsPerCu workgroups per compute unit.
// (Declared ahead of the launcher template in bnb_launchers.h; bnb_mi355x_optimizer_update_grid reports it to tests and tools.)
long optimizer_update_grid(long n) {
    const long blocks = (n + 255) / 256;
    const long grid = (blocks + 3) / 4;
    const long max_grid = static_cast<long>(kOptim8WorkgroupsPerCu) * device_cu_count_or_default();
    return grid > max_grid ? max_grid : grid;
}

int optimizer_update(int state_bits, const OptimUpdateCall& a, hipStream_t stream) {
    if (a.optimizer < kOptAdam || a.optimizer > kOptLion)
        return kOptimRefusedOptimizer;
    if (a.dtype < 0 || a.dtype > 2)
        return kOptimRefusedDtype;
    const bool two = a.optimizer == kOptAdam, q8 = state_bits == 8;
    if ((state_bits != 8 && state_bits != 32) || a.n < 0 || a.g == nullptr || a.p == nullptr || a.state1 == nullptr || (two && a.state2 == nullptr))
        return kOptimMalformed;
    if (q8 && (a.qmap1 == nullptr || a.absmax1 == nullptr || (two && (a.qmap2 == nullptr || a.absmax2 == nullptr))))
        return kOptimMalformed;
    if (a.n == 0)
        return kOptimOk;
    return q8 ? launch_by_dtype<uint8_t>(a, stream) : launch_by_dtype<float>(a, stream);
}

} // namespace bnb
