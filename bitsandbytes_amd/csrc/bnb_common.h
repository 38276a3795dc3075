// bnb_common.h — shared device-side helpers for the MI355X (gfx950 / CDNA4) 4-bit kernels.
//
// This library is written for gfx950 only: wave64, 256 CUs, 160 KiB LDS per CU. There is no CUDA
// path, no hipify layer and no multi-arch dispatch.
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

namespace bnb {

// Loads / stores of the standalone streaming kernels (quantize / dequantize: every byte is touched once). NT selects the
// non-temporal cache policy. Measured on MI355X at 16.7 M elements (profiles/r3_stream_nt_policy_ab.txt): 16-bit quantize4
// 12.4 -> 11.0 us, dequantize4 10.0 -> 9.0, FP4 quantize 15.2 -> 13.3, the 8-bit pair -4 ... -5 %; but fp32 dequantize4
// 20.1 -> 26.7 us (a lane's 32 bytes leave as two 16-byte stores at a 32-byte stride: half lines written around the L2) and
// fp32 quantize4 +2.5 % - so the 4-bit kernels use it for 16-bit tensors only.
template <bool NT, typename V> __device__ __forceinline__ V stream_load(const V* ptr) {
    if constexpr (NT)
        return __builtin_nontemporal_load(ptr);
    else
        return *ptr;
}
template <bool NT, typename V> __device__ __forceinline__ void stream_store(V val, V* ptr) {
    if constexpr (NT)
        __builtin_nontemporal_store(val, ptr);
    else
        *ptr = val;
}

constexpr int kWave = 64;

// quant_type codes on the C ABI (reference csrc/common.h:3-7)
enum QuantType : int { kGeneral8bit = 0, kFP4 = 1, kNF4 = 2 };

// ---------------------------------------------------------------------------------------------
// Error convention of the reference ABI: the C entry points return void; a failed launch prints
// and terminates the process (reference csrc/compat.cuh:78-85, used at csrc/ops.cu:74,93,450).
// ---------------------------------------------------------------------------------------------
#define BNB_HIP_CHECK(expr)                                                                        \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            fprintf(stderr, "bitsandbytes_amd: HIP error %s at %s:%d\n", hipGetErrorString(_e),    \
                    __FILE__, __LINE__);                                                           \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

#define BNB_CHECK_LAUNCH() BNB_HIP_CHECK(hipPeekAtLastError())

// ---------------------------------------------------------------------------------------------
// Dynamic LDS above 64 KiB needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel. The attribute
// belongs to (kernel, device), so it is tracked per device: a process that drives several GPUs must set it
// on each of them. Raised monotonically, never lowered. Host-side; callable from several threads: the fast
// path is one relaxed atomic load, the (rare) raise is serialised so the attribute and the record agree.
// ---------------------------------------------------------------------------------------------
struct LdsLimit {
    static constexpr int kMaxDevices = 64;
    std::atomic<size_t> bytes[kMaxDevices] = {};
    std::mutex raise;
};
inline void ensure_dynamic_lds(LdsLimit& state, const void* kernel, size_t dynamic_bytes, size_t static_bytes = 0) {
    if (dynamic_bytes + static_bytes <= 64 * 1024)
        return;
    int dev = 0;
    BNB_HIP_CHECK(hipGetDevice(&dev));
    dev = (dev >= 0 && dev < LdsLimit::kMaxDevices) ? dev : 0;
    if (dynamic_bytes <= state.bytes[dev].load(std::memory_order_acquire))
        return;
    std::lock_guard<std::mutex> lock(state.raise);
    if (dynamic_bytes > state.bytes[dev].load(std::memory_order_relaxed)) {
        BNB_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(dynamic_bytes)));
        state.bytes[dev].store(dynamic_bytes, std::memory_order_release);
    }
}

// ---------------------------------------------------------------------------------------------
// Tuning knobs (bnb_mi355x_set_tuning / bnb_mi355x_set_stream_tuning: sweeps, tests, tools - every setting computes correct
// results) are THREAD-LOCAL: a tool or test that changes one and forgets to reset it changes the launches of its own thread
// only, never the routing of another thread's calls in the same process. (load / store keep the std::atomic spelling of
// the globals they replace.)
// ---------------------------------------------------------------------------------------------
struct TlsKnob {
    int v;
    int load(std::memory_order = std::memory_order_relaxed) const { return v; }
    void store(int x, std::memory_order = std::memory_order_relaxed) { v = x; }
};

// Which kernel family the calling thread's last gemm_4bit / gemv_4bit call launched (bnb_mi355x_last_gemm_kernel: tests assert
// that the kernel they name is the kernel that ran - a forced geometry that silently falls back to another family is not
// coverage). Written by the launchers themselves, at the point of the launch.
enum GemmKernelId { kKernelNone = 0, kKernelStream = 1, kKernelGeneric = 2, kKernelRt = 3, kKernelPc = 4, kKernelPs = 5, kKernelKq = 6, kKernelSm = 7, kKernelTall = 8, kKernelExperts = 9 };
extern thread_local int g_last_gemm_kernel;

// ---------------------------------------------------------------------------------------------
// Element types. fp16/bf16 travel as their native clang types so that conversions lower to the
// gfx950 hardware converts (v_cvt_f16_f32 / v_cvt_pk_bf16_f32, both round-to-nearest-even).
// ---------------------------------------------------------------------------------------------
using f16 = _Float16;
using bf16 = __bf16;

template <typename T> struct TypeInfo;
template <> struct TypeInfo<float> {
    static constexpr int bytes = 4;
};
template <> struct TypeInfo<f16> {
    static constexpr int bytes = 2;
};
template <> struct TypeInfo<bf16> {
    static constexpr int bytes = 2;
};

template <typename T> __device__ __forceinline__ float to_f32(T v) { return static_cast<float>(v); }
template <typename T> __device__ __forceinline__ T from_f32(float v) { return static_cast<T>(v); }

// ---------------------------------------------------------------------------------------------
// 4-bit code tables (reference bitsandbytes/functional.py:788-823). FP4 is the raw table divided
// by 12 in fp32, exactly as `data.div_(data.abs().max())` does (functional.py:853); entry 8 is
// +0.0 as in the Python table.
// ---------------------------------------------------------------------------------------------
#define BNB_NF4_VALUES                                                                             \
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,                      \
        -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,                 \
        0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,    \
        0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f

#define BNB_FP4_VALUES                                                                             \
    0.0f / 12.0f, 0.0625f / 12.0f, 8.0f / 12.0f, 12.0f / 12.0f, 4.0f / 12.0f, 6.0f / 12.0f,       \
        2.0f / 12.0f, 3.0f / 12.0f, 0.0f / 12.0f, -0.0625f / 12.0f, -8.0f / 12.0f, -12.0f / 12.0f, \
        -4.0f / 12.0f, -6.0f / 12.0f, -2.0f / 12.0f, -3.0f / 12.0f

// Device-resident copies. Deliberately plain __device__ (global address space), not __constant__:
// kernels select between these and a caller-supplied table pointer, and mixing address spaces would
// turn the gather into flat_load, whose completion the compiler can only await with vmcnt(0).
__device__ static const float kNF4Code[16] = {BNB_NF4_VALUES};
__device__ static const float kFP4Code[16] = {BNB_FP4_VALUES};

// explicit global-address-space view of a device pointer (forces global_load, which vmcnt can count)
typedef const float __attribute__((address_space(1))) * gfloat_ptr;

// The reference rounds `code * absmax` to fp32 first and to T second (csrc/cpu_ops.cpp:419-431).
// hipcc would otherwise fuse the multiply and the fp16 convert into v_fma_mix{lo,hi}_f16, which
// rounds once and differs from the two-step result in rare double-rounding cases. An empty asm
// makes the fp32 product an opaque register value: no instruction is emitted, the fusion is blocked.
// The fused epilogues use it the same way, for every fp32 intermediate that two separate torch kernels
// (and the plain form) would have rounded to fp32 before the conversion to T.
__device__ __forceinline__ float rounded_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// The fp32 scale of a double-quantised block, absmax[b] = code2[q] * absmax2 + offset, with the TWO roundings of the host-side
// sequence (dequantize_blockwise, then `+= offset`: reference bitsandbytes/functional.py:1002-1006). Written as
// __fadd_rn(__fmul_rn(c, a), offset) hipcc 7.2 emits ONE v_fma_f32 (the intrinsics are plain * and + by the time the contraction pass
// runs): one rounding, a last-bit difference in ~1/5 of the scales - enough to flip a bf16 output of a 14336-row layer every few
// calls, which is how it was found (the sharded FFN block carries un-nested statistics and is compared bit for bit with the unsharded
// block). The empty asm (not volatile: it may be scheduled freely) makes the product opaque.
__device__ __forceinline__ float nested_scale(float c, float a, float offset) {
    float prod = c * a;
    asm("" : "+v"(prod));
    return prod + offset;
}

// A zero the compiler cannot see through, materialised at the point of the call. Adding it to the
// shift amounts of the nibble/byte extraction ties the whole decode to program order *after* this
// point: without it LLVM hoists the first v_bfe_u32 of the decode above the workgroup barrier and
// into the middle of the load-issue sequence, where its s_waitcnt vmcnt stalls the wavefront for a
// full HBM round trip before the rest of its loads are even issued (seen in the ISA and as +1 us).
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}

// ---------------------------------------------------------------------------------------------
// Device primitives shared by the 4-bit kernels. ONE definition of each: a kernel file uses these names and does not
// re-define them. All are __forceinline__: none leaves a symbol in a code object.
// ---------------------------------------------------------------------------------------------
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;

// Two floats rounded to T (bf16 / f16, round-to-nearest-even) in one dword: `first` in the low half.
template <typename T> __device__ __forceinline__ uint32_t pack2(float first, float second) {
    using V = __attribute__((ext_vector_type(2))) T;
    V v;
    v[0] = static_cast<T>(first);
    v[1] = static_cast<T>(second);
    return __builtin_bit_cast(uint32_t, v);
}

// MFMA traits, T in {bf16, f16}: operands travel as four dwords (eight T) per lane, accumulators in fp32.
template <typename T> struct Mma16x16x32 {
    using frag = __attribute__((ext_vector_type(8))) T;
    static __device__ __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
        if constexpr (std::is_same_v<T, bf16>)
            return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c, 0, 0, 0);
        else
            return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t pack(float first, float second) { return pack2<T>(first, second); }
};
template <typename T> struct Mma32x32x16 {
    using frag = __attribute__((ext_vector_type(8))) T;
    static __device__ __forceinline__ f32x16 run(u32x4 a, u32x4 b, f32x16 c) {
        if constexpr (std::is_same_v<T, bf16>)
            return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c, 0, 0, 0);
        else
            return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t pack(float first, float second) { return pack2<T>(first, second); }
};

// Entry i of the NF4 / FP4 code as a compare/select tree over literals (15 v_cndmask; the inner select is scalar, and folds
// away where fp4 is a compile-time constant): no memory access in front of a kernel's decode-table build.
__device__ __forceinline__ float code_literal(int i, bool fp4) {
    constexpr float nf4[16] = {BNB_NF4_VALUES};
    constexpr float fp4v[16] = {BNB_FP4_VALUES};
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        v = (i == j) ? (fp4 ? fp4v[j] : nf4[j]) : v;
    return v;
}

// Buffer descriptors. kBufferWholeSpace is the record count (bytes, stride 0) of a descriptor that exists for its addressing
// mode and for the out-of-range trick only - every offset a kernel can form legitimately is below 2^31, an offset with the top
// bit set reads zeros and fetches nothing - not for a bounds check against the tensor; a descriptor that does check carries its
// real size. kBufferFlags is word 3 on gfx950: DATA_FORMAT = 32 bits, everything else (swizzle, index stride, add-tid) off.
constexpr int kBufferWholeSpace = 0x7FFFFFFF;
constexpr int kBufferFlags = 0x00020000;
// The same descriptor built by hand as four dwords (base[47:0], stride 0), as the "s" operand of the asm below.
__device__ __forceinline__ i32x4 buffer_rsrc(const void* base) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    return i32x4{static_cast<int>(a), static_cast<int>((a >> 32) & 0xFFFFu), kBufferWholeSpace, kBufferFlags};
}

// LDS-DMA (buffer_load ... lds: 16, 4 or 1 byte per lane from rs + voff + soff straight into LDS at M0 + 16 / 4 / 4 x lane),
// spelled in asm instead of the builtin because the compiler then does NOT know that it is a vector-memory operation. With the
// builtin it treats the vmcnt counter as out of order - every register wait of the kernel's ordinary loads becomes vmcnt(0) -
// and makes every later ds_read wait for ALL outstanding DMA. Unseen, the DMAs leave the compiler's counted waits for the other
// loads counted (a DMA that is YOUNGER than a load the compiler waits for only makes that wait stricter). The price: nothing
// waits for the DMAs themselves, so the kernel writes those waits by hand - wait_vm<N>() below, N = the vector-memory
// operations of the wavefront that may still be in flight, then a barrier where another wavefront reads the data. The LDS base
// and the scalar offset must be wavefront-uniform (they go through readfirstlane into M0 / an SGPR); voff is per lane.
__device__ __forceinline__ void lds_dma16(i32x4 rs, uint32_t lds, uint32_t voff, uint32_t soff) {
    lds = __builtin_amdgcn_readfirstlane(lds);
    soff = __builtin_amdgcn_readfirstlane(soff);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds), "v"(voff), "s"(rs), "s"(soff) : "memory", "m0");
}
// (weights: read once, by one CU - the non-temporal policy shortens issue -> landed by ~18 %, MI355X guide "nt-weights")
__device__ __forceinline__ void lds_dma16_nt(i32x4 rs, uint32_t lds, uint32_t voff, uint32_t soff) {
    lds = __builtin_amdgcn_readfirstlane(lds);
    soff = __builtin_amdgcn_readfirstlane(soff);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen nt lds" ::"s"(lds), "v"(voff), "s"(rs), "s"(soff) : "memory", "m0");
}
__device__ __forceinline__ void lds_dma4(i32x4 rs, uint32_t lds, uint32_t voff) {
    lds = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds" ::"s"(lds), "v"(voff), "s"(rs) : "memory", "m0");
}
__device__ __forceinline__ void lds_dma1(i32x4 rs, uint32_t lds, uint32_t voff) {
    // one byte per lane, landing in the lane's dword slot (the other three bytes are not defined: the reader masks)
    lds = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_ubyte %1, %2, 0 offen lds" ::"s"(lds), "v"(voff), "s"(rs) : "memory", "m0");
}
// Counted wait: returns when at most N vector-memory operations of the wavefront are outstanding (they retire in order).
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ---------------------------------------------------------------------------------------------
// wave64 reductions
// ---------------------------------------------------------------------------------------------
template <int WIDTH> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = 1; off < WIDTH; off <<= 1)
        v = fmaxf(v, __shfl_xor(v, off, kWave));
    return v;
}

// Sum over the 64 lanes, result valid in every lane. All cross-lane traffic stays in the VALU (DPP
// modifiers + v_readlane): no ds_bpermute round trips through the LDS pipe, which measured ~0.5 us
// for the two reductions at the end of the M = 1 gemv (s_memtime timeline, profiles/).
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
    // v + (v moved by DPP control CTRL); all rows/banks enabled, bound_ctrl irrelevant (full wave active)
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
    return v + __builtin_bit_cast(float, moved);
}

__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add<0xB1>(v);  // quad_perm [1,0,3,2]  : lane ^ 1
    v = dpp_add<0x4E>(v);  // quad_perm [2,3,0,1]  : lane ^ 2
    v = dpp_add<0x141>(v); // row_half_mirror      : the other quad of each 8
    v = dpp_add<0x140>(v); // row_mirror           : the other half of each 16-lane row
    // every lane of a row now holds its row sum; combine the four rows through SGPRs
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return (r0 + r1) + (r2 + r3);
}

// C independent wave sums in lock step: every DPP stage runs over all C values before the next one, so the chains
// overlap instead of paying the DPP / readlane hazards C times in a row.
template <int C> __device__ __forceinline__ void wave_sum_n(float (&v)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0xB1>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0x4E>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0x141>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0x140>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[c]), 0));
        const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[c]), 16));
        const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[c]), 32));
        const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[c]), 48));
        v[c] = (r0 + r1) + (r2 + r3);
    }
}

// wave_sum_n with the four rows combined in the vector unit: the same four row steps, then two more DPP adds instead of
// four v_readlane and three adds on SGPR values (a VALU instruction takes one SGPR operand: the compiler adds moves).
//   row_bcast:15, row mask 0xA: lane 15 of row 0 / 2 into every lane of row 1 / 3 -> row 1 = r1 + r0, row 3 = r3 + r2
//   row_bcast:31, row mask 0xC: lane 31 into every lane of rows 2 and 3          -> row 3 = (r3 + r2) + (r1 + r0)
// The association is wave_sum_n's, (r0 + r1) + (r2 + r3), and fp32 addition is commutative: the same bits. The sum is valid
// in LANE 63 ONLY (rows 0 - 2 hold partial sums). Needs the full wave active. Spelled in asm: the rows that the mask leaves
// out keep the destination, which the builtin can only express through a copy; written by hand, the DPP read of a VGPR that
// the VALU has just written needs its two wait states by hand as well (s_nop 1).
template <int C> __device__ __forceinline__ void wave_sum_n_lane63(float (&v)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0xB1>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0x4E>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0x141>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        v[c] = dpp_add<0x140>(v[c]);
#pragma unroll
    for (int c = 0; c < C; ++c)
        asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
            "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
            : "+v"(v[c]));
}

// CU-count override (bnb_mi355x_set_cu_count: tests and tools - every setting computes correct results). A knob like the ones above:
// thread-local, 0 = ask the device. The launch plans of the calling thread are then made for a device of that many compute units -
// what a partitioned MI355X presents (DPX / QPX / CPX: 128 / 64 / 32) - whatever device runs them.
inline thread_local TlsKnob g_cu_count_override{0};

// Compute units of the current device (cached per device); 256 (MI355X) when no device can be queried - the launch-plan
// functions that use it are also reachable from pure size queries (workspace bytes) on a host without a GPU. The override
// above goes first: it neither reads nor writes the per-device cache.
inline int device_cu_count_or_default() {
    const int forced = g_cu_count_override.load(std::memory_order_relaxed);
    if (forced > 0)
        return forced;
    static std::atomic<int> cached[LdsLimit::kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 256;
    }
    const int slot = (dev >= 0 && dev < LdsLimit::kMaxDevices) ? dev : 0;
    int v = cached[slot].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            v = 256;
        }
        cached[slot].store(v, std::memory_order_relaxed);
    }
    return v;
}

static inline int ilog2(int v) {
    int s = 0;
    while ((1 << s) < v)
        ++s;
    return s;
}

static inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

static inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

} // namespace bnb
