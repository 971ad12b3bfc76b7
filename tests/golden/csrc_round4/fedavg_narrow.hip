// fedavg_narrow.hip -- weighted FedAvg over float16 / bfloat16 client values with a 16-bit running sum.
//
// Reference: weighted_aggregation_helper.py:181-236 when the client arrays are float16 (numpy) or
// float16 / bfloat16 tensors (torch): the total keeps the input's 16-bit dtype and every library
// operation rounds to it.  The library sequence, restated per element:
//
//   numpy float16 (NEP 50: the python weight becomes half(w), computed on the host from fp64):
//       first  T = h(v * w)                   numpy half loops compute in fp32 and round once
//       step   T = h(T + h(v * w))            (:210-214, two library operations)
//       SCALE  T = h(T * half(1.0 / count))   (:236)
//   torch CPU float16 / bfloat16 (vectorised kernels, fp32 "opmath"):
//       first  T = r(v * float(w))            mul with a CPU scalar keeps the scalar as float
//       step   T = r(fma(v, r(w), T))         add_(v, alpha=w): alpha cast to the tensor dtype, vec::fmadd
//       DIV    T = r(T / float(count))        div_ with a CPU scalar, fp32 division
//   weigh_by_local_iter=False: first T = v, step T = r(T + v).
//
// The running value lives in an fp32 register but always holds a representable 16-bit value, so partial
// sums chain through 16-bit acc_in / out buffers without changing a bit.  Bytes per element: 2K + 2;
// HBM-bound like the fp32 kernel.  Each lane handles 8 consecutive elements with 16-byte loads when every
// pointer is 16-byte aligned; the remainder and unaligned rows take the per-element loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fedavg_internal.h"

namespace fedavg {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int FMT>
__device__ __forceinline__ float load16(uint16_t b) {
    if constexpr (FMT == FEDAVG_BF16) {
        return __uint_as_float((uint32_t)b << 16);
    } else {
        _Float16 h;
        __builtin_memcpy(&h, &b, 2);
        return (float)h;
    }
}

template <int FMT>
__device__ __forceinline__ uint16_t bits16(float x) {
    if constexpr (FMT == FEDAVG_BF16) {
        // c10::BFloat16 round_to_nearest_even (add the rounding bias, truncate; NaN -> a quiet NaN) is what
        // gfx950's v_cvt_pk_bf16_f32 does in one instruction: equal bits for every non-NaN fp32 input,
        // denormals included (exhaustive check over all 2^32 inputs: tools/bf16_cvt_probe.hip).
        asm volatile("" : "+v"(x));
        const __bf16 h = (__bf16)x;
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    } else {
        // The fp32 value must exist before it is narrowed: without this barrier LLVM folds
        // fptrunc(fma(a, b, c)) into v_fma_mixlo_f16, which rounds the exact result to fp16 ONCE -- torch
        // rounds to fp32 first and then to fp16 (a different result when the fp32 rounding makes a tie).
        asm volatile("" : "+v"(x));
        const _Float16 h = (_Float16)x;  // v_cvt_f16_f32: round to nearest even, fp16 denormals kept
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
}

template <int FMT>
__device__ __forceinline__ float rnd(float x) {
    return load16<FMT>(bits16<FMT>(x));
}

template <int FMT, int OP>
__device__ __forceinline__ float first16(float v, float w) {
    if constexpr (OP == FEDAVG_OP_UNWEIGHTED) {
        return v;
    } else {
        return rnd<FMT>(v * w);
    }
}

// torch-ROCm's float16 add_(v, alpha) on device-resident tensors (FEDAVG_OP_TORCH_DEVICE) in its unrolled
// (non-vector) path: the exact fma rounded once, straight to fp16 (v_fma_mixlo_f16; established against torch
// on the GPU: tools/debug_fp16_device.py), where its vector path and the CPU kernel round to fp32 first.
// Explicit, so that no compiler choice decides it; all three sources are fp32 (op_sel_hi 0), result in the low
// half.
__device__ __forceinline__ float fma_f16_once(float a, float b, float c) {
    uint32_t d = 0;
    asm volatile("v_fma_mixlo_f16 %0, %1, %2, %3" : "+v"(d) : "v"(a), "v"(b), "v"(c));
    return load16<FEDAVG_F16>((uint16_t)(d & 0xffffu));
}

template <int FMT, int OP>
__device__ __forceinline__ float step16(float t, float v, float w) {
    if constexpr (OP == FEDAVG_OP_TORCH) {
        return rnd<FMT>(__builtin_fmaf(v, w, t));
    } else if constexpr (OP == FEDAVG_OP_NUMPY) {
        return rnd<FMT>(t + rnd<FMT>(v * w));
    } else {
        return rnd<FMT>(t + v);
    }
}

template <int FMT, int FIN>
__device__ __forceinline__ float fin16(float t, float s) {
    if constexpr (FIN == FEDAVG_FIN_SCALE) {
        return rnd<FMT>(t * s);
    } else if constexpr (FIN == FEDAVG_FIN_DIV) {
        return rnd<FMT>(t / s);
    } else {
        return t;
    }
}

template <int FMT, int OP, int FIN, bool ACC_IN>
__device__ __forceinline__ float elem16(const RowTableNarrow& tab, int K, const uint16_t* acc_in, int64_t i, float fv) {
    float t;
    int k = 0;
    if constexpr (ACC_IN) {
        t = load16<FMT>(acc_in[i]);
    } else {
        t = first16<FMT, OP>(load16<FMT>(static_cast<const uint16_t*>(tab.rows[0])[i]), tab.w_first[0]);
        k = 1;
    }
    for (; k < K; ++k) t = step16<FMT, OP>(t, load16<FMT>(static_cast<const uint16_t*>(tab.rows[k])[i]), tab.w_step[k]);
    return fin16<FMT, FIN>(t, fv);
}

__device__ __forceinline__ uint16_t half_of(const u32x4& v, int j) {
    return (uint16_t)((v[j >> 1] >> ((j & 1) * 16)) & 0xffffu);
}

template <int FMT, int OP, int FIN, bool ACC_IN, bool VEC>
__global__ void __launch_bounds__(kBlock) fedavg_rows_narrow(const RowTableNarrow tab, const int K,
                                                              const uint16_t* acc_in, uint16_t* out, const int64_t n,
                                                              const float fv) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t done = 0;
    if constexpr (VEC) {
        const int64_t n8 = n / 8;
        for (int64_t g = tid; g < n8; g += stride) {
            float t[8];
            int k = 0;
            if constexpr (ACC_IN) {
                const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(acc_in) + g);
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = load16<FMT>(half_of(a, j));
            } else {
                const u32x4 a = __builtin_nontemporal_load(static_cast<const u32x4*>(tab.rows[0]) + g);
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = first16<FMT, OP>(load16<FMT>(half_of(a, j)), tab.w_first[0]);
                k = 1;
            }
            // four clients' loads in flight before their arrival-ordered arithmetic (as the fp32 kernel)
            for (; k + 4 <= K; k += 4) {
                u32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(static_cast<const u32x4*>(tab.rows[k + u]) + g);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float w = tab.w_step[k + u];
#pragma unroll
                    for (int j = 0; j < 8; ++j) t[j] = step16<FMT, OP>(t[j], load16<FMT>(half_of(v[u], j)), w);
                }
            }
            for (; k < K; ++k) {
                const u32x4 v = __builtin_nontemporal_load(static_cast<const u32x4*>(tab.rows[k]) + g);
                const float w = tab.w_step[k];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = step16<FMT, OP>(t[j], load16<FMT>(half_of(v, j)), w);
            }
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = (uint32_t)bits16<FMT>(fin16<FMT, FIN>(t[2 * j], fv)) |
                       ((uint32_t)bits16<FMT>(fin16<FMT, FIN>(t[2 * j + 1], fv)) << 16);
            }
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(out) + g);
        }
        done = n8 * 8;
    }
    for (int64_t i = done + tid; i < n; i += stride) out[i] = bits16<FMT>(elem16<FMT, OP, FIN, ACC_IN>(tab, K, acc_in, i, fv));
}

// ---------------------------------------------------------------------------------------------
// TILED storage (the engine's slab layout for 16-bit keys): element i of client k lives at
//   bases[k] + (i / 4096) * tile_stride + i % 4096      (16-bit elements)
// A block owns a tile (4096 elements = 8 KiB per client); each lane owns two 8-element groups, so a wave
// reads 1 KiB contiguous per client and group, and one tile's K client segments form one sequential run
// (S * 8 KiB) when the slots are interleaved.  Units below are 8-element groups (u32x4).
// ---------------------------------------------------------------------------------------------
constexpr int kTile16 = 4096;
constexpr int kCpl16 = kTile16 / (8 * kBlock);  // 2
#ifndef FEDAVG_NARROW_BURST_WAVES
#define FEDAVG_NARROW_BURST_WAVES 2  // waves per SIMD the burst kernel is compiled for (register budget)
#endif
#ifndef FEDAVG_NARROW_UNROLL
#define FEDAVG_NARROW_UNROLL 6  // clients whose loads are in flight together (A/B: profiles/r01/narrow_unroll_ab.jsonl)
#endif
// Burst launches under this many clients take groups of 4 (round 4, bf16, groups of 4 against 6: 8 / 12 / 16 clients
// 79.8 / 80.6 / 84.2 % against 77.8 / 77.5 / 82.0 %, but 64 clients 71.0 % against 89.4 %; profiles/r04/s13/)
constexpr int kNarrowUnroll4MaxK = 32;

// One tile's arrival-ordered sum for this lane's kCpl16 8-element groups, packed to the output format.
// GROUPED (the burst form): load groups of UNROLL clients from client 0 on, as fedavg_arith.h tile_sum.
template <int FMT, int OP, int FIN, bool ACC_IN, bool GROUPED = false, int UNROLL = FEDAVG_NARROW_UNROLL>
__device__ __forceinline__ void tile_sum16(u32x4 (&res)[kCpl16], const RowTableNarrow& tab, const int K,
                                           const int64_t off, const int64_t col, const u32x4* acc_in, const int64_t b8,
                                           const int64_t e8, const float fv) {
    float acc[kCpl16][8];
    int k = 0;
    if constexpr (ACC_IN) {
#pragma unroll
        for (int c = 0; c < kCpl16; ++c) {
            const int64_t i = col + c * kBlock;
            const u32x4 a = (i >= b8 && i < e8) ? acc_in[i] : u32x4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[c][j] = load16<FMT>(half_of(a, j));
        }
    }
    if constexpr (GROUPED) {
        for (; k < K; k += UNROLL) {
            u32x4 v[UNROLL][kCpl16];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const u32x4* r = static_cast<const u32x4*>(tab.rows[k + u < K ? k + u : K - 1]) + off;
#pragma unroll
                for (int c = 0; c < kCpl16; ++c) v[u][c] = __builtin_nontemporal_load(r + c * kBlock);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (k + u < K) {
                    if (!ACC_IN && k + u == 0) {
                        const float w = tab.w_first[0];
#pragma unroll
                        for (int c = 0; c < kCpl16; ++c)
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[c][j] = first16<FMT, OP>(load16<FMT>(half_of(v[u][c], j)), w);
                    } else {
                        const float w = tab.w_step[k + u];
#pragma unroll
                        for (int c = 0; c < kCpl16; ++c)
#pragma unroll
                            for (int j = 0; j < 8; ++j)
                                acc[c][j] = step16<FMT, OP>(acc[c][j], load16<FMT>(half_of(v[u][c], j)), w);
                    }
                }
            }
        }
        k = K;
    } else if constexpr (!ACC_IN) {
        const u32x4* r = static_cast<const u32x4*>(tab.rows[0]) + off;
#pragma unroll
        for (int c = 0; c < kCpl16; ++c) {
            const u32x4 a = __builtin_nontemporal_load(r + c * kBlock);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[c][j] = first16<FMT, OP>(load16<FMT>(half_of(a, j)), tab.w_first[0]);
        }
        k = 1;
    }
    for (; k + UNROLL <= K; k += UNROLL) {
        u32x4 v[UNROLL][kCpl16];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const u32x4* r = static_cast<const u32x4*>(tab.rows[k + u]) + off;
#pragma unroll
            for (int c = 0; c < kCpl16; ++c) v[u][c] = __builtin_nontemporal_load(r + c * kBlock);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const float w = tab.w_step[k + u];
#pragma unroll
            for (int c = 0; c < kCpl16; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[c][j] = step16<FMT, OP>(acc[c][j], load16<FMT>(half_of(v[u][c], j)), w);
        }
    }
    for (; k < K; ++k) {
        const u32x4* r = static_cast<const u32x4*>(tab.rows[k]) + off;
        const float w = tab.w_step[k];
#pragma unroll
        for (int c = 0; c < kCpl16; ++c) {
            const u32x4 v = __builtin_nontemporal_load(r + c * kBlock);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[c][j] = step16<FMT, OP>(acc[c][j], load16<FMT>(half_of(v, j)), w);
        }
    }
#pragma unroll
    for (int c = 0; c < kCpl16; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            res[c][j] = (uint32_t)bits16<FMT>(fin16<FMT, FIN>(acc[c][2 * j], fv)) |
                        ((uint32_t)bits16<FMT>(fin16<FMT, FIN>(acc[c][2 * j + 1], fv)) << 16);
}

// per-tile-store form (launch variant bit 3): each tile's results stored as it finishes
template <int FMT, int OP, int FIN, bool ACC_IN>
__global__ void __launch_bounds__(kBlock) fedavg_tiles_narrow(const RowTableNarrow tab, const int K,
                                                               const int64_t tstride8, const u32x4* acc_in,
                                                               u32x4* out, const int64_t b8, const int64_t e8,
                                                               const float fv) {
    constexpr int64_t T8 = (int64_t)kCpl16 * kBlock;
    const int64_t t_last = (e8 - 1) / T8;
    for (int64_t t = b8 / T8 + blockIdx.x; t <= t_last; t += gridDim.x) {
        u32x4 res[kCpl16];
        tile_sum16<FMT, OP, FIN, ACC_IN>(res, tab, K, t * tstride8 + threadIdx.x, t * T8 + threadIdx.x, acc_in, b8, e8, fv);
#pragma unroll
        for (int c = 0; c < kCpl16; ++c) {
            const int64_t i = t * T8 + threadIdx.x + c * kBlock;
            if (i >= b8 && i < e8) __builtin_nontemporal_store(res[c], out + i);
        }
    }
}

// BURST form (the default; fedavg_tiles.h fedavg_tiles_burst_f32x4 has the measurements): TPB tiles per
// block per launch, their packed results held in registers and stored after the block's last tile; client
// loads grouped from client 0 on (bf16 64 x 1e9: 85.6 % against 84.4 % ungrouped and 82.0 % for the per-tile
// form, profiles/r02/ab/narrow_burst_grouped.jsonl).
// TPB_LDS > 0 (the default; burst mode 2): that many more tiles per block, their packed results held in LDS
// (8 KiB per tile; each lane reads back only what it wrote) -- launches (TPB + TPB_LDS) / TPB times longer.
template <int FMT, int OP, int FIN, bool ACC_IN, int TPB, int TPB_LDS = 0, int UNROLL = FEDAVG_NARROW_UNROLL>
__global__ void __launch_bounds__(kBlock)
__attribute__((amdgpu_waves_per_eu(FEDAVG_NARROW_BURST_WAVES, FEDAVG_NARROW_BURST_WAVES))) fedavg_tiles_narrow_burst(const RowTableNarrow tab, const int K, const int64_t tstride8, const u32x4* acc_in, u32x4* out,
                          const int64_t b8, const int64_t e8, const float fv, const int64_t t0, const int64_t t_end) {
    constexpr int64_t T8 = (int64_t)kCpl16 * kBlock;
    u32x4 res[TPB][kCpl16];
    __shared__ u32x4 staged[TPB_LDS > 0 ? TPB_LDS * kCpl16 * kBlock : 1];
#pragma unroll
    for (int m = 0; m < TPB; ++m) {
        const int64_t t = t0 + blockIdx.x + (int64_t)m * gridDim.x;
        if (t < t_end)
            tile_sum16<FMT, OP, FIN, ACC_IN, true, UNROLL>(res[m], tab, K, t * tstride8 + threadIdx.x, t * T8 + threadIdx.x,
                                                   acc_in, b8, e8, fv);
    }
    // the LDS-held tiles in a rolled loop: one more copy of the (long) tile body, not TPB_LDS of them
#pragma unroll 1
    for (int m = TPB; m < TPB + TPB_LDS; ++m) {
        const int64_t t = t0 + blockIdx.x + (int64_t)m * gridDim.x;
        if (t < t_end) {
            u32x4 r[kCpl16];
            tile_sum16<FMT, OP, FIN, ACC_IN, true, UNROLL>(r, tab, K, t * tstride8 + threadIdx.x, t * T8 + threadIdx.x, acc_in,
                                                   b8, e8, fv);
#pragma unroll
            for (int c = 0; c < kCpl16; ++c) staged[((m - TPB) * kCpl16 + c) * kBlock + threadIdx.x] = r[c];
        }
    }
#pragma unroll 1
    for (int m = TPB; m < TPB + TPB_LDS; ++m) {
        const int64_t t = t0 + blockIdx.x + (int64_t)m * gridDim.x;
        if (t < t_end) {
#pragma unroll
            for (int c = 0; c < kCpl16; ++c) {
                const int64_t i = t * T8 + threadIdx.x + c * kBlock;
                if (i >= b8 && i < e8)
                    __builtin_nontemporal_store(staged[((m - TPB) * kCpl16 + c) * kBlock + threadIdx.x], out + i);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < TPB; ++m) {
        const int64_t t = t0 + blockIdx.x + (int64_t)m * gridDim.x;
        if (t < t_end) {
#pragma unroll
            for (int c = 0; c < kCpl16; ++c) {
                const int64_t i = t * T8 + threadIdx.x + c * kBlock;
                if (i >= b8 && i < e8) __builtin_nontemporal_store(res[m][c], out + i);
            }
        }
    }
}

template <int FMT, int OP, int FIN>
static hipError_t launch_t16_a(const RowTableNarrow& tab, int K, int64_t tstride8, const void* acc_in, void* out,
                               int64_t b8, int64_t e8, float fv, int grid, int burst, hipStream_t s, uint64_t* nl) {
    const u32x4* ai = static_cast<const u32x4*>(acc_in);
    u32x4* o = static_cast<u32x4*>(out);
    constexpr int64_t T8 = (int64_t)kCpl16 * kBlock;
    if (burst == 2) {  // default: kBurstTiles in registers + kBurstLdsTiles16 in LDS per block and launch
        // client groups of 4 under kNarrowUnroll4MaxK clients, of FEDAVG_NARROW_UNROLL (6) from there on
        const bool u4 = K < kNarrowUnroll4MaxK;
        return burst_launches(b8 / T8, (e8 - 1) / T8 + 1, grid, kBurstTiles + kBurstLdsTiles16, nl, false,
                              [&](int nb, int64_t t0, int64_t t_end, uint32_t) {
#define FEDAVG_T16_BURST(AI, U)                                                                                        \
    hipLaunchKernelGGL((fedavg_tiles_narrow_burst<FMT, OP, FIN, AI, kBurstTiles, kBurstLdsTiles16, U>), dim3(nb),      \
                       dim3(kBlock), 0, s, tab, K, tstride8, ai, o, b8, e8, fv, t0, t_end)
            if (acc_in && u4) FEDAVG_T16_BURST(true, 4);
            else if (acc_in) FEDAVG_T16_BURST(true, FEDAVG_NARROW_UNROLL);
            else if (u4) FEDAVG_T16_BURST(false, 4);
            else FEDAVG_T16_BURST(false, FEDAVG_NARROW_UNROLL);
#undef FEDAVG_T16_BURST
        });
    }
    if (burst) {
        return burst_launches(b8 / T8, (e8 - 1) / T8 + 1, grid, kBurstTiles, nl, false, [&](int nb, int64_t t0, int64_t t_end, uint32_t) {
            if (acc_in)
                hipLaunchKernelGGL((fedavg_tiles_narrow_burst<FMT, OP, FIN, true, kBurstTiles>), dim3(nb), dim3(kBlock), 0,
                                   s, tab, K, tstride8, ai, o, b8, e8, fv, t0, t_end);
            else
                hipLaunchKernelGGL((fedavg_tiles_narrow_burst<FMT, OP, FIN, false, kBurstTiles>), dim3(nb), dim3(kBlock),
                                   0, s, tab, K, tstride8, ai, o, b8, e8, fv, t0, t_end);
        });
    }
    if (acc_in) {
        hipLaunchKernelGGL((fedavg_tiles_narrow<FMT, OP, FIN, true>), dim3(grid), dim3(kBlock), 0, s, tab, K, tstride8, ai,
                           o, b8, e8, fv);
    } else {
        hipLaunchKernelGGL((fedavg_tiles_narrow<FMT, OP, FIN, false>), dim3(grid), dim3(kBlock), 0, s, tab, K, tstride8,
                           ai, o, b8, e8, fv);
    }
    if (nl) ++*nl;
    return hipGetLastError();
}

template <int FMT, int OP>
static hipError_t launch_t16_f(const RowTableNarrow& tab, int K, int64_t tstride8, const void* acc_in, void* out,
                               int64_t b8, int64_t e8, int fin, float fv, int grid, int burst, hipStream_t s,
                               uint64_t* nl) {
    switch (fin) {
        case FEDAVG_FIN_SCALE:
            return launch_t16_a<FMT, OP, FEDAVG_FIN_SCALE>(tab, K, tstride8, acc_in, out, b8, e8, fv, grid, burst, s, nl);
        case FEDAVG_FIN_DIV:
            return launch_t16_a<FMT, OP, FEDAVG_FIN_DIV>(tab, K, tstride8, acc_in, out, b8, e8, fv, grid, burst, s, nl);
        default:
            return launch_t16_a<FMT, OP, FEDAVG_FIN_NONE>(tab, K, tstride8, acc_in, out, b8, e8, fv, grid, burst, s, nl);
    }
}

template <int FMT>
static hipError_t launch_t16_o(const RowTableNarrow& tab, int K, int64_t tstride8, const void* acc_in, void* out,
                               int64_t b8, int64_t e8, int op, int fin, float fv, int grid, int burst, hipStream_t s,
                               uint64_t* nl) {
    switch (op) {
        case FEDAVG_OP_TORCH_DEVICE:  // same steps; the host keeps alpha in fp32 in the table
        case FEDAVG_OP_TORCH:
            return launch_t16_f<FMT, FEDAVG_OP_TORCH>(tab, K, tstride8, acc_in, out, b8, e8, fin, fv, grid, burst, s, nl);
        case FEDAVG_OP_UNWEIGHTED:
            return launch_t16_f<FMT, FEDAVG_OP_UNWEIGHTED>(tab, K, tstride8, acc_in, out, b8, e8, fin, fv, grid, burst, s,
                                                            nl);
        default:
            return launch_t16_f<FMT, FEDAVG_OP_NUMPY>(tab, K, tstride8, acc_in, out, b8, e8, fin, fv, grid, burst, s, nl);
    }
}

hipError_t launch_tiles_narrow(const RowTableNarrow& tab, int K, int64_t tstride_elems, const void* acc_in, void* out,
                               int64_t begin, int64_t end, int fmt, int op, int fin, float fin_val, int grid,
                               int burst, hipStream_t s, uint64_t* nl) {
    const int64_t ts8 = tstride_elems / 8, b8 = begin / 8, e8 = end / 8;
    if (fmt == FEDAVG_BF16)
        return launch_t16_o<FEDAVG_BF16>(tab, K, ts8, acc_in, out, b8, e8, op, fin, fin_val, grid, burst, s, nl);
    if (fmt == FEDAVG_F16)
        return launch_t16_o<FEDAVG_F16>(tab, K, ts8, acc_in, out, b8, e8, op, fin, fin_val, grid, burst, s, nl);
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// torch's scalar remainder.  torch CPU runs T.add_(v, alpha=w) on float16 / bfloat16 tensors
// (weighted_aggregation_helper.py:207) over the ranges at::parallel_for gives its threads (one range below
// 32768 elements), each through cpu_kernel_vec's vectorized loop -- one fp32 fma, the TORCH step above --
// and, for the last (range length mod 32) elements of the range, through the scalar remainder loop, whose
// c10::Half / c10::BFloat16 operators round the product and the sum separately:  p = r(v * r(w)), T = r(T + p).
// (The first v.mul(w) and the final div_ compute the same in both loops.)  The engine lists those elements;
// fedavg_torch16_tails recomputes them from the same inputs into a side buffer before the tile kernel runs
// (acc_in may alias out), and fedavg_scatter16 writes them over the tile kernel's results after it.
// ---------------------------------------------------------------------------------------------
// DEVICE: the listed elements are those torch-ROCm's float16 add_ runs through its unrolled path (the last
// partial block of its vectorized kernel): one rounding of the exact fma, fma_f16_once.
template <int FMT, int FIN, bool ACC_IN, bool DEVICE>
__global__ void __launch_bounds__(kBlock) fedavg_torch16_tails(const RowTableNarrow tab, const int K, const int64_t tile,
                                                                const int64_t tstride, const int64_t* idx,
                                                                const int64_t m, const uint16_t* acc_in,
                                                                uint16_t* vals, const float fv) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const int64_t i = idx[j];
    const int64_t off = (i / tile) * tstride + i % tile;
    float t;
    int k = 0;
    if constexpr (ACC_IN) {
        t = load16<FMT>(acc_in[i]);
    } else {
        t = first16<FMT, FEDAVG_OP_TORCH>(load16<FMT>(static_cast<const uint16_t*>(tab.rows[0])[off]), tab.w_first[0]);
        k = 1;
    }
    for (; k < K; ++k) {
        const float v = load16<FMT>(static_cast<const uint16_t*>(tab.rows[k])[off]);
        if constexpr (DEVICE)
            t = fma_f16_once(v, tab.w_step[k], t);  // tab.w_step[k] = float(w): torch-ROCm's fp32 opmath alpha
        else
            t = rnd<FMT>(t + rnd<FMT>(v * tab.w_step[k]));  // tab.w_step[k] = r(w): c10 casts alpha to the dtype
    }
    vals[j] = bits16<FMT>(fin16<FMT, FIN>(t, fv));
}

__global__ void __launch_bounds__(kBlock) fedavg_scatter16(const int64_t* idx, const uint16_t* vals, const int64_t m,
                                                            uint16_t* out) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < m) out[idx[j]] = vals[j];
}

template <int FMT, int FIN, bool DEVICE>
static hipError_t launch_tails_a(const RowTableNarrow& tab, int K, int64_t tile, int64_t tstride, const int64_t* idx,
                                 int64_t m, const void* acc_in, void* vals, float fv, int grid, hipStream_t s) {
    const uint16_t* ai = static_cast<const uint16_t*>(acc_in);
    uint16_t* v = static_cast<uint16_t*>(vals);
    if (acc_in)
        hipLaunchKernelGGL((fedavg_torch16_tails<FMT, FIN, true, DEVICE>), dim3(grid), dim3(kBlock), 0, s, tab, K, tile,
                           tstride, idx, m, ai, v, fv);
    else
        hipLaunchKernelGGL((fedavg_torch16_tails<FMT, FIN, false, DEVICE>), dim3(grid), dim3(kBlock), 0, s, tab, K, tile,
                           tstride, idx, m, ai, v, fv);
    return hipGetLastError();
}

template <int FMT, bool DEVICE>
static hipError_t launch_tails_f(const RowTableNarrow& tab, int K, int64_t tile, int64_t tstride, const int64_t* idx,
                                 int64_t m, const void* acc_in, void* vals, int fin, float fv, int grid, hipStream_t s) {
    switch (fin) {  // (FEDAVG_FIN_RECIP arrives as its SCALE form)
        case FEDAVG_FIN_SCALE:
            return launch_tails_a<FMT, FEDAVG_FIN_SCALE, DEVICE>(tab, K, tile, tstride, idx, m, acc_in, vals, fv, grid, s);
        case FEDAVG_FIN_DIV:
            return launch_tails_a<FMT, FEDAVG_FIN_DIV, DEVICE>(tab, K, tile, tstride, idx, m, acc_in, vals, fv, grid, s);
        default:
            return launch_tails_a<FMT, FEDAVG_FIN_NONE, DEVICE>(tab, K, tile, tstride, idx, m, acc_in, vals, fv, grid, s);
    }
}

hipError_t launch_torch16_tails(const RowTableNarrow& tab, int K, int64_t tile, int64_t tstride, const int64_t* idx,
                                int64_t m, const void* acc_in, void* vals, int fmt, int op, int fin, float fin_val,
                                hipStream_t s) {
    const int grid = (int)((m + kBlock - 1) / kBlock);
    if (grid == 0) return hipSuccess;
    if (op == FEDAVG_OP_TORCH_DEVICE) {  // float16 only: bfloat16 has no single-rounding path in torch-ROCm
        if (fmt != FEDAVG_F16) return hipErrorInvalidValue;
        return launch_tails_f<FEDAVG_F16, true>(tab, K, tile, tstride, idx, m, acc_in, vals, fin, fin_val, grid, s);
    }
    if (fmt == FEDAVG_BF16)
        return launch_tails_f<FEDAVG_BF16, false>(tab, K, tile, tstride, idx, m, acc_in, vals, fin, fin_val, grid, s);
    if (fmt == FEDAVG_F16)
        return launch_tails_f<FEDAVG_F16, false>(tab, K, tile, tstride, idx, m, acc_in, vals, fin, fin_val, grid, s);
    return hipErrorInvalidValue;
}

hipError_t launch_scatter16(const int64_t* idx, const void* vals, int64_t m, void* out, hipStream_t s) {
    const int grid = (int)((m + kBlock - 1) / kBlock);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(fedavg_scatter16, dim3(grid), dim3(kBlock), 0, s, idx, static_cast<const uint16_t*>(vals), m,
                       static_cast<uint16_t*>(out));
    return hipGetLastError();
}

template <int FMT, int OP, int FIN, bool ACC_IN>
static hipError_t launch_n_v(const RowTableNarrow& tab, int K, const void* acc_in, void* out, int64_t n, float fv,
                             int grid, bool vec, hipStream_t s) {
    if (vec) {
        hipLaunchKernelGGL((fedavg_rows_narrow<FMT, OP, FIN, ACC_IN, true>), dim3(grid), dim3(kBlock), 0, s, tab, K,
                           static_cast<const uint16_t*>(acc_in), static_cast<uint16_t*>(out), n, fv);
    } else {
        hipLaunchKernelGGL((fedavg_rows_narrow<FMT, OP, FIN, ACC_IN, false>), dim3(grid), dim3(kBlock), 0, s, tab, K,
                           static_cast<const uint16_t*>(acc_in), static_cast<uint16_t*>(out), n, fv);
    }
    return hipGetLastError();
}

template <int FMT, int OP, int FIN>
static hipError_t launch_n_a(const RowTableNarrow& tab, int K, const void* acc_in, void* out, int64_t n, float fv,
                             int grid, bool vec, hipStream_t s) {
    return acc_in ? launch_n_v<FMT, OP, FIN, true>(tab, K, acc_in, out, n, fv, grid, vec, s)
                  : launch_n_v<FMT, OP, FIN, false>(tab, K, acc_in, out, n, fv, grid, vec, s);
}

template <int FMT, int OP>
static hipError_t launch_n_f(const RowTableNarrow& tab, int K, const void* acc_in, void* out, int64_t n, int fin,
                             float fv, int grid, bool vec, hipStream_t s) {
    switch (fin) {
        case FEDAVG_FIN_SCALE:
            return launch_n_a<FMT, OP, FEDAVG_FIN_SCALE>(tab, K, acc_in, out, n, fv, grid, vec, s);
        case FEDAVG_FIN_DIV:
            return launch_n_a<FMT, OP, FEDAVG_FIN_DIV>(tab, K, acc_in, out, n, fv, grid, vec, s);
        default:
            return launch_n_a<FMT, OP, FEDAVG_FIN_NONE>(tab, K, acc_in, out, n, fv, grid, vec, s);
    }
}

template <int FMT>
static hipError_t launch_n_o(const RowTableNarrow& tab, int K, const void* acc_in, void* out, int64_t n, int op, int fin,
                             float fv, int grid, bool vec, hipStream_t s) {
    switch (op) {
        case FEDAVG_OP_TORCH_DEVICE:
        case FEDAVG_OP_TORCH:
            return launch_n_f<FMT, FEDAVG_OP_TORCH>(tab, K, acc_in, out, n, fin, fv, grid, vec, s);
        case FEDAVG_OP_UNWEIGHTED:
            return launch_n_f<FMT, FEDAVG_OP_UNWEIGHTED>(tab, K, acc_in, out, n, fin, fv, grid, vec, s);
        default:
            return launch_n_f<FMT, FEDAVG_OP_NUMPY>(tab, K, acc_in, out, n, fin, fv, grid, vec, s);
    }
}

hipError_t launch_rows_narrow(const RowTableNarrow& tab, int K, const void* acc_in, void* out, int64_t n, int fmt,
                              int op, int fin, float fin_val, int grid, hipStream_t s) {
    bool vec = reinterpret_cast<uintptr_t>(out) % 16 == 0 && reinterpret_cast<uintptr_t>(acc_in) % 16 == 0;
    for (int k = 0; vec && k < K; ++k) vec = reinterpret_cast<uintptr_t>(tab.rows[k]) % 16 == 0;
    if (fmt == FEDAVG_BF16) return launch_n_o<FEDAVG_BF16>(tab, K, acc_in, out, n, op, fin, fin_val, grid, vec, s);
    if (fmt == FEDAVG_F16) return launch_n_o<FEDAVG_F16>(tab, K, acc_in, out, n, op, fin, fin_val, grid, vec, s);
    return hipErrorInvalidValue;
}

}  // namespace fedavg
