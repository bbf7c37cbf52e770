// Optimizer updates: 8-bit blockwise states, 8-bit states with one global maximum per state
// tensor, and 32-bit states, gfx950.
//
//   8-bit blockwise  kOptimizerStatic8bit2StateBlockwise  ref:sycl/sycl_code/kernel_quant.cpp:2715-2972
//                    kOptimizerStatic8bit1StateBlockwise  ref:sycl/sycl_code/kernel_quant.cpp:2977-3208
//                    launcher optimizerStatic8bitBlockwise ref:sycl/sycl_code/op_quant.cpp:1135-1240
//                    C-ABI c<name>_8bit_blockwise_grad_<T> ref:sycl/pythonInterface.cpp:264-284
//   32-bit           kOptimizer32bit2State / 1State       ref:sycl/sycl_code/kernel_quant.cpp:1614-2060
//                    C-ABI c<name>32bit_grad_<T>          ref:sycl/pythonInterface.cpp:223-241
//   8-bit global max kPreconditionOptimizerStatic8bit{2,1}State, kOptimizerStatic8bit{2,1}State
//                                                         ref:sycl/sycl_code/kernel_quant.cpp:2030-2645
//                    launcher optimizerStatic8bit         ref:sycl/sycl_code/op_quant.cpp:930-1130
//                    C-ABI c<name>_static_8bit_grad_<T>   ref:sycl/pythonInterface.cpp:243-263
//   norms            kPercentileClipping                  ref:sycl/sycl_code/kernel_quant.cpp:2653-2703
//                    kPreconditionOptimizer32bit{2,1}State ref:sycl/sycl_code/kernel_quant.cpp:1500-1608, 1775-1880
//                    C-ABI cpercentile_clipping_g<T>      ref:sycl/pythonInterface.cpp:284-285
//
// Semantics are the reference's formulas, op for op in fp32 (build: -ffp-contract=off), with the
// intended behaviour where the reference is defective:
//   * the state re-quantiser is the dynamic-map binary search with midpoint rounding that
//     quantize_2D performs upstream (kernel_quant.cpp:840-888 compares against 0 instead of the code
//     after the first step, Q21); with code[255] == 1 it equals dQuantize<0>, quantize_dynamic8 here;
//   * 1-state optimizers are selected by the enum of ops.h:68-76 (MOMENTUM 1, RMSPROP 2, ADAGRAD 4,
//     LION 5); the reference's kernel switches on 1/2/3/4, so ADAGRAD runs the Lion update and LION
//     runs none (Q22);
//   * tail elements of the last 2048-block are loaded as the upstream defaults (g = 0, state1 code
//     128, state2 code 0) and never stored; the reference loads past n (Q2-style, Q23);
//   * the gradient and update norms are fixed-order fp64 sums that overwrite their destination; the
//     reference accumulates them with float atomics (Q24) into a float it zeroes first, for unorm
//     with std::memset on the device pointer (Q25); max_unorm is refused for Lion and Adagrad (Q26, Q27);
//   * the departures of the global-max 8-bit path (Q28-Q35) are listed above its kernels.
// sqrt is __builtin_sqrtf, which hipcc lowers to the correctly rounded sequence (v_sqrt_f32 + two fma
// residual checks); __fsqrt_rn lowers to the bare 1-ulp v_sqrt_f32 on ROCm 7.2.
// The bias corrections are computed once on the host in double (the reference's pow(float, int)
// promotes to double) and rounded to fp32, as the oracle does.
//
// MI355X design: 16 B/element of HBM traffic for Adam fp32 8-bit (g, p read+write, two state bytes
// read+write), but VALU-bound in practice (a wave64 VALU op issues over 4 cycles; ~1450 per
// wave-block in the first version).  A 256-thread workgroup walks 2048-element blocks (grid = 4x the
// resident workgroups) with the next block's loads in flight; 8 contiguous elements per thread
// (16/32-B vector loads); the maps in LDS in the search layout of common.hpp DynMapView (branch-free,
// level-synchronous Eytzinger search, 3 VALU per level); the re-quantisation quotient via an fp64
// reciprocal product (exact, see requant8); one barrier per block for both absmax reductions.
// Lab (tools/optim_lab.hip, 2^27 fp32 elements): 920 us -> 676-689 us, bit-identical to the scalar form.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>
#include <vector>

namespace bnb {

enum OptimizerKind { ADAM = 0, MOMENTUM = 1, RMSPROP = 2, LARS = 3, ADAGRAD = 4, LION = 5 };   // ref ops.h:68-76

constexpr int OPT_BLOCK = 2048, OPT_THREADS = 256, OPT_NPT = 8;

struct OptScalars {
  float beta1, beta2, eps, lr, weight_decay, gnorm_scale;
  float step_size;      // (-lr * correction2) / correction1
  float c2eps;          // correction2 * eps
  float decay;          // 1 - lr * weight_decay
  int step;
  bool skip_zeros;
};

__device__ __forceinline__ float sgnf(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }

// 8 contiguous elements of T <-> fp32 (vector accesses when the whole group is in range and aligned)
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ src, long long i, int n, float (&v)[8], float fill) {
  if (i + 8 <= n && (((uintptr_t)(src + i)) & 15) == 0) {
    if constexpr (sizeof(T) == 4) {
      const float4 a = reinterpret_cast<const float4*>(src + i)[0], b = reinterpret_cast<const float4*>(src + i)[1];
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
      const uint4 u = *reinterpret_cast<const uint4*>(src + i);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[2 * j] = Io<T>::to_f32(__builtin_bit_cast(T, (uint16_t)(w[j] & 0xFFFF)));
        v[2 * j + 1] = Io<T>::to_f32(__builtin_bit_cast(T, (uint16_t)(w[j] >> 16)));
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (i + j < n) ? Io<T>::to_f32(src[i + j]) : fill;
  }
}
template <typename T>
__device__ __forceinline__ void store8(T* __restrict__ dst, long long i, int n, const T (&v)[8]) {
  if (i + 8 <= n && (((uintptr_t)(dst + i)) & 15) == 0) {
    if constexpr (sizeof(T) == 4) {
      reinterpret_cast<float4*>(dst + i)[0] = make_float4(v[0], v[1], v[2], v[3]);
      reinterpret_cast<float4*>(dst + i)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w[j] = (uint32_t)__builtin_bit_cast(uint16_t, v[2 * j]) | ((uint32_t)__builtin_bit_cast(uint16_t, v[2 * j + 1]) << 16);
      *reinterpret_cast<uint4*>(dst + i) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i + j < n) dst[i + j] = v[j];
  }
}
__device__ __forceinline__ void load8u(const uint8_t* __restrict__ src, long long i, int n, uint32_t (&c)[8], uint32_t fill) {
  if (i + 8 <= n && (((uintptr_t)(src + i)) & 7) == 0) {
    const uint2 u = *reinterpret_cast<const uint2*>(src + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = (u.x >> (8 * j)) & 0xFF; c[4 + j] = (u.y >> (8 * j)) & 0xFF; }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = (i + j < n) ? src[i + j] : fill;
  }
}
// 8 state bytes packed little-endian in a uint2 (tail bytes = fill)
__device__ __forceinline__ uint2 load8u_packed(const uint8_t* __restrict__ src, long long i, int n, uint32_t fill) {
  if (i + 8 <= n && (((uintptr_t)(src + i)) & 7) == 0) return *reinterpret_cast<const uint2*>(src + i);
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j >> 2] |= ((i + j < n) ? (uint32_t)src[i + j] : fill) << (8 * (j & 3));
  return make_uint2(w[0], w[1]);
}
__device__ __forceinline__ void store8u(uint8_t* __restrict__ dst, long long i, int n, const uint32_t (&c)[8]) {
  if (i + 8 <= n && (((uintptr_t)(dst + i)) & 7) == 0) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo |= (c[j] & 0xFF) << (8 * j); hi |= (c[4 + j] & 0xFF) << (8 * j); }
    *reinterpret_cast<uint2*>(dst + i) = make_uint2(lo, hi);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i + j < n) dst[i + j] = (uint8_t)c[j];
  }
}

// re-quantise a state value against its block absmax; the signed map keeps the sign of the value
// (kernel_quant.cpp:2930-2941)
template <bool SIGNED, class Code>
__device__ __forceinline__ uint32_t requant(Code code, float s, float absmax) {
  uint32_t c = quantize_dynamic8(code, __fdiv_rn(s, absmax));
  if (SIGNED && ((__float_as_uint(code[c]) ^ __float_as_uint(s)) >> 31)) c = (s > 0.0f) ? ((c + 1) & 0xFF) : ((c - 1) & 0xFF);
  return c;
}

// the same for the 8 values of a thread, searches interleaved (common.hpp dynmap_quantize_n)
template <bool SIGNED>
__device__ __forceinline__ void requant8(DynMapView code, const float (&s)[8], float absmax, uint32_t (&c)[8]) {
  // x = RN32(s / absmax) as (float)(s * RN64(1 / absmax)): 3 VALU instead of the ~11 of the fp32
  // division.  Exact: the fp64 product is within 2^-52 (relative) of s / absmax, while a quotient of
  // two 24-bit floats that is not itself a rounding midpoint lies at least 2^-49 from every midpoint
  // (s - m * absmax is a non-zero multiple of 2^(e_m + e_absmax) against |m * absmax| < 2^(49 + e_m +
  // e_absmax)), and an exact midpoint would need a 25-bit odd significand times a 24-bit one to fit in
  // 24 bits.  So the final rounding to fp32 lands where the IEEE division does (0/0 and x/inf alike).
  const double r64 = 1.0 / (double)absmax;
  float x[8], cq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = (float)((double)s[j] * r64);
  dynmap_quantize_n<8, SIGNED>(code, x, c, cq);
  if (SIGNED) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if ((__float_as_uint(cq[j]) ^ __float_as_uint(s[j])) >> 31) c[j] = (s[j] > 0.0f) ? ((c[j] + 1) & 0xFF) : ((c[j] - 1) & 0xFF);
  }
}

// The maps live in LDS in the search layout of common.hpp DynMapView (breadth-first pivots, the
// final pick's records, the plain map for dequantisation).
template <bool TWO>
struct OptLds {
  float map1[DYNMAP_FLOATS], map2[TWO ? DYNMAP_FLOATS : 1];
  float xch[2][8];                               // double-buffered by block parity
};

// block max of two values over the workgroup with one barrier: xch alternates between two buffers
// by block parity, so the reads of block i finish (every wave passes block i+1's barrier) before
// block i+2 writes the same buffer
__device__ __forceinline__ void block_max256x2(float& a, float& b, float* xch) {
  a = wave_max_xor(a, 64);
  b = wave_max_xor(b, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { xch[wave] = a; xch[4 + wave] = b; }
  __syncthreads();
  a = fmaxf(fmaxf(xch[0], xch[1]), fmaxf(xch[2], xch[3]));
  b = fmaxf(fmaxf(xch[4], xch[5]), fmaxf(xch[6], xch[7]));
}

// one thread's inputs of a 2048-block, kept packed while in flight (the prefetch of the next block)
template <typename T>
struct Opt2InT {
  float gv[8], pv[8];
  uint2 c1, c2;
  float am1, am2;
  __device__ __forceinline__ void load(const T* __restrict__ g, const T* __restrict__ p, const uint8_t* __restrict__ s1,
                                       const uint8_t* __restrict__ s2, const float* __restrict__ a1,
                                       const float* __restrict__ a2, long long blk, int n) {
    const long long i0 = blk * OPT_BLOCK + (long long)threadIdx.x * OPT_NPT;
    load8(g, i0, n, gv, 0.0f);
    c1 = load8u_packed(s1, i0, n, 0x80u);
    if (s2) c2 = load8u_packed(s2, i0, n, 0u);
    load8(p, i0, n, pv, 0.0f);
    am1 = a1[blk];
    am2 = a2 ? a2[blk] : 0.0f;
  }
  __device__ __forceinline__ void unpack(float (&g)[8], float (&p)[8], uint32_t (&q1)[8], uint32_t (&q2)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      g[j] = gv[j];
      p[j] = pv[j];
      q1[j] = ((j < 4 ? c1.x : c1.y) >> (8 * (j & 3))) & 0xFF;
      q2[j] = ((j < 4 ? c2.x : c2.y) >> (8 * (j & 3))) & 0xFF;
    }
  }
};

// ---------------------------------------------------------------- 8-bit blockwise, two states (Adam)
// FL (design lab only; 0 in the library): 1 = no re-quantisation, 2 = division only (timings of the
// parts), 8 = the scalar one-search-at-a-time re-quantiser
template <typename T, int OPT, int FL = 0>
__global__ void __launch_bounds__(OPT_THREADS)
k_optimizer_8bit_blockwise_2state(T* __restrict__ p, const T* __restrict__ g, uint8_t* __restrict__ state1,
                                  uint8_t* __restrict__ state2, const float* __restrict__ qmap1,
                                  const float* __restrict__ qmap2, float* __restrict__ absmax1,
                                  float* __restrict__ absmax2, OptScalars k, int n) {
  __shared__ __attribute__((aligned(16))) OptLds<true> L;
  dynmap_stage(L.map1, qmap1);
  dynmap_stage(L.map2, qmap2);
  __syncthreads();
  const DynMapView code1{reinterpret_cast<const char*>(L.map1)}, code2{reinterpret_cast<const char*>(L.map2)};
  const long long nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  // software pipeline over the grid-stride loop: the next block's inputs are in flight while this
  // block's search runs (without it the HBM stream idles during the search, ~2x the HBM time)
  Opt2InT<T> in;
  long long blk = blockIdx.x;
  if (blk < nb) in.load(g, p, state1, state2, absmax1, absmax2, blk, n);
  for (int par = 0; blk < nb; blk += gridDim.x, par ^= 1) {
    const long long i0 = blk * OPT_BLOCK + (long long)threadIdx.x * OPT_NPT;
    float gv[8], pv[8], s1[8], s2[8];
    uint32_t c1[8], c2[8];
    in.unpack(gv, pv, c1, c2);
    const float am1 = in.am1, am2 = in.am2;
    if (blk + gridDim.x < nb) in.load(g, p, state1, state2, absmax1, absmax2, blk + gridDim.x, n);
    float m1 = -FLT_MAX, m2 = -FLT_MAX;
    bool ok[8];
    const float omb1 = __fsub_rn(1.0f, k.beta1), omb2 = __fsub_rn(1.0f, k.beta2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {                // branch-free: non-finite gradients select 0 states
      ok[j] = __builtin_isfinite(gv[j]);
      const float gs = __fmul_rn(gv[j], k.gnorm_scale);
      const float d2 = __fmul_rn(code2[c2[j]], am2), d1 = __fmul_rn(code1[c1[j]], am1);
      s2[j] = ok[j] ? __fadd_rn(__fmul_rn(d2, k.beta2), __fmul_rn(__fmul_rn(omb2, gs), gs)) : 0.0f;
      s1[j] = ok[j] ? __fadd_rn(__fmul_rn(d1, k.beta1), __fmul_rn(omb1, gs)) : 0.0f;
      m1 = fmaxf(m1, fabsf(s1[j]));
      m2 = fmaxf(m2, fabsf(s2[j]));
    }
    block_max256x2(m1, m2, L.xch[par]);
    if (threadIdx.x == 0) { absmax1[blk] = m1; absmax2[blk] = m2; }
    T po[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float upd = __fmul_rn(k.step_size, __fdiv_rn(s1[j], __fadd_rn(__builtin_sqrtf(s2[j]), k.c2eps)));
      T pt = Io<T>::from_f32(__fadd_rn(pv[j], upd));
      if (k.weight_decay > 0.0f) pt = Io<T>::from_f32(__fmul_rn(Io<T>::to_f32(pt), k.decay));
      po[j] = ok[j] ? pt : Io<T>::from_f32(pv[j]);
    }
    store8(p, i0, n, po);
    if constexpr (FL == 0) {
      requant8<true>(code1, s1, m1, c1);
      requant8<false>(code2, s2, m2, c2);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (FL & 1) {
          c1[j] = __float_as_uint(s1[j]) >> 24;
          c2[j] = __float_as_uint(s2[j]) >> 24;
        } else if (FL & 2) {                     // division only
          c1[j] = __float_as_uint(__fdiv_rn(s1[j], m1)) >> 24;
          c2[j] = __float_as_uint(__fdiv_rn(s2[j], m2)) >> 24;
        } else {                                 // FL 8: one search at a time (the scalar form)
          c1[j] = requant<true>(code1, s1[j], m1);
          c2[j] = requant<false>(code2, s2[j], m2);
        }
      }
    }
    store8u(state1, i0, n, c1);
    store8u(state2, i0, n, c2);
  }
}

// ---------------------------------------------------------------- 8-bit blockwise, one state
template <typename T, int OPT>
__global__ void __launch_bounds__(OPT_THREADS)
k_optimizer_8bit_blockwise_1state(T* __restrict__ p, const T* __restrict__ g, uint8_t* __restrict__ state1,
                                  const float* __restrict__ qmap1, float* __restrict__ absmax1, OptScalars k, int n) {
  __shared__ __attribute__((aligned(16))) OptLds<false> L;
  dynmap_stage(L.map1, qmap1);
  __syncthreads();
  const DynMapView code1{reinterpret_cast<const char*>(L.map1)};
  const long long nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  Opt2InT<T> in;                                 // software pipeline, as the 2-state kernel
  long long blk = blockIdx.x;
  if (blk < nb) in.load(g, p, state1, nullptr, absmax1, nullptr, blk, n);
  for (int par = 0; blk < nb; blk += gridDim.x, par ^= 1) {
    const long long i0 = blk * OPT_BLOCK + (long long)threadIdx.x * OPT_NPT;
    float gv[8], pv[8], s1[8], gl[8];
    uint32_t c1[8], c2[8];
    in.unpack(gv, pv, c1, c2);
    const float am1 = in.am1;
    if (blk + gridDim.x < nb) in.load(g, p, state1, nullptr, absmax1, nullptr, blk + gridDim.x, n);
    float m1 = -FLT_MAX, m2 = 0.0f;
    bool upd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gs = __fmul_rn(gv[j], k.gnorm_scale);
      upd[j] = !k.skip_zeros || gv[j] != 0.0f;
      s1[j] = __fmul_rn(code1[c1[j]], am1);        // skipped elements keep their dequantised state
      gl[j] = gv[j];
      if (upd[j]) {
        if (k.weight_decay > 0.0f) {
          if (OPT == LION) pv[j] = Io<T>::to_f32(Io<T>::from_f32(__fmul_rn(pv[j], k.decay)));
          else gs = __fadd_rn(gs, __fmul_rn(pv[j], k.weight_decay));
        }
        if (OPT == MOMENTUM) {
          s1[j] = (k.step == 1) ? gs : __fadd_rn(__fmul_rn(s1[j], k.beta1), gs);
        } else if (OPT == LION) {
          // the smoothed sign is kept in T, as the reference stores it in g_vals (kernel_quant.cpp:3095)
          gl[j] = Io<T>::to_f32(Io<T>::from_f32(
              __fmul_rn(k.lr, sgnf(__fadd_rn(__fmul_rn(s1[j], k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), gs))))));
          s1[j] = __fadd_rn(__fmul_rn(s1[j], k.beta2), __fmul_rn(__fsub_rn(1.0f, k.beta2), gs));
        } else if (OPT == RMSPROP) {
          s1[j] = __fadd_rn(__fmul_rn(s1[j], k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), __fmul_rn(gs, gs)));
        } else {   // ADAGRAD
          s1[j] = __fadd_rn(s1[j], __fmul_rn(gs, gs));
        }
      }
      m1 = fmaxf(m1, fabsf(s1[j]));
    }
    block_max256x2(m1, m2, L.xch[par]);
    if (threadIdx.x == 0) absmax1[blk] = m1;
    T po[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pn = pv[j];
      if (upd[j]) {
        if (OPT == MOMENTUM) pn = __fsub_rn(pv[j], __fmul_rn(k.lr, s1[j]));
        else if (OPT == LION) pn = __fsub_rn(pv[j], gl[j]);
        else pn = __fsub_rn(pv[j], __fmul_rn(k.lr, __fdiv_rn(gl[j], __fadd_rn(__builtin_sqrtf(s1[j]), k.eps))));
      }
      po[j] = Io<T>::from_f32(pn);
    }
    store8(p, i0, n, po);
    requant8<true>(code1, s1, m1, c1);
    store8u(state1, i0, n, c1);
  }
}

// ---------------------------------------------------------------- deterministic sums of squares
// The full-tensor L2 norms ahead of the element-wise update: the gradient norm of percentile clipping
// (kPercentileClipping, kernel_quant.cpp:2653-2703) and the norm of the trial update of max_unorm
// (kPreconditionOptimizer32bit{2,1}State, kernel_quant.cpp:1500-1608, 1775-1880).  The reference adds
// one fp32 partial per workgroup into a single float with an atomic, so its sum depends on the order
// in which workgroups retire.  Here the summation order is a function of n alone:
//
//   1. the tensor is cut into chunks of NORM_CHUNK = 4096 elements; slot b (0 <= b < NORM_SLOTS = 1024)
//      takes chunks b, b + 1024, b + 2048, ... in that order.  Workgroup b of k_sumsq_partials owns
//      slot b; the grid is min(chunks, 1024), whatever the device.
//   2. inside a chunk, thread t (0..255) takes elements [8t, 8t + 8) and then [2048 + 8t, 2048 + 8t + 8),
//      each group in index order, and adds every term to one fp64 accumulator as it goes (elements
//      at or past n add +0.0).  A term is the exact fp64 square of the gradient, or the fp32 square of
//      the trial update converted to fp64.
//   3. the 256 accumulators of a workgroup are summed by wg_sum256: in each wave a butterfly over lane
//      distances 32, 16, 8, 4, 2, 1 (lane i adds the value of lane i ^ d; fp addition commutes, so all
//      lanes hold the same bits), then (w0 + w1) + (w2 + w3) over the four waves.  Thread 0 writes the
//      slot with a plain store.
//   4. k_sumsq_finish, one workgroup on the same stream: thread t adds slots t, t + 256, t + 512,
//      t + 768 in that order, the same wg_sum256 follows, and the total is rounded once to fp32.
//
// No atomics anywhere.  The slots (8 KB of fp64) live in a workspace the library owns per (device,
// stream): launches on one stream are ordered, two streams never share slots.  The finishing step is a
// launch of its own rather than a prologue of every update workgroup; that A/B and the achieved
// bandwidth (fp32, 2^24 elements: 5.7 TB/s, 71 % of HBM peak) are in DESIGN.md §4.
constexpr int NORM_CHUNK = 4096, NORM_SLOTS = 1024;
constexpr int NORM_GRAD = -1;                      // the kind beside ADAM / MOMENTUM / RMSPROP

struct NormScalars {
  float beta1, beta2, eps, gnorm_scale;
  float pc1, pc2;       // Adam's 1 / (1 - beta^step), kernel_quant.cpp:1522-1523
  int step;
};

__device__ __forceinline__ double wg_sum256(double v, double* xch) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) xch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (xch[0] + xch[1]) + (xch[2] + xch[3]);
}

template <typename T, int KIND>
__global__ void __launch_bounds__(OPT_THREADS)
k_sumsq_partials(const T* __restrict__ g, const float* __restrict__ state1, const float* __restrict__ state2,
                 NormScalars k, int n, double* __restrict__ partials) {
  __shared__ double xch[4];
  const long long chunks = ((long long)n + NORM_CHUNK - 1) / NORM_CHUNK;
  double acc = 0.0;
  for (long long c = blockIdx.x; c < chunks; c += NORM_SLOTS) {
    const long long i0 = c * NORM_CHUNK + (long long)threadIdx.x * OPT_NPT;
    float gv[2][8], s1[2][8], s2[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                  // both halves' loads in flight before the arithmetic
      load8(g, i0 + h * OPT_BLOCK, n, gv[h], 0.0f);
      if (KIND != NORM_GRAD) load8(state1, i0 + h * OPT_BLOCK, n, s1[h], 0.0f);
      if (KIND == ADAM) load8(state2, i0 + h * OPT_BLOCK, n, s2[h], 0.0f);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        double term;
        if (KIND == NORM_GRAD) {
          const double d = (double)gv[h][j];
          term = d * d;                            // exact: 48 significant bits
        } else {
          // op for op kernel_quant.cpp:1577-1590 (two states), 1834-1855 (one state); no weight decay and no
          // skip_zeros in the precondition, as there
          const float gt = Io<T>::to_f32(Io<T>::from_f32(__fmul_rn(k.gnorm_scale, gv[h][j])));
          float u;
          if (KIND == ADAM) {
            float a = __fadd_rn(__fmul_rn(s1[h][j], k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), gt));
            float b = __fadd_rn(__fmul_rn(s2[h][j], k.beta2), __fmul_rn(__fsub_rn(1.0f, k.beta2), __fmul_rn(gt, gt)));
            a = __fmul_rn(a, k.pc1);
            b = __fmul_rn(b, k.pc2);
            u = __fdiv_rn(a, __fadd_rn(__builtin_sqrtf(b), k.eps));
          } else if (KIND == MOMENTUM) {
            u = (k.step == 1) ? gt : __fadd_rn(__fmul_rn(s1[h][j], k.beta1), gt);
          } else {   // RMSPROP
            const float a = __fadd_rn(__fmul_rn(s1[h][j], k.beta1), __fmul_rn(__fmul_rn(__fsub_rn(1.0f, k.beta1), gt), gt));
            u = __fdiv_rn(gt, __fadd_rn(__builtin_sqrtf(a), k.eps));
          }
          term = (double)__fmul_rn(u, u);
        }
        acc += (i0 + h * OPT_BLOCK + j < n) ? term : 0.0;
      }
    }
  }
  const double total = wg_sum256(acc, xch);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// sums the slots and writes (float)total to out[first .. first + count), count <= 256
__global__ void __launch_bounds__(OPT_THREADS)
k_sumsq_finish(const double* __restrict__ partials, int slots, float* __restrict__ out, int first, int count) {
  __shared__ double xch[4];
  double acc = 0.0;
  for (int s = threadIdx.x; s < slots; s += OPT_THREADS) acc += partials[s];
  const double total = wg_sum256(acc, xch);
  if ((int)threadIdx.x < count) out[first + threadIdx.x] = (float)total;
}

// ---------------------------------------------------------------- 8-bit states, one global max per state
// kPreconditionOptimizerStatic8bit{2,1}State + kOptimizerStatic8bit{2,1}State (kernel_quant.cpp:2030-2645): each state
// tensor is quantised against one fp32 maximum.  A step is three stream-ordered launches, no atomics, no memset:
//
//   1. k_static8_precondition walks the tensor in the chunk and slot order of k_sumsq_partials, dequantises the old
//      state with max[0], forms the new fp32 state values (static8_state, the function the update calls too) and
//      keeps per thread max |s1|, max |s2| and, with max_unorm > 0, the fp64 sum of the squared update terms.  Elements
//      at or past n give -FLT_MAX and +0.0.  Workgroup b writes slot b of the workspace: three doubles per slot, laid
//      out as three arrays of NORM_SLOTS (sum, max1, max2; a float maximum is exact in a double).
//   2. k_static8_finish, one workgroup: the sum in the order of k_sumsq_finish, the maxima with fmaxf; it overwrites
//      new_max1[0], new_max2[0] and (max_unorm > 0) unorm[0].
//   3. k_optimizer_8bit_static has the structure of the blockwise kernels (2048-element blocks, the next block's loads
//      in flight, resident_grid); it reads max, new_max and unorm from device memory, re-quantises against new_max
//      and stores p and the state bytes.
//
// The arithmetic is the reference's static kernels op for op in fp32, with the departures of DESIGN.md §2 Q28-Q35:
// every element below n is updated, new_max is overwritten each step, the quotient is the IEEE division of requant8,
// the precondition sees the weight-decayed state the update stores (so new_max is the exact maximum of what is
// quantised), momentum's state takes the scaled and decayed gradient, Adam's decayed weight is not multiplied by
// update_scale, and max_unorm is refused for RMSprop and Lion.
template <int OPT>
__device__ __forceinline__ void static8_state(const OptScalars& k, float g, float p, float d1, float d2, float& gs,
                                              float& s1, float& s2) {
  gs = __fmul_rn(k.gnorm_scale, g);
  s2 = 0.0f;
  if (OPT == ADAM) {
    s1 = __fadd_rn(__fmul_rn(d1, k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), gs));
    s2 = __fadd_rn(__fmul_rn(d2, k.beta2), __fmul_rn(__fmul_rn(__fsub_rn(1.0f, k.beta2), gs), gs));
  } else {
    if ((OPT == MOMENTUM || OPT == RMSPROP) && k.weight_decay > 0.0f) gs = __fadd_rn(gs, __fmul_rn(p, k.weight_decay));
    if (OPT == MOMENTUM) s1 = (k.step == 1) ? gs : __fadd_rn(__fmul_rn(d1, k.beta1), gs);
    else if (OPT == LION) s1 = __fadd_rn(__fmul_rn(d1, k.beta2), __fmul_rn(__fsub_rn(1.0f, k.beta2), gs));
    else s1 = __fadd_rn(__fmul_rn(d1, k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), __fmul_rn(gs, gs)));   // RMSPROP
  }
}

template <typename T, int OPT>
__global__ void __launch_bounds__(OPT_THREADS)
k_static8_precondition(const T* __restrict__ g, const T* __restrict__ p, const uint8_t* __restrict__ state1,
                       const uint8_t* __restrict__ state2, const float* __restrict__ qmap1,
                       const float* __restrict__ qmap2, const float* __restrict__ max1,
                       const float* __restrict__ max2, OptScalars k, float pc1, float pc2, bool want_unorm, int n,
                       double* __restrict__ ws) {
  __shared__ float map1[256], map2[OPT == ADAM ? 256 : 1];
  __shared__ double xch[4];
  __shared__ float xm[8];
  map1[threadIdx.x] = qmap1[threadIdx.x];
  if (OPT == ADAM) map2[threadIdx.x] = qmap2[threadIdx.x];
  __syncthreads();
  const float mx1 = max1[0], mx2 = (OPT == ADAM) ? max2[0] : 0.0f;
  // only the weight-decayed gradient of momentum and RMSprop depends on p
  const bool need_p = (OPT == MOMENTUM || OPT == RMSPROP) && k.weight_decay > 0.0f;
  const long long chunks = ((long long)n + NORM_CHUNK - 1) / NORM_CHUNK;
  double acc = 0.0;
  float m1 = -FLT_MAX, m2 = -FLT_MAX;
  for (long long c = blockIdx.x; c < chunks; c += NORM_SLOTS) {
    const long long i0 = c * NORM_CHUNK + (long long)threadIdx.x * OPT_NPT;
    float gv[2][8], pv[2][8];
    uint32_t c1[2][8], c2[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                  // both halves' loads in flight before the arithmetic
      load8(g, i0 + h * OPT_BLOCK, n, gv[h], 0.0f);
      load8u(state1, i0 + h * OPT_BLOCK, n, c1[h], 0x80u);
      if (OPT == ADAM) load8u(state2, i0 + h * OPT_BLOCK, n, c2[h], 0u);
      if (need_p) load8(p, i0 + h * OPT_BLOCK, n, pv[h], 0.0f);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool inside = i0 + h * OPT_BLOCK + j < n;
        const float d1 = __fmul_rn(map1[c1[h][j]], mx1);
        const float d2 = (OPT == ADAM) ? __fmul_rn(map2[c2[h][j]], mx2) : 0.0f;
        float gs, s1, s2;
        static8_state<OPT>(k, gv[h][j], need_p ? pv[h][j] : 0.0f, d1, d2, gs, s1, s2);
        m1 = fmaxf(m1, inside ? fabsf(s1) : -FLT_MAX);
        if (OPT == ADAM) m2 = fmaxf(m2, inside ? fabsf(s2) : -FLT_MAX);
        if ((OPT == ADAM || OPT == MOMENTUM) && want_unorm) {
          float u = s1;                            // momentum: the state is the update (kernel_quant.cpp:2445-2446)
          if (OPT == ADAM)                         // kernel_quant.cpp:2142-2147
            u = __fdiv_rn(__fmul_rn(s1, pc1), __fadd_rn(__builtin_sqrtf(__fmul_rn(s2, pc2)), k.eps));
          acc += inside ? (double)__fmul_rn(u, u) : 0.0;
        }
      }
    }
  }
  const double total = wg_sum256(acc, xch);
  block_max256x2(m1, m2, xm);
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = total;
    ws[NORM_SLOTS + blockIdx.x] = (double)m1;
    ws[2 * NORM_SLOTS + blockIdx.x] = (double)m2;
  }
}

// reduces the slots; new_max2 and unorm may be null (one state, max_unorm == 0)
__global__ void __launch_bounds__(OPT_THREADS)
k_static8_finish(const double* __restrict__ ws, int slots, float* __restrict__ new_max1, float* __restrict__ new_max2,
                 float* __restrict__ unorm) {
  __shared__ double xch[4];
  __shared__ float xm[8];
  double acc = 0.0;
  float m1 = -FLT_MAX, m2 = -FLT_MAX;
  for (int s = threadIdx.x; s < slots; s += OPT_THREADS) {
    acc += ws[s];
    m1 = fmaxf(m1, (float)ws[NORM_SLOTS + s]);
    m2 = fmaxf(m2, (float)ws[2 * NORM_SLOTS + s]);
  }
  const double total = wg_sum256(acc, xch);
  block_max256x2(m1, m2, xm);
  if (threadIdx.x == 0) {
    new_max1[0] = m1;
    if (new_max2 != nullptr) new_max2[0] = m2;
    if (unorm != nullptr) unorm[0] = (float)total;
  }
}

// one thread's inputs of a 2048-block while in flight (Opt2InT without the per-block absmax)
template <typename T>
struct Static8InT {
  float gv[8], pv[8];
  uint2 c1, c2;
  __device__ __forceinline__ void load(const T* __restrict__ g, const T* __restrict__ p, const uint8_t* __restrict__ s1,
                                       const uint8_t* __restrict__ s2, long long blk, int n) {
    const long long i0 = blk * OPT_BLOCK + (long long)threadIdx.x * OPT_NPT;
    load8(g, i0, n, gv, 0.0f);
    c1 = load8u_packed(s1, i0, n, 0x80u);
    c2 = s2 ? load8u_packed(s2, i0, n, 0u) : make_uint2(0u, 0u);
    load8(p, i0, n, pv, 0.0f);
  }
};

// `unorm` is null when max_unorm == 0; `bound` = max_unorm * param_norm (no eps in the static kernels,
// kernel_quant.cpp:2211-2217, 2499-2505)
template <typename T, int OPT>
__global__ void __launch_bounds__(OPT_THREADS)
k_optimizer_8bit_static(T* __restrict__ p, const T* __restrict__ g, uint8_t* __restrict__ state1,
                        uint8_t* __restrict__ state2, const float* __restrict__ qmap1, const float* __restrict__ qmap2,
                        const float* __restrict__ max1, const float* __restrict__ max2,
                        const float* __restrict__ new_max1, const float* __restrict__ new_max2,
                        const float* __restrict__ unorm, float bound, OptScalars k, int n) {
  __shared__ __attribute__((aligned(16))) OptLds<OPT == ADAM> L;
  dynmap_stage(L.map1, qmap1);
  if (OPT == ADAM) dynmap_stage(L.map2, qmap2);
  __syncthreads();
  const DynMapView code1{reinterpret_cast<const char*>(L.map1)}, code2{reinterpret_cast<const char*>(L.map2)};
  const long long nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  Static8InT<T> in;                              // software pipeline, as the blockwise kernels
  long long blk = blockIdx.x;
  if (blk < nb) in.load(g, p, state1, state2, blk, n);
  const float mx1 = max1[0], nm1 = new_max1[0];
  const float mx2 = (OPT == ADAM) ? max2[0] : 0.0f, nm2 = (OPT == ADAM) ? new_max2[0] : 0.0f;
  float update_scale = 1.0f;
  if (unorm != nullptr) {
    const float un = __builtin_sqrtf(unorm[0]);
    if (un > bound) update_scale = __fdiv_rn(bound, un);
  }
  for (; blk < nb; blk += gridDim.x) {
    const long long i0 = blk * OPT_BLOCK + (long long)threadIdx.x * OPT_NPT;
    float gv[8], pv[8], s1[8], s2[8];
    uint32_t c1[8], c2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      gv[j] = in.gv[j];
      pv[j] = in.pv[j];
      c1[j] = ((j < 4 ? in.c1.x : in.c1.y) >> (8 * (j & 3))) & 0xFF;
      c2[j] = ((j < 4 ? in.c2.x : in.c2.y) >> (8 * (j & 3))) & 0xFF;
    }
    if (blk + gridDim.x < nb) in.load(g, p, state1, state2, blk + gridDim.x, n);
    T po[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d1 = __fmul_rn(code1[c1[j]], mx1);
      const float d2 = (OPT == ADAM) ? __fmul_rn(code2[c2[j]], mx2) : 0.0f;
      float gs;
      static8_state<OPT>(k, gv[j], pv[j], d1, d2, gs, s1[j], s2[j]);
      if (OPT == ADAM) {
        const float upd = __fmul_rn(__fmul_rn(update_scale, k.step_size),
                                    __fdiv_rn(s1[j], __fadd_rn(__builtin_sqrtf(s2[j]), k.c2eps)));
        po[j] = Io<T>::from_f32(__fadd_rn(pv[j], upd));
        if (k.weight_decay > 0.0f) po[j] = Io<T>::from_f32(__fmul_rn(Io<T>::to_f32(po[j]), k.decay));
      } else if (OPT == MOMENTUM) {
        po[j] = Io<T>::from_f32(__fadd_rn(pv[j], __fmul_rn(__fmul_rn(-k.lr, update_scale), s1[j])));
      } else if (OPT == LION) {                  // kernel_quant.cpp:2583-2585, 2601-2604
        float pd = pv[j];
        if (k.weight_decay > 0.0f) pd = Io<T>::to_f32(Io<T>::from_f32(__fmul_rn(pv[j], k.decay)));
        const float t = __fadd_rn(__fmul_rn(d1, k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), gs));
        po[j] = Io<T>::from_f32(__fsub_rn(pd, __fmul_rn(k.lr, sgnf(t))));
      } else {                                   // RMSPROP, kernel_quant.cpp:2605-2608
        po[j] = Io<T>::from_f32(
            __fsub_rn(pv[j], __fdiv_rn(__fmul_rn(k.lr, gs), __fadd_rn(__builtin_sqrtf(s1[j]), k.eps))));
      }
    }
    store8(p, i0, n, po);
    requant8<true>(code1, s1, nm1, c1);
    store8u(state1, i0, n, c1);
    if (OPT == ADAM) {
      requant8<false>(code2, s2, nm2, c2);
      store8u(state2, i0, n, c2);
    }
  }
}

// ---------------------------------------------------------------- 32-bit states
// kOptimizer32bit2State / 1State; gradients are rounded to T after scaling (and after weight decay for
// one state), as the reference keeps them in g_vals.  update_scale (kernel_quant.cpp:1635-1641,
// 1897-1903) is formed on the device from unorm[0], which k_sumsq_finish wrote on this stream, after
// the thread's loads are issued (its square root and division then hide behind them; ahead of the loads
// they cost the max_unorm == 0 path 1 %); `bound` is max_unorm * param_norm (+ eps for one state).
// unorm == nullptr (max_unorm == 0) gives 1.0f, and the products by it are exact.
template <typename T, int OPT>
__global__ void __launch_bounds__(OPT_THREADS)
k_optimizer_32bit(T* __restrict__ p, const T* __restrict__ g, float* __restrict__ state1, float* __restrict__ state2,
                  OptScalars k, const float* __restrict__ unorm, float bound, int n) {
  const long long i0 = ((long long)blockIdx.x * OPT_THREADS + threadIdx.x) * OPT_NPT;
  if (i0 >= n) return;
  float gv[8], pv[8], s1[8], s2[8];
  load8(g, i0, n, gv, 0.0f);
  load8(p, i0, n, pv, 0.0f);
  load8(state1, i0, n, s1, 0.0f);
  if (OPT == ADAM) load8(state2, i0, n, s2, 0.0f);
  float update_scale = 1.0f;
  if (unorm != nullptr) {
    const float un = __builtin_sqrtf(unorm[0]);
    if (un > bound) update_scale = __fdiv_rn(bound, un);
  }
  T po[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float gt = Io<T>::to_f32(Io<T>::from_f32(__fmul_rn(k.gnorm_scale, gv[j])));
    if (OPT != ADAM && k.weight_decay > 0.0f) gt = Io<T>::to_f32(Io<T>::from_f32(__fadd_rn(gt, __fmul_rn(pv[j], k.weight_decay))));
    float pn = pv[j];
    if (!k.skip_zeros || gt != 0.0f) {
      if (OPT == ADAM) {
        s1[j] = __fadd_rn(__fmul_rn(s1[j], k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), gt));
        s2[j] = __fadd_rn(__fmul_rn(s2[j], k.beta2), __fmul_rn(__fsub_rn(1.0f, k.beta2), __fmul_rn(gt, gt)));
        pn = Io<T>::to_f32(Io<T>::from_f32(
            __fadd_rn(pv[j], __fmul_rn(__fmul_rn(update_scale, k.step_size),
                                       __fdiv_rn(s1[j], __fadd_rn(__builtin_sqrtf(s2[j]), k.c2eps))))));
        if (k.weight_decay > 0.0f) pn = __fmul_rn(pn, k.decay);
      } else if (OPT == MOMENTUM) {
        s1[j] = (k.step == 1) ? gt : __fadd_rn(__fmul_rn(s1[j], k.beta1), gt);
        pn = __fadd_rn(pv[j], __fmul_rn(update_scale, -__fmul_rn(k.lr, s1[j])));
      } else if (OPT == LION) {
        pn = __fsub_rn(pv[j], __fmul_rn(k.lr, sgnf(__fadd_rn(__fmul_rn(s1[j], k.beta1), __fmul_rn(__fsub_rn(1.0f, k.beta1), gt)))));
        s1[j] = __fadd_rn(__fmul_rn(s1[j], k.beta2), __fmul_rn(__fsub_rn(1.0f, k.beta2), gt));
      } else if (OPT == RMSPROP) {
        s1[j] = __fadd_rn(__fmul_rn(s1[j], k.beta1), __fmul_rn(__fmul_rn(__fsub_rn(1.0f, k.beta1), gt), gt));
        pn = __fsub_rn(pv[j], __fmul_rn(update_scale, __fdiv_rn(__fmul_rn(k.lr, gt), __fadd_rn(__builtin_sqrtf(s1[j]), k.eps))));
      } else {   // ADAGRAD
        s1[j] = __fadd_rn(s1[j], __fmul_rn(gt, gt));
        pn = __fsub_rn(pv[j], __fdiv_rn(__fmul_rn(k.lr, gt), __fadd_rn(__builtin_sqrtf(s1[j]), k.eps)));
      }
    }
    po[j] = Io<T>::from_f32(pn);
  }
  store8(p, i0, n, po);
  store8(state1, i0, n, s1);
  if (OPT == ADAM) store8(state2, i0, n, s2);
}

// ---------------------------------------------------------------- host side
static OptScalars make_scalars(float beta1, float beta2, float eps, int step, float lr, float weight_decay,
                               float gnorm_scale, bool skip_zeros) {
  OptScalars k{};
  k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.lr = lr; k.weight_decay = weight_decay;
  k.gnorm_scale = gnorm_scale; k.step = step; k.skip_zeros = skip_zeros;
  // pow(float, int) in the reference promotes to double (kernel_quant.cpp:2740-2741)
  const float correction1 = (float)(1.0 - std::pow((double)beta1, (double)step));
  const float correction2 = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
  const float neg_lr_c2 = -lr * correction2;     // fp32, as the kernel's (-lr*correction2) / correction1
  k.step_size = neg_lr_c2 / correction1;
  k.c2eps = correction2 * eps;
  const float lr_wd = lr * weight_decay;
  k.decay = 1.0f - lr_wd;
  return k;
}

// grid of the pipelined 8-bit kernels: every workgroup resident at once (CUs x occupancy, queried once
// per kernel and device), each walking its blocks with the next one's loads in flight
template <class K>
static unsigned resident_grid(K kernel, long long nb) {
  static int cached[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  int& slots = cached[dev & 63];
  if (slots == 0) {
    int cus = 0, per_cu = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, OPT_THREADS, 0);
    slots = 4 * std::max(cus, 1) * std::max(per_cu, 1);   // 4 waves of workgroups: even tails (lab: 722 vs 752 us at 1x)
  }
  return (unsigned)std::min<long long>(nb, slots);
}

template <typename T, int OPT>
void optimizer_8bit_blockwise(T* p, T* g, uint8_t* state1, uint8_t* state2, float beta1, float beta2, float eps, int step,
                              float lr, float* qmap1, float* qmap2, float* absmax1, float* absmax2, float weight_decay,
                              float gnorm_scale, bool skip_zeros, int n) {
  if (n <= 0) return;
  const OptScalars k = make_scalars(beta1, beta2, eps, step, lr, weight_decay, gnorm_scale, skip_zeros);
  const long long nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  if constexpr (OPT == ADAM) {
    const auto kern = k_optimizer_8bit_blockwise_2state<T, OPT>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(kern, nb)), dim3(OPT_THREADS), 0, current_stream(), p, g, state1,
                       state2, qmap1, qmap2, absmax1, absmax2, k, n);
  } else {
    const auto kern = k_optimizer_8bit_blockwise_1state<T, OPT>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(kern, nb)), dim3(OPT_THREADS), 0, current_stream(), p, g, state1,
                       qmap1, absmax1, k, n);
  }
  BNB_LAUNCH_CHECK("optimizer_8bit_blockwise");
}

// The fp64 slots of the reductions: one 24 KB buffer per (device, stream), allocated on first use and kept for the
// life of the process.  Three doubles per slot as three arrays of NORM_SLOTS: the sums of squares use the first, the
// global-max 8-bit step all three (sum, max1, max2).  A stream that is capturing a graph cannot allocate; it needs a
// buffer from an earlier (eager) call on that stream.
static double* norm_workspace(hipStream_t stream) {
  struct Entry { int dev; hipStream_t stream; double* ptr; };
  static std::mutex mu;
  static std::vector<Entry> entries;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  for (const Entry& e : entries)
    if (e.dev == dev && e.stream == stream) return e.ptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    set_error(1, "optimizer norm: no workspace for this stream yet and the stream is capturing a graph "
                 "(run one step on the stream before the capture)");
    return nullptr;
  }
  double* ptr = nullptr;
  if (hipMalloc(&ptr, 3 * NORM_SLOTS * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    set_error(2, "optimizer norm: workspace allocation failed");
    return nullptr;
  }
  entries.push_back({dev, stream, ptr});
  return ptr;
}

// out[first .. first + count) = (float)(sum of the KIND terms over n elements); false when nothing was written
template <typename T, int KIND>
static bool sumsq(const T* g, const float* state1, const float* state2, const NormScalars& k, int n, float* out,
                  int first, int count) {
  const hipStream_t stream = current_stream();
  double* ws = norm_workspace(stream);
  if (ws == nullptr) return false;
  const int slots = n <= 0 ? 0 : (int)std::min<long long>(((long long)n + NORM_CHUNK - 1) / NORM_CHUNK, NORM_SLOTS);
  if (slots > 0)
    hipLaunchKernelGGL((k_sumsq_partials<T, KIND>), dim3(slots), dim3(OPT_THREADS), 0, stream, g, state1, state2, k, n,
                       ws);
  hipLaunchKernelGGL(k_sumsq_finish, dim3(1), dim3(OPT_THREADS), 0, stream, ws, slots, out, first, count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error((int)e, "optimizer norm"); return false; }
  return true;
}

template <typename T>
void percentile_clipping(T* g, float* gnorm_vec, int step, int n) {
  if (gnorm_vec == nullptr) { set_error(1, "percentile_clipping: gnorm_vec is null"); return; }
  const bool all = step == 1;                      // the first step seeds every entry (kernel_quant.cpp:2691-2697)
  sumsq<T, NORM_GRAD>(g, nullptr, nullptr, NormScalars{}, n, gnorm_vec, all ? 0 : ((step % 100) + 100) % 100,
                      all ? 100 : 1);
}

template <typename T, int OPT>
void optimizer_32bit(T* g, T* p, float* state1, float* state2, float* unorm, float max_unorm, float param_norm,
                     float beta1, float beta2, float eps, float weight_decay, int step, float lr, float gnorm_scale,
                     bool skip_zeros, int n) {
  if (n <= 0) return;
  const OptScalars k = make_scalars(beta1, beta2, eps, step, lr, weight_decay, gnorm_scale, skip_zeros);
  const unsigned blocks = (unsigned)((n + OPT_THREADS * OPT_NPT - 1) / (OPT_THREADS * OPT_NPT));
  const float* unorm_in = nullptr;
  float bound = 0.0f;
  if (max_unorm > 0.0f) {
    if constexpr (OPT == LION) {
      set_error(1, "optimizer32bit: max_unorm > 0 is refused for lion (the reference's precondition sums the "
                   "unsquared state, so its update norm is a signed sum)");
      return;
    } else if constexpr (OPT == ADAGRAD) {
      set_error(1, "optimizer32bit: max_unorm > 0 is refused for adagrad (the reference's update ignores the "
                   "update scale)");
      return;
    } else {
      if (unorm == nullptr) { set_error(1, "optimizer32bit: max_unorm > 0 needs unorm (one float)"); return; }
      NormScalars ns{};
      ns.beta1 = beta1; ns.beta2 = beta2; ns.eps = eps; ns.gnorm_scale = gnorm_scale; ns.step = step;
      // 1.0f / (1.0f - pow(beta, step)) with pow(float, int) in double, rounded once (kernel_quant.cpp:1522-1523)
      ns.pc1 = (float)(1.0 / (1.0 - std::pow((double)beta1, (double)step)));
      ns.pc2 = (float)(1.0 / (1.0 - std::pow((double)beta2, (double)step)));
      const float mp = max_unorm * param_norm;
      bound = (OPT == ADAM) ? mp : mp + eps;
      if (!sumsq<T, OPT>(g, state1, state2, ns, n, unorm, 0, 1)) return;
      unorm_in = unorm;
    }
  }
  hipLaunchKernelGGL((k_optimizer_32bit<T, OPT>), dim3(blocks), dim3(OPT_THREADS), 0, current_stream(), p, g, state1,
                     state2, k, unorm_in, bound, n);
  BNB_LAUNCH_CHECK("optimizer_32bit");
}

// One step with a global maximum per state tensor: precondition, finish, update (see k_static8_precondition).
template <typename T, int OPT>
void optimizer_8bit_static(T* p, T* g, uint8_t* state1, uint8_t* state2, float* unorm, float max_unorm, float param_norm,
                           float beta1, float beta2, float eps, int step, float lr, float* qmap1, float* qmap2,
                           float* max1, float* max2, float* new_max1, float* new_max2, float weight_decay,
                           float gnorm_scale, int n) {
  if (n <= 0) return;
  if (max1 == nullptr || new_max1 == nullptr || qmap1 == nullptr ||
      (OPT == ADAM && (state2 == nullptr || qmap2 == nullptr || max2 == nullptr || new_max2 == nullptr))) {
    set_error(1, "optimizer_static_8bit: a map or max pointer is null");
    return;
  }
  const bool want_unorm = max_unorm > 0.0f;
  if (want_unorm) {
    if constexpr (OPT == RMSPROP || OPT == LION) {
      set_error(1, "optimizer_static_8bit: max_unorm > 0 is refused for rmsprop and lion (the reference's "
                   "precondition accumulates no update norm for them and its update would read a stale one)");
      return;
    }
    if (unorm == nullptr) { set_error(1, "optimizer_static_8bit: max_unorm > 0 needs unorm (one float)"); return; }
  }
  const OptScalars k = make_scalars(beta1, beta2, eps, step, lr, weight_decay, gnorm_scale, false);
  const hipStream_t stream = current_stream();
  double* ws = norm_workspace(stream);
  if (ws == nullptr) return;
  // 1.0f / (1.0f - pow(beta, step)), as NormScalars (kernel_quant.cpp:2142-2143)
  const float pc1 = (float)(1.0 / (1.0 - std::pow((double)beta1, (double)step)));
  const float pc2 = (float)(1.0 / (1.0 - std::pow((double)beta2, (double)step)));
  const int slots = (int)std::min<long long>(((long long)n + NORM_CHUNK - 1) / NORM_CHUNK, NORM_SLOTS);
  float* nm2 = (OPT == ADAM) ? new_max2 : nullptr;
  hipLaunchKernelGGL((k_static8_precondition<T, OPT>), dim3(slots), dim3(OPT_THREADS), 0, stream, g, p, state1, state2,
                     qmap1, qmap2, max1, max2, k, pc1, pc2, want_unorm, n, ws);
  hipLaunchKernelGGL(k_static8_finish, dim3(1), dim3(OPT_THREADS), 0, stream, ws, slots, new_max1, nm2,
                     want_unorm ? unorm : nullptr);
  const long long nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  const auto kern = k_optimizer_8bit_static<T, OPT>;
  hipLaunchKernelGGL(kern, dim3(resident_grid(kern, nb)), dim3(OPT_THREADS), 0, stream, p, g, state1, state2, qmap1,
                     qmap2, max1, max2, new_max1, nm2, want_unorm ? unorm : nullptr, max_unorm * param_norm, k, n);
  BNB_LAUNCH_CHECK("optimizer_static_8bit");
}

}  // namespace bnb

using namespace bnb;

extern "C" {

#define BNB_BLOCKWISE8(fname, OPT, gtype, gbits)                                                                   \
  void c##fname##_8bit_blockwise_grad_##gbits(gtype* p, gtype* g, unsigned char* state1, unsigned char* state2,    \
                                              float beta1, float beta2, float eps, int step, float lr,             \
                                              float* quantiles1, float* quantiles2, float* absmax1, float* absmax2, \
                                              float weight_decay, const float gnorm_scale, bool skip_zeros, int n) { \
    BNB_RANGE("c" #fname "_8bit_blockwise_grad_" #gbits);                                                         \
    optimizer_8bit_blockwise<gtype, OPT>(p, g, state1, state2, beta1, beta2, eps, step, lr, quantiles1, quantiles2, \
                                         absmax1, absmax2, weight_decay, gnorm_scale, skip_zeros, n);              \
  }
// ref:sycl/pythonInterface.cpp:271-284 (+ the dtypes it leaves out, additive)
BNB_BLOCKWISE8(adam, ADAM, float, fp32)
BNB_BLOCKWISE8(adam, ADAM, fp16_t, fp16)
BNB_BLOCKWISE8(adam, ADAM, bf16_t, bf16)
BNB_BLOCKWISE8(momentum, MOMENTUM, float, fp32)
BNB_BLOCKWISE8(momentum, MOMENTUM, fp16_t, fp16)
BNB_BLOCKWISE8(momentum, MOMENTUM, bf16_t, bf16)
BNB_BLOCKWISE8(rmsprop, RMSPROP, float, fp32)
BNB_BLOCKWISE8(rmsprop, RMSPROP, fp16_t, fp16)
BNB_BLOCKWISE8(rmsprop, RMSPROP, bf16_t, bf16)
BNB_BLOCKWISE8(adagrad, ADAGRAD, float, fp32)
BNB_BLOCKWISE8(adagrad, ADAGRAD, fp16_t, fp16)
BNB_BLOCKWISE8(adagrad, ADAGRAD, bf16_t, bf16)
BNB_BLOCKWISE8(lion, LION, float, fp32)
BNB_BLOCKWISE8(lion, LION, fp16_t, fp16)
BNB_BLOCKWISE8(lion, LION, bf16_t, bf16)

#define BNB_STATIC8(fname, OPT, gtype, gbits)                                                                      \
  void c##fname##_static_8bit_grad_##gbits(gtype* p, gtype* g, unsigned char* state1, unsigned char* state2,         \
                                           float* unorm, float max_unorm, float param_norm, float beta1, float beta2, \
                                           float eps, int step, float lr, float* quantiles1, float* quantiles2,      \
                                           float* max1, float* max2, float* new_max1, float* new_max2,               \
                                           float weight_decay, float gnorm_scale, int n) {                           \
    BNB_RANGE("c" #fname "_static_8bit_grad_" #gbits);                                                             \
    optimizer_8bit_static<gtype, OPT>(p, g, state1, state2, unorm, max_unorm, param_norm, beta1, beta2, eps, step,   \
                                      lr, quantiles1, quantiles2, max1, max2, new_max1, new_max2, weight_decay,      \
                                      gnorm_scale, n);                                                               \
  }
// ref:sycl/pythonInterface.cpp:243-262 + the bf16 siblings (additive)
BNB_STATIC8(adam, ADAM, float, 32)
BNB_STATIC8(adam, ADAM, fp16_t, 16)
BNB_STATIC8(adam, ADAM, bf16_t, bf16)
BNB_STATIC8(momentum, MOMENTUM, float, 32)
BNB_STATIC8(momentum, MOMENTUM, fp16_t, 16)
BNB_STATIC8(momentum, MOMENTUM, bf16_t, bf16)
BNB_STATIC8(rmsprop, RMSPROP, float, 32)
BNB_STATIC8(rmsprop, RMSPROP, fp16_t, 16)
BNB_STATIC8(rmsprop, RMSPROP, bf16_t, bf16)
BNB_STATIC8(lion, LION, float, 32)
BNB_STATIC8(lion, LION, fp16_t, 16)
BNB_STATIC8(lion, LION, bf16_t, bf16)

#define BNB_FUNC32(fname, OPT, gtype, gbits)                                                                    \
  void c##fname##32bit_grad_##gbits(gtype* g, gtype* p, float* state1, float* state2, float* unorm,             \
                                    float max_unorm, float param_norm, const float beta1, const float beta2,    \
                                    const float eps, const float weight_decay, const int step, const float lr,  \
                                    const float gnorm_scale, bool skip_zeros, const int n) {                    \
    BNB_RANGE("c" #fname "32bit_grad_" #gbits);                                                              \
    optimizer_32bit<gtype, OPT>(g, p, state1, state2, unorm, max_unorm, param_norm, beta1, beta2, eps,          \
                                weight_decay, step, lr, gnorm_scale, skip_zeros, n);                            \
  }
// ref:sycl/pythonInterface.cpp:230-241 (names as the reference spells them) + bf16 siblings (additive)
BNB_FUNC32(adam, ADAM, float, fp32)
BNB_FUNC32(adam, ADAM, fp16_t, fp16)
BNB_FUNC32(adam, ADAM, bf16_t, bf16)
BNB_FUNC32(momentum, MOMENTUM, float, 32)
BNB_FUNC32(momentum, MOMENTUM, fp16_t, 16)
BNB_FUNC32(momentum, MOMENTUM, bf16_t, bf16)
BNB_FUNC32(rmsprop, RMSPROP, float, 32)
BNB_FUNC32(rmsprop, RMSPROP, fp16_t, 16)
BNB_FUNC32(rmsprop, RMSPROP, bf16_t, bf16)
BNB_FUNC32(lion, LION, float, fp32)
BNB_FUNC32(lion, LION, fp16_t, fp16)
BNB_FUNC32(lion, LION, bf16_t, bf16)
BNB_FUNC32(adagrad, ADAGRAD, float, 32)
BNB_FUNC32(adagrad, ADAGRAD, fp16_t, 16)
BNB_FUNC32(adagrad, ADAGRAD, bf16_t, bf16)

#define BNB_PERCENTILE_CLIPPING(gtype, gbits)                                                        \
  void cpercentile_clipping_g##gbits(gtype* g, float* gnorm_vec, int step, const int n) {            \
    BNB_RANGE("cpercentile_clipping_g" #gbits);                                                      \
    percentile_clipping<gtype>(g, gnorm_vec, step, n);                                               \
  }
// ref:sycl/pythonInterface.cpp:284-285 + the bf16 sibling (additive)
BNB_PERCENTILE_CLIPPING(float, 32)
BNB_PERCENTILE_CLIPPING(fp16_t, 16)
BNB_PERCENTILE_CLIPPING(bf16_t, bf16)

}  // extern "C"
