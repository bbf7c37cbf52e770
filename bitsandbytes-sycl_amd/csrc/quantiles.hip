// Quantile code books and the 2-D error histogram.
//
//   cestimate_quantiles_<T>     ref:sycl/pythonInterface.cpp:194-195 -> ops estimateQuantiles, op_quant.cpp:309-347,
//                               kEstimateQuantiles, kernel_quant.cpp:1067-1157
//   chistogram_scatter_add_2d   ref:sycl/pythonInterface.cpp:286 -> kHistogramScatterAdd2D, kernel_quant.cpp:939-951
//
// The reference's port of kEstimateQuantiles has its block sort commented out, lets colliding quantile indices race
// for one LDS cell and sums with float atomics across workgroups.  This file implements the algorithm its comments and
// launch code describe, with a result that is a function of the input alone:
//
//   1. n < 4096: one block A[0:n], valid = n.  Otherwise B = n / 4096 full blocks, valid = 4096; the n % 4096
//      trailing elements are not read ("do not process half-blocks", kernel_quant.cpp:1090-1091).
//   2. a block's elements are converted exactly to fp32 and sorted ascending by IEEE totalOrder on the bits (key
//      u ^ 0xFFFFFFFF for a set sign bit, else u | 0x80000000, compared unsigned): -0.0 before +0.0, positive NaNs
//      after +inf, negative NaNs before -inf.  A short block is padded with the largest key; padding is never read
//      from memory.
//   3. idx[t] = (int)roundf((offset + t * q_interval) * (float)(valid - 1)), q_interval = (1 - 2 offset) / 255, in
//      fp32 without contraction (kernel_quant.cpp:1140-1142); every t reads its own sorted[idx[t]].
//   4. slot s (0 <= s < 1024) takes blocks s, s + 1024, ... in that order and adds (double)sorted_b[idx[t]] to one fp64
//      accumulator per t (from +0.0); workgroup s owns slot s, the grid is min(B, 1024) whatever the device.
//      k_quantile_finish adds the slots in ascending order per t (from +0.0), divides by (double)B, rounds once to
//      fp32 and overwrites code[0..255].  No atomics; code need not be zeroed.
//
// The sort: 256 threads hold the 4096 keys 16 per thread, position i = 16 * thread + register.  A bitonic network:
// strides 1..8 are compare-exchanges between a thread's own registers, strides 16..512 (lane bits) exchange through
// __shfl_xor, strides 1024 and 2048 (the wave bits: three steps of the 78) go through the 16 KB LDS image, stored
// [register][thread] so that every ds_write_b32 / ds_read_b32 of a wave covers 64 consecutive dwords (conflict-free).
// The same image serves the final gather of sorted[idx[t]].
#include "common.hpp"

#include <algorithm>
#include <mutex>
#include <vector>

namespace bnb {

constexpr int QE_THREADS = 256, QE_NPT = 16, QE_BLOCK = QE_THREADS * QE_NPT, QE_SLOTS = 1024;
constexpr uint32_t QE_PAD = 0xFFFFFFFFu;           // sorts last (the key of the largest positive NaN)

__device__ __forceinline__ uint32_t order_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// the fp32 bits of element e of a raw 16-byte load (exact conversions)
template <typename T> __device__ __forceinline__ uint32_t f32_bits_of(const uint4& raw, int e) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  if constexpr (sizeof(T) == 4) {
    return w[e];
  } else {
    const uint16_t h = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
    return __float_as_uint(Io<T>::to_f32(__builtin_bit_cast(T, h)));
  }
}

// keys of one block into registers, in any order (a sort does not care): 16-byte loads for a full block on a
// 16-byte-aligned base, else element loads, lanes on consecutive elements, bounded by `valid`
template <typename T>
__device__ __forceinline__ void load_keys(const T* __restrict__ p, int valid, bool vec, uint32_t (&k)[QE_NPT]) {
  constexpr int PER = 16 / (int)sizeof(T);         // elements per 16-byte load
  if (vec) {
    uint4 raw[QE_NPT / PER];
#pragma unroll
    for (int c = 0; c < QE_NPT / PER; ++c)
      raw[c] = *reinterpret_cast<const uint4*>(p + (size_t)(c * QE_THREADS + threadIdx.x) * PER);
#pragma unroll
    for (int c = 0; c < QE_NPT / PER; ++c)
#pragma unroll
      for (int e = 0; e < PER; ++e) k[c * PER + e] = order_key(f32_bits_of<T>(raw[c], e));
  } else {
#pragma unroll
    for (int r = 0; r < QE_NPT; ++r) {
      const int e = r * QE_THREADS + (int)threadIdx.x;
      k[r] = e < valid ? order_key(__float_as_uint(Io<T>::to_f32(p[e]))) : QE_PAD;
    }
  }
}

// compare-exchange of registers r and r | J for every r without bit J; asc: the smaller key goes to r
template <int J> __device__ __forceinline__ void cx_regs(uint32_t (&k)[QE_NPT], bool asc) {
#pragma unroll
  for (int r = 0; r < QE_NPT; ++r) {
    if (r & J) continue;
    const uint32_t lo = min(k[r], k[r | J]), hi = max(k[r], k[r | J]);
    k[r] = asc ? lo : hi;
    k[r | J] = asc ? hi : lo;
  }
}

// the first four stages (runs of 2, 4, 8, 16): all inside a thread; the direction of a run of K keys is bit K of
// the position, a register bit below 16 and the thread's lowest bit at K = 16
__device__ __forceinline__ void sort16_alternating(uint32_t (&k)[QE_NPT]) {
#pragma unroll
  for (int K = 2; K <= 8; K <<= 1) {
#pragma unroll
    for (int j = K >> 1; j >= 1; j >>= 1) {
#pragma unroll
      for (int r = 0; r < QE_NPT; ++r) {
        if (r & j) continue;
        const uint32_t lo = min(k[r], k[r | j]), hi = max(k[r], k[r | j]);
        const bool asc = (r & K) == 0;
        k[r] = asc ? lo : hi;
        k[r | j] = asc ? hi : lo;
      }
    }
  }
  const bool asc = (threadIdx.x & 1) == 0;
  cx_regs<8>(k, asc);
  cx_regs<4>(k, asc);
  cx_regs<2>(k, asc);
  cx_regs<1>(k, asc);
}

// sorts the workgroup's 4096 keys ascending; on return position i is register i % 16 of thread i / 16.
// image: QE_BLOCK dwords of LDS.  Every thread of the workgroup calls this.
__device__ __forceinline__ void sort4096(uint32_t (&k)[QE_NPT], uint32_t* image) {
  const int t = threadIdx.x;
  sort16_alternating(k);
  for (int KT = 2; KT <= QE_THREADS; KT <<= 1) {   // runs of 16 * KT keys
    const bool asc = (t & KT) == 0;                // KT = 256: every thread ascending
    for (int d = KT >> 1; d >= 1; d >>= 1) {       // partner thread t ^ d, same register
      const bool keep_min = ((t & d) == 0) == asc;
      if (d >= 64) {                               // another wave: through LDS
        __syncthreads();
#pragma unroll
        for (int r = 0; r < QE_NPT; ++r) image[r * QE_THREADS + t] = k[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < QE_NPT; ++r) {
          const uint32_t o = image[r * QE_THREADS + (t ^ d)];
          k[r] = keep_min ? min(k[r], o) : max(k[r], o);
        }
      } else {
#pragma unroll
        for (int r = 0; r < QE_NPT; ++r) {
          const uint32_t o = (uint32_t)__shfl_xor((int)k[r], d, 64);
          k[r] = keep_min ? min(k[r], o) : max(k[r], o);
        }
      }
    }
    cx_regs<8>(k, asc);
    cx_regs<4>(k, asc);
    cx_regs<2>(k, asc);
    cx_regs<1>(k, asc);
  }
}

// partials[slot * 256 + t]: the fp64 sum of sorted_b[idx[t]] over the slot's blocks
template <typename T>
__global__ void __launch_bounds__(QE_THREADS)
k_quantile_partials(const T* __restrict__ A, float offset, int valid, long long blocks, double* __restrict__ partials) {
  __shared__ uint32_t image[QE_BLOCK];
  const int t = threadIdx.x;
  // kernel_quant.cpp:1140-1142, op for op in fp32; the clamp only matters for an offset outside [0, 0.5]
  const float q_interval = __fdiv_rn(__fsub_rn(1.0f, __fmul_rn(2.0f, offset)), 255.0f);
  const float pos = __fmul_rn(__fadd_rn(offset, __fmul_rn((float)t, q_interval)), (float)(valid - 1));
  const int idx = min(max((int)roundf(pos), 0), valid - 1);
  const bool vec = valid == QE_BLOCK && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  double acc = 0.0;
  for (long long b = blockIdx.x; b < blocks; b += QE_SLOTS) {
    uint32_t k[QE_NPT];
    load_keys<T>(A + b * QE_BLOCK, valid, vec, k);
    sort4096(k, image);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < QE_NPT; ++r) image[r * QE_THREADS + t] = k[r];
    __syncthreads();
    acc += (double)key_value(image[(idx & (QE_NPT - 1)) * QE_THREADS + (idx >> 4)]);
  }
  partials[(size_t)blockIdx.x * QE_THREADS + t] = acc;
}

// code[t] = (float)((slot 0 + slot 1 + ... in that order, from +0.0) / blocks).  The chain of one t is serial, so the
// parallelism is across t: workgroup g owns the 16 entries t = 16 g + (0..15).  All 256 threads stage 256 slots x 16
// entries at a time in LDS (16 loads in flight per thread, 128-byte segments), then 16 threads add them in slot order.
// A single workgroup would pull all 2 MB of slots through one CU: 241 us at 1024 slots against 14 us this way.
constexpr int QF_ENTRIES = 16, QF_GROUPS = QE_THREADS / QF_ENTRIES, QF_TILE = 256;

__global__ void __launch_bounds__(QE_THREADS)
k_quantile_finish(const double* __restrict__ partials, int slots, double blocks, float* __restrict__ code) {
  __shared__ double tile[QF_TILE][QF_ENTRIES];
  const int e = threadIdx.x % QF_ENTRIES, p = threadIdx.x / QF_ENTRIES;
  const int t = blockIdx.x * QF_ENTRIES + e;
  double acc = 0.0;
  for (int s0 = 0; s0 < slots; s0 += QF_TILE) {
    const int rows = min(QF_TILE, slots - s0);
    double v[QF_TILE / QF_GROUPS];
#pragma unroll
    for (int u = 0; u < QF_TILE / QF_GROUPS; ++u) {
      const int r = u * QF_GROUPS + p;
      v[u] = r < rows ? partials[(size_t)(s0 + r) * QE_THREADS + t] : 0.0;
    }
    __syncthreads();                               // the adders are done with the previous tile
#pragma unroll
    for (int u = 0; u < QF_TILE / QF_GROUPS; ++u) tile[u * QF_GROUPS + p][e] = v[u];
    __syncthreads();
    if (p == 0)
      for (int r = 0; r < rows; ++r) acc += tile[r][e];
  }
  if (p == 0) code[t] = (float)(acc / blocks);
}

// kernel_quant.cpp:939-951; the hardware fp32 atomic add, so bins that take non-representable partial sums depend on
// the arrival order, as the reference's do
__global__ void __launch_bounds__(256)
k_histogram_scatter_add_2d(float* __restrict__ histogram, const int* __restrict__ index1,
                           const int* __restrict__ index2, const float* __restrict__ src, int maxidx1, int n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    unsafeAtomicAdd(&histogram[(long long)index1[i] * maxidx1 + index2[i]], src[i]);
}

// The fp64 slots of the quantile mean: QE_SLOTS x 256 doubles (2 MB) per (device, stream), allocated on first use and
// kept for the life of the process, as the optimizer norms keep theirs (norm_workspace, optim.hip).  A stream that is
// capturing a graph cannot allocate; it needs a buffer from an earlier (eager) call on that stream.
static double* quantile_workspace(hipStream_t stream) {
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
    set_error(1, "estimate_quantiles: no workspace for this stream yet and the stream is capturing a graph "
                 "(run one call on the stream before the capture)");
    return nullptr;
  }
  double* ptr = nullptr;
  if (hipMalloc(&ptr, (size_t)QE_SLOTS * QE_THREADS * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    set_error(2, "estimate_quantiles: workspace allocation failed");
    return nullptr;
  }
  entries.push_back({dev, stream, ptr});
  return ptr;
}

template <typename T> void estimate_quantiles(const T* A, float* code, float offset, int n) {
  if (n < 1) return;
  if (A == nullptr || code == nullptr) { set_error(1, "estimate_quantiles: A or code is null"); return; }
  const hipStream_t stream = current_stream();
  double* ws = quantile_workspace(stream);
  if (ws == nullptr) return;
  const int valid = std::min(n, QE_BLOCK);
  const long long blocks = n < QE_BLOCK ? 1 : n / QE_BLOCK;
  const int slots = (int)std::min<long long>(blocks, QE_SLOTS);
  hipLaunchKernelGGL(k_quantile_partials<T>, dim3(slots), dim3(QE_THREADS), 0, stream, A, offset, valid, blocks, ws);
  hipLaunchKernelGGL(k_quantile_finish, dim3(QE_THREADS / QF_ENTRIES), dim3(QE_THREADS), 0, stream, ws, slots,
                     (double)blocks, code);
  BNB_LAUNCH_CHECK("estimate_quantiles");
}

}  // namespace bnb

using namespace bnb;

extern "C" {

void cestimate_quantiles_fp32(float* A, float* code, float offset, int n) {
  BNB_RANGE("cestimate_quantiles_fp32");
  estimate_quantiles<float>(A, code, offset, n);
}

void cestimate_quantiles_fp16(fp16_t* A, float* code, float offset, int n) {
  BNB_RANGE("cestimate_quantiles_fp16");
  estimate_quantiles<fp16_t>(A, code, offset, n);
}

// [additive] bf16 sibling
void cestimate_quantiles_bf16(bf16_t* A, float* code, float offset, int n) {
  BNB_RANGE("cestimate_quantiles_bf16");
  estimate_quantiles<bf16_t>(A, code, offset, n);
}

void chistogram_scatter_add_2d(float* histogram, int* index1, int* index2, float* src, int maxidx1, int n) {
  BNB_RANGE("chistogram_scatter_add_2d");
  if (n <= 0) return;
  const unsigned grid = (unsigned)std::min<long long>(((long long)n + 255) / 256, 2048);
  hipLaunchKernelGGL(k_histogram_scatter_add_2d, dim3(grid), dim3(256), 0, current_stream(), histogram, index1, index2,
                     src, maxidx1, n);
  BNB_LAUNCH_CHECK("histogram_scatter_add_2d");
}

}  // extern "C"
