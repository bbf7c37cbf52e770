// LLM.int8 prefill with a threshold and no host round trip (gfx950): the launches around the unchanged int8 GEMM that
// find the outlier columns of the activations on the device.  No COO, no unique, no value read back, no allocation.
//
//   S           = { c : some row r has |A[r, c]| >= thr }                            (fp32 compare, equal is an outlier)
//   rowStats[r] = max_c (|A[r, c]| >= thr ? 0 : |A[r, c]|), -50000 when nothing compares >= 0   (k_colrow_stats<true>)
//   CA[r, c]    = c in S ? 0 : rint_i8(A[r, c] * (127 / rowStats[r]))                  (k_double_rowcol_quant's row half)
//   first       = igemmlt_dequant(CA, CB, rowStats, SCB, bias)                            (the caller's routed GEMM, fp16)
//   out[r, j]   = fp16(float(first[r, j]) + (SCB[j] / 127) * sum_{c in S, ascending} float(A[r, c]) * float(CB[j, c]))
// Every product is exact in fp32 and the sum is sequential in ascending column order, so the result does not depend on
// the grid: equal inputs give equal bits.  No float atomics.
//
// Workspace (caller's, cint8_outlier_workspace_bytes(k)): int count | 12 bytes unused | one bit per column, padded to
// 16 bytes | int idx[k].  Stream order of one forward:
//   memset node     count and the bit mask to zero (a stale mask never reaches the next call)
//   k_outl_scan     one wave per row: the row maximum without the outliers; a 16-B vector that holds an outlier ORs
//                   its 8 bits into the mask (integer atomic: order-free, and rare)
//   k_outl_quant    one wave per row: CA with the marked columns zero; workgroup 0 instead turns the complete mask into
//                   the ascending list idx[] and count by a prefix popcount (never an atomic counter: the order defines
//                   the sum)
//   (the int8 GEMM with the fused dequant)
//   k_outlier_side  256 x 128 tiles of out in four 64-row sub-tiles; reads count first and returns when it is 0; walks
//                   the list in chunks of 64, each chunk's activations (fp16) and weight bytes gathered into LDS,
//                   accumulates in ascending order across the chunks, then one read-modify-write of out
#include "int8_common.hpp"

#include <cmath>

namespace bnb {

constexpr int OP_HEAD = 16;                   // bytes in front of the mask: count and padding
constexpr int OP_TM = 64, OP_TN = 128;        // the side kernel's sub-tile of out
constexpr int OP_SUB = 4;                     // sub-tiles (of rows) per workgroup
constexpr int OP_CHUNK = 64;                  // list entries staged per round

__host__ __device__ __forceinline__ long long op_mask_bytes(int k) { return pad_to(((long long)k + 31) / 32 * 4, 16); }
__host__ __device__ __forceinline__ long long op_ws_bytes(int k) { return OP_HEAD + op_mask_bytes(k) + 4ll * k; }

__device__ __forceinline__ float op_half(uint32_t w, int j) {
  return (float)__builtin_bit_cast(fp16_t, (uint16_t)(w >> (16 * j)));
}

// ---------------------------------------------------------------------------------------------- pass 1: scan
__global__ void __launch_bounds__(256)
k_outl_scan(const fp16_t* __restrict__ A, float* __restrict__ rowStats, uint32_t* __restrict__ mask, int rows, int cols,
            float thr) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = cols >> 3;
  const uint4* src = reinterpret_cast<const uint4*>(A + (long long)row * cols);
  float m = -3.402823466e+38f;
#pragma unroll 1
  for (int c0 = lane; c0 < nvec; c0 += 256) {           // four independent 16-B loads per lane and round
    uint4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 64 * i;
      v[i] = c < nvec ? src[c] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 64 * i;
      if (c >= nvec) continue;                          // (a padding zero would turn an all-NaN row's -50000 into 0)
      const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
      uint32_t ob = 0;                                  // bit j: column 8 c + j holds an outlier in this row
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = fabsf(op_half(w[j >> 1], j & 1));
        const bool o = a >= thr;                        // false for a NaN, which fmaxf then ignores
        ob |= (uint32_t)o << j;
        m = fmaxf(m, o ? 0.0f : a);
      }
      if (ob != 0) atomicOr(&mask[c >> 2], ob << (8 * (c & 3)));
    }
  }
  m = wave_max_xor(m, 64);
  if (!(m >= 0.0f)) m = -50000.0f;                      // cget_col_row_stats' pre-fill, untouched by its atomicMax
  if (lane == 0) rowStats[row] = m;
}

// ---------------------------------------------------------------------------------------------- pass 2: quantise + list
__global__ void __launch_bounds__(256)
k_outl_quant(const fp16_t* __restrict__ A, const float* __restrict__ rowStats, int8_t* __restrict__ CA,
             const uint32_t* __restrict__ mask, int* __restrict__ count, int* __restrict__ idx, int rows, int cols) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0) {
    // the ascending column list from the complete mask: 256 words a round, a prefix popcount places every word's bits
    const int nwords = (cols + 31) >> 5;
    int running = 0;
#pragma unroll 1
    for (int w0 = 0; w0 < nwords; w0 += 256) {
      const int w = w0 + tid;
      uint32_t bits = w < nwords ? mask[w] : 0u;
      const int cnt = __popc(bits);
      int inc = cnt;                                    // inclusive scan over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) s_wave[wave] = inc;
      __syncthreads();
      int before = running, total = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = s_wave[i];
        if (i < wave) before += s;
        total += s;
      }
      int pos = before + inc - cnt;
      while (bits != 0) {
        const int c = 32 * w + __builtin_ctz(bits);
        if (pos < cols && c < cols) idx[pos] = c;       // always true for a mask pass 1 wrote; keeps the store inside
        ++pos;
        bits &= bits - 1;
      }
      running += total;
      __syncthreads();
    }
    if (tid == 0) count[0] = min(running, cols);
    return;
  }
  const int row = (blockIdx.x - 1) * 4 + wave;
  if (row >= rows) return;
  const int nvec = cols >> 3;
  const uint4* src = reinterpret_cast<const uint4*>(A + (long long)row * cols);
  uint2* dst = reinterpret_cast<uint2*>(CA + (long long)row * cols);
  const uint8_t* mbytes = reinterpret_cast<const uint8_t*>(mask);   // byte c: the 8 columns of vector c
  const float rsc = __fdiv_rn(127.0f, rowStats[row]);
#pragma unroll 1
  for (int c0 = lane; c0 < nvec; c0 += 256) {
    uint4 v[4];
    uint32_t mk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 64 * i;
      const bool in = c < nvec;
      v[i] = in ? src[c] : make_uint4(0, 0, 0, 0);
      mk[i] = in ? (uint32_t)mbytes[c] : 0u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 64 * i;
      if (c >= nvec) continue;
      const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
      uint32_t q[2] = {0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int8_t r8 = rint_i8(__fmul_rn(op_half(w[j >> 1], j & 1), rsc));
        q[j >> 2] |= (uint32_t)(uint8_t)r8 << (8 * (j & 3));
      }
      if (mk[i] != 0) {                                 // rare: bit j of the mask byte clears byte j
        q[0] &= ~(((mk[i] & 15u) * 0x00204081u & 0x01010101u) * 0xffu);
        q[1] &= ~(((mk[i] >> 4) * 0x00204081u & 0x01010101u) * 0xffu);
      }
      dst[c] = make_uint2(q[0], q[1]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- the side product
// A workgroup owns OP_SUB row sub-tiles of 64 x 128 under one another.  Thread (ty, tx) of the 16 x 16 workgroup owns
// rows 4 ty .. 4 ty + 3 and columns 8 tx .. 8 tx + 7 of a sub-tile: one 16-B read-modify-write per row where out
// allows it (VEC), element by element otherwise.  The gathers are what the kernel costs beyond the read-modify-write
// (a 64-B sector per gathered element), so a list that fits one chunk -- the usual case -- stages its weight bytes
// once for all the sub-tiles; a longer list stages them again for every sub-tile.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_outlier_side(int M, int N, int K, const fp16_t* __restrict__ A, const int8_t* __restrict__ B,
               const float* __restrict__ colStats, fp16_t* __restrict__ out, int ldc, const int* __restrict__ count,
               const int* __restrict__ idx, int tiles_n) {
  __shared__ int s_idx[OP_CHUNK];
  __shared__ __attribute__((aligned(16))) uint16_t s_a[OP_CHUNK][OP_TM];     // [list entry][row of the tile], fp16 bits
  __shared__ __attribute__((aligned(16))) int8_t s_b[OP_CHUNK][OP_TN];       // [list entry][column of the tile]
  const int n_outl = min(count[0], K);
  if (n_outl <= 0) return;                              // uniform over the grid: nothing is written
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int rb = (int)(blockIdx.x / tiles_n) * (OP_TM * OP_SUB), c0 = (int)(blockIdx.x % tiles_n) * OP_TN;
  const int col = c0 + 8 * tx;
  const bool one_chunk = n_outl <= OP_CHUNK;
  float sc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) sc[c] = col + c < N ? __fdiv_rn(colStats[col + c], 127.0f) : 0.0f;

#pragma unroll 1
  for (int sub = 0; sub < OP_SUB; ++sub) {
    const int r0 = rb + sub * OP_TM;
    if (r0 >= M) break;                                 // uniform over the workgroup
    const int row = r0 + 4 * ty;

    // first's values of this thread, fetched before the walk
    uint4 first[4];
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        first[i] = (row + i < M && col < N) ? *reinterpret_cast<const uint4*>(out + (long long)(row + i) * ldc + col)
                                            : make_uint4(0, 0, 0, 0);
    }

    float side[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) side[i][j] = 0.0f;

#pragma unroll 1
    for (int base = 0; base < n_outl; base += OP_CHUNK) {
      const int len = min(OP_CHUNK, n_outl - base);
      const bool stage_b = !(one_chunk && sub > 0);     // one chunk: s_idx and s_b stay as the first sub-tile left them
      __syncthreads();                                  // the previous chunk has been read
      if (stage_b) {
        if (tid < len) s_idx[tid] = min(max(idx[base + tid], 0), K - 1);   // inside A and B whatever the list holds
        __syncthreads();
      }
      for (int e = tid; e < OP_TM * len; e += 256) {
        const int r = e / len, j = e - r * len;
        s_a[j][r] = r0 + r < M ? __builtin_bit_cast(uint16_t, A[(long long)(r0 + r) * K + s_idx[j]]) : (uint16_t)0;
      }
      if (stage_b) {
        for (int e = tid; e < OP_TN * len; e += 256) {
          const int n = e / len, j = e - n * len;
          s_b[j][n] = c0 + n < N ? B[(long long)(c0 + n) * K + s_idx[j]] : (int8_t)0;
        }
      }
      __syncthreads();
#pragma unroll 2
      for (int j = 0; j < len; ++j) {
        const uint2 a2 = *reinterpret_cast<const uint2*>(&s_a[j][4 * ty]);
        const uint2 b2 = *reinterpret_cast<const uint2*>(&s_b[j][8 * tx]);
        const float av[4] = {op_half(a2.x, 0), op_half(a2.x, 1), op_half(a2.y, 0), op_half(a2.y, 1)};
        float bv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) bv[c] = (float)(int8_t)(uint8_t)((c < 4 ? b2.x : b2.y) >> (8 * (c & 3)));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 8; ++c) side[i][c] = __fadd_rn(side[i][c], __fmul_rn(av[i], bv[c]));
      }
    }

    if (col < N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (row + i >= M) break;
        fp16_t* o = out + (long long)(row + i) * ldc + col;
        if constexpr (VEC) {
          const uint32_t w[4] = {first[i].x, first[i].y, first[i].z, first[i].w};
          uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const float t = opaque(__fmul_rn(sc[c], side[i][c]));
            const fp16_t h = Io<fp16_t>::from_f32(__fadd_rn(op_half(w[c >> 1], c & 1), t));
            r[c >> 1] |= (uint32_t)__builtin_bit_cast(uint16_t, h) << (16 * (c & 1));
          }
          *reinterpret_cast<uint4*>(o) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (col + c < N) {
              const float t = opaque(__fmul_rn(sc[c], side[i][c]));
              o[c] = Io<fp16_t>::from_f32(__fadd_rn((float)o[c], t));
            }
          }
        }
      }
    }
  }
}

static bool op_covers(int k, const void* A) { return k >= 8 && k % 8 == 0 && ((uintptr_t)A & 15) == 0; }

}  // namespace bnb

using namespace bnb;

extern "C" {

// [additive] bytes of the workspace the two entries below share for activations of k columns
long long cint8_outlier_workspace_bytes(int k) { return k > 0 ? op_ws_bytes(k) : 0; }

// [additive] row statistics, CA with the outlier columns zeroed, and the outlier columns' ascending list in ws.
// 0 = launched (or nothing to do), 1 = error, 2 = not covered: nothing launched
int cint8_outlier_quant_fp16(int m, int k, const fp16_t* A, float threshold, char* CA, float* rowStats, void* ws,
                             long long ws_bytes) {
  BNB_RANGE("cint8_outlier_quant_fp16");
  if (m <= 0 || k <= 0) return 0;
  if (!op_covers(k, A) || ((uintptr_t)CA & 7) || ws == nullptr || ((uintptr_t)ws & 15) || ws_bytes < op_ws_bytes(k))
    return 2;
  if (!std::isfinite(threshold) || !(threshold > 0.0f)) return 2;
  const long long blocks = ((long long)m + 3) / 4;
  if (blocks + 1 > 0x7fffffffll) return 2;
  const long long head = OP_HEAD + op_mask_bytes(k);
  int* count = reinterpret_cast<int*>(ws);
  uint32_t* mask = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + OP_HEAD);
  int* idx = reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + head);
  hipStream_t s = current_stream();
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)head, s);
  if (e != hipSuccess) { set_error((int)e, "int8_outlier_quant memset"); return 1; }
  hipLaunchKernelGGL(k_outl_scan, dim3((unsigned)blocks), dim3(256), 0, s, A, rowStats, mask, m, k, threshold);
  hipLaunchKernelGGL(k_outl_quant, dim3((unsigned)(blocks + 1)), dim3(256), 0, s, A, rowStats, (int8_t*)CA, mask, count,
                     idx, m, k);
  e = hipGetLastError();
  if (e != hipSuccess) { set_error((int)e, "int8_outlier_quant launch"); return 1; }
  return 0;
}

// [additive] out[r, j] += (colStats[j] / 127) * sum over the listed columns of A[r, c] * B[j, c], in fp32, ascending,
// one rounding to fp16; nothing is written when the list is empty.  Same return convention
int cint8_outlier_side_fp16(int m, int n, int k, const fp16_t* A, const int8_t* B, const float* colStats, fp16_t* out,
                            int ldc, const void* ws) {
  BNB_RANGE("cint8_outlier_side_fp16");
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  if (!op_covers(k, A) || ws == nullptr || ((uintptr_t)ws & 15) || ldc < n || ((uintptr_t)out & 1)) return 2;
  const long long tiles_n = ((long long)n + OP_TN - 1) / OP_TN;
  const long long tiles_m = ((long long)m + OP_TM * OP_SUB - 1) / (OP_TM * OP_SUB);
  if (tiles_n * tiles_m > 0x7fffffffll) return 2;
  const int* count = reinterpret_cast<const int*>(ws);
  const int* idx = reinterpret_cast<const int*>(reinterpret_cast<const char*>(ws) + OP_HEAD + op_mask_bytes(k));
  const dim3 grid((unsigned)(tiles_n * tiles_m)), block(256);
  const bool vec = ldc % 8 == 0 && n % 8 == 0 && ((uintptr_t)out & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_outlier_side<true>, grid, block, 0, current_stream(), m, n, k, A, B, colStats, out, ldc, count,
                       idx, (int)tiles_n);
  else
    hipLaunchKernelGGL(k_outlier_side<false>, grid, block, 0, current_stream(), m, n, k, A, B, colStats, out, ldc, count,
                       idx, (int)tiles_n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error((int)e, "int8_outlier_side launch"); return 1; }
  return 0;
}

}  // extern "C"
