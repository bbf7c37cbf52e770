// LLM.int8 decode with a threshold: the one-launch inference forward of igemv8.hip (k_igemv8<MT, true>) that also
// finds the outlier columns of the activations and carries their product in fp32 (gfx950).  No COO, no column list on
// the host, no synchronisation, no workspace.
//
//   S          = { c : some row r < M has |A[r, c]| >= thr }
//   rowStat[r] = max_c (|A[r, c]| >= thr ? 0 : |A[r, c]|), -50000 when nothing compares >= 0   (k_colrow_stats<true>)
//   q[r, c]    = c in S ? 0 : rint_i8(A[r, c] * (127 / rowStat[r]))     -- the whole column leaves the int8 product
//   acc[r, j]  = sum_c q[r, c] * B[j, c]                                                        (int32, exact)
//   S empty:     out[r, j] = mm_dequant_value(acc, rowStat[r], colStats[j], bias[j])  -- the bits of k_igemv8<MT, true>
//   otherwise:   side[r, j] = sum_{c in S, ascending} float(A[r, c]) * float(B[j, c])      (fp32, every product exact)
//                out[r, j]  = fp16((v + bias[j]) + side[r, j] * (colStats[j] / 127)),  v = mm_dequant_value's product
// One rounding to fp16; the order of every sum is fixed, so equal inputs give equal bits.
//
// Workgroup shape, stream, double buffering, the LDS meeting of the eight partial tiles and the early epilogue fetches
// are k_igemv8's.  What is added:
//   * a bitmask of the outlier columns in LDS (K <= 65536: 8 KiB), zeroed before the pre-pass.  The pre-pass reads all
//     of A for the row maxima anyway; a 16-B vector that holds an outlier ORs its 8 bits in (integer LDS atomic: order
//     free, and rare).  The pre-pass's barriers publish the mask; between them the set bits are counted.
//     The mask is kept as 16-bit groups (one per 16-column chunk) with the two low 2-bit fields of the group index
//     swapped (gvo_group): the four chunks j = 0..3 of a lane's step (columns 256 s + 64 j + 16 g) then lie side by
//     side, one 8-byte LDS read per step.
//   * consume() clears the bytes of the quantised dwords whose mask bits are set (a branch lanes rarely take).
//   * after the partial tiles met, and only when S is not empty, the epilogue waves walk the mask: 64 words per ballot,
//     and for every non-zero word the thread loads its token's 32 activations and its weight row's 32 bytes (16-B
//     loads through the bounds-checked resources, four words' loads in flight together) and adds the set columns in
//     ascending order.  Any number of outlier columns is right; the walk costs one load round per four non-zero words.
#include "igemv8_common.hpp"

#include <cmath>

namespace bnb {

constexpr int GVO_MAX_K = 65536;              // the mask is static LDS
constexpr int GVO_WORDS = GVO_MAX_K / 32;

// where the mask keeps the 16 bits of the 16-column chunk q (an index of 16-bit groups): chunk 16 s + 4 j + g of step
// s sits at 16 s + 4 g + j.  Its own inverse
__device__ __forceinline__ int gvo_group(int q) { return (q & ~15) | ((q & 3) << 2) | ((q >> 2) & 3); }

template <int MT>
__global__ void __launch_bounds__(GV_THREADS)
k_igemv8_outl(int M, int N, int K, const fp16_t* __restrict__ A, int lda, const int8_t* __restrict__ B, int ldb,
              fp16_t* __restrict__ out, int ldc, float* __restrict__ rowStats_out, int* __restrict__ outlier_cols_out,
              const float* __restrict__ colStats, const fp16_t* __restrict__ bias, float thr) {
  __shared__ uint32_t s_part[GV_WAVES][MT][4][64];
  __shared__ float s_stat[GV_MAX_M];
  __shared__ float s_wmax[GV_WAVES][GV_MAX_M];
  __shared__ uint32_t s_mask[GVO_WORDS];      // bit c: column c holds an outlier
  __shared__ int s_count;                     // |S|

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int r0 = blockIdx.x * GV_ROWS;
  const int nrows = min(GV_ROWS, N - r0);
  const int nsteps = (K + GV_STEP - 1) / GV_STEP;
  const int s0 = wave * nsteps / GV_WAVES, s1 = (wave + 1) * nsteps / GV_WAVES;   // this wave's steps (may be none)
  const int kend = min(s1 * GV_STEP, K);

  // weight rows r0 .. r0 + nrows - 1 and activation rows 0 .. M - 1 as raw buffers (the host checks that both fit
  // below 2^31 bytes); a lane whose row does not exist carries GV_OOB as its row offset
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<int8_t*>(B) + (long long)r0 * ldb, (short)0, (int)((long long)(nrows - 1) * ldb + K), 0x00020000);
  const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<fp16_t*>(A), (short)0, (int)(((long long)(M - 1) * lda + K) * 2), 0x00020000);
  const uint32_t wrow = n < nrows ? (uint32_t)(n * ldb) : GV_OOB;
  uint32_t arow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int t = 16 * mt + n;
    arow[mt] = t < M ? (uint32_t)(t * lda * 2) : GV_OOB;
  }

  struct Frag {
    uint4 w[4];
    uint4 a[4][MT][2];
  };
  auto issue = [&](Frag& F, int s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = s * GV_STEP + 64 * j + 16 * g;
      const bool in = k < kend;                         // K % 16 == 0: a chunk is wholly inside or outside
      F.w[j] = gv_load16_nt(wr, in ? wrow + (uint32_t)k : GV_OOB);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int h = 0; h < 2; ++h) F.a[j][mt][h] = gv_load16(ar, in ? arow[mt] + (uint32_t)(k * 2 + 16 * h) : GV_OOB);
    }
  };
  gv_i32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = gv_i32x4_t{0, 0, 0, 0};
  float rsc[MT];
  // (s: the step F holds.  A step past the wave's share has zero activations whatever bits it is given, so its index
  // is only kept inside the mask)
  auto consume = [&](const Frag& F, int s) {
    const uint2 mk2 = reinterpret_cast<const uint2*>(s_mask)[min(s, nsteps - 1) * 4 + g];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const gv_i32x4_t b = __builtin_bit_cast(gv_i32x4_t, F.w[j]);
      const uint32_t mk = ((j >> 1 ? mk2.y : mk2.x) >> (16 * (j & 1))) & 0xffffu;   // the 16 bits of chunk j
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const uint4 lo = F.a[j][mt][0], hi = F.a[j][mt][1];
        uint4 a = make_uint4(gv_quant4(lo.x, lo.y, rsc[mt]), gv_quant4(lo.z, lo.w, rsc[mt]),
                             gv_quant4(hi.x, hi.y, rsc[mt]), gv_quant4(hi.z, hi.w, rsc[mt]));
        if (mk != 0) {                                  // rare: nibble d of the mask clears bytes of dword d
          a.x &= ~(((mk & 15u) * 0x00204081u & 0x01010101u) * 0xffu);
          a.y &= ~((((mk >> 4) & 15u) * 0x00204081u & 0x01010101u) * 0xffu);
          a.z &= ~((((mk >> 8) & 15u) * 0x00204081u & 0x01010101u) * 0xffu);
          a.w &= ~(((mk >> 12) * 0x00204081u & 0x01010101u) * 0xffu);
        }
        acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(gv_i32x4_t, a), b, acc[mt], 0, 0, 0);
      }
    }
  };

  Frag f0, f1;
  issue(f0, s0);                                        // the stream starts before everything else

  // the epilogue's operands, fetched now (k_igemv8): thread tid finishes accumulator register r of lane l of tile mt,
  // i.e. token 16 mt + 4 (l >> 4) + r and weight row l & 15
  const int e_mt = tid >> 8, e_r = (tid >> 6) & 3;
  const int e_token = 16 * e_mt + 4 * (lane >> 4) + e_r, e_col = r0 + (lane & 15);
  const bool e_live = tid < MT * 256 && e_token < M && e_col < N;
  const __amdgpu_buffer_rsrc_t csr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(colStats), (short)0, N * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t bsr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<fp16_t*>(bias), (short)0, bias != nullptr ? N * 2 : 0, 0x00020000);
  const uint32_t e_cs_bits = __builtin_amdgcn_raw_buffer_load_b32(csr, e_live ? e_col * 4 : (int)GV_OOB, 0, 0);
  const uint16_t e_bias_bits = __builtin_amdgcn_raw_buffer_load_b16(bsr, e_live ? e_col * 2 : (int)GV_OOB, 0, 0);
  __builtin_amdgcn_sched_barrier(0);

  for (int i = tid; i < GVO_WORDS; i += GV_THREADS) s_mask[i] = 0;
  if (tid == 0) s_count = 0;
  __syncthreads();

  {
    // row maxima below the threshold and the outlier columns: wave w takes its eighth of every row's 16-B vectors, the
    // eight partial maxima meet in LDS; rows >= M get a harmless 1 (their activations are zeros)
    const int nvec = K >> 3;
    const int c0 = wave * nvec / GV_WAVES, c1 = (wave + 1) * nvec / GV_WAVES;
    const int thr_bits = (int)__float_as_uint(thr);     // the host passes a finite thr > 0
#pragma unroll 1
    for (int rb = 0; rb < M; rb += 4) {                 // four rows at a time: their loads are independent
      const uint4* src[4];
      float m[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        src[i] = reinterpret_cast<const uint4*>(A + (long long)min(rb + i, M - 1) * lda);
        m[i] = -3.402823466e+38f;
      }
#pragma unroll 1
      for (int c = c0 + lane; c < c1; c += 64) {
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = src[i][c];
        uint32_t ob = 0;                                // bit j: column 8 c + j holds an outlier in one of the rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float a = fabsf((float)__builtin_bit_cast(fp16_t, (uint16_t)(w[j >> 1] >> (16 * (j & 1)))));
            // a >= thr on the bits (a's sign is clear, thr > 0: the floats order as their bits do, and a NaN lies
            // above infinity's): keep is all ones for an ordinary value or a NaN, zero for an outlier.  Written
            // without a compare, whose 32 lane masks would not fit the scalar registers
            const int ab = (int)__float_as_uint(a);
            const int keep = ((ab - thr_bits) | (0x7f800000 - ab)) >> 31;
            ob |= (uint32_t)(keep + 1) << j;
            m[i] = fmaxf(m[i], __uint_as_float((uint32_t)(ab & keep)));
          }
          // finish this row's maximum here: left to itself the compiler keeps all 32 elements' values alive across
          // the atomic's branch, and the registers cost the second resident workgroup
          m[i] = opaque(m[i]);
        }
        if (ob != 0) {                                  // byte c & 1 of the 16-bit group of chunk c >> 1
          const int byte = 2 * gvo_group(c >> 1) + (c & 1);
          atomicOr(&s_mask[byte >> 2], ob << (8 * (byte & 3)));
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        m[i] = wave_max_xor(m[i], 64);
        if (lane == 0 && rb + i < M) s_wmax[wave][rb + i] = m[i];
      }
    }
    __syncthreads();
    if (tid < GV_MAX_M) {
      float m = 1.0f;
      if (tid < M) {
        m = s_wmax[0][tid];
#pragma unroll
        for (int w = 1; w < GV_WAVES; ++w) m = fmaxf(m, s_wmax[w][tid]);
        if (!(m >= 0.0f)) m = -50000.0f;
      }
      s_stat[tid] = m;
    }
    {
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < GVO_WORDS / GV_THREADS; ++i) cnt += __popc(s_mask[tid + i * GV_THREADS]);
      if (cnt != 0) atomicAdd(&s_count, cnt);
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) rsc[mt] = __fdiv_rn(127.0f, s_stat[16 * mt + n]);
    if (blockIdx.x == 0) {
      if (rowStats_out != nullptr && tid < M) rowStats_out[tid] = s_stat[tid];
      if (outlier_cols_out != nullptr && tid == 0) outlier_cols_out[0] = s_count;
    }
  }
  const int n_outl = __builtin_amdgcn_readfirstlane(s_count);

#pragma unroll 1
  for (int s = s0; s < s1; s += 2) {
    // the next buffer's loads leave before this buffer's MFMAs wait; steps past s1 are issued all the same, with
    // out-of-range offsets (zeros, no memory access), so that every path has the same count of loads in flight
    issue(f1, s + 1);
    __builtin_amdgcn_sched_barrier(0);
    consume(f0, s);
    issue(f0, s + 2);
    __builtin_amdgcn_sched_barrier(0);
    consume(f1, s + 1);
  }

  // the eight partial tiles meet in LDS: accumulator register r of lane l is token 4 (l >> 4) + r, weight row l & 15
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[wave][mt][r][lane] = (uint32_t)acc[mt][r];
  __syncthreads();
  if (wave >= MT * 4) return;                           // the epilogue's waves (wave-uniform)

  // the outlier columns' product of this thread's (token, weight row), in ascending column order
  float side = 0.0f;
  if (n_outl != 0) {
    const uint32_t e_arow = e_live ? (uint32_t)(e_token * lda * 2) : GV_OOB;
    const uint32_t e_wrow = e_live ? (uint32_t)((lane & 15) * ldb) : GV_OOB;
    struct Seg {
      uint4 a[4];                                       // 32 activations of the token
      uint4 b[2];                                       // 32 weight bytes of the row
    };
    // columns 32 wi .. 32 wi + 31 (wi < 0: nothing); a 16-column half beyond K is not read
    auto load_seg = [&](Seg& sg, int wi) {
      const int c = 32 * wi;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool in = wi >= 0 && c + 16 * h < K;
        sg.b[h] = gv_load16(wr, in ? e_wrow + (uint32_t)(c + 16 * h) : GV_OOB);
        sg.a[2 * h] = gv_load16(ar, in ? e_arow + (uint32_t)(2 * c + 32 * h) : GV_OOB);
        sg.a[2 * h + 1] = gv_load16(ar, in ? e_arow + (uint32_t)(2 * c + 32 * h + 16) : GV_OOB);
      }
    };
    const int nwords = (K + 31) >> 5;
#pragma unroll 1
    for (int base = 0; base < nwords; base += 64) {
      // lane l: the 32 columns from 32 (base + l), i.e. chunks 2 (base + l) and the next, in ascending bit order
      const uint16_t* mask16 = reinterpret_cast<const uint16_t*>(s_mask);
      const int q = 2 * min(base + lane, nwords - 1);
      const uint32_t mw = base + lane < nwords
                              ? (uint32_t)mask16[gvo_group(q)] | ((uint32_t)mask16[gvo_group(q + 1)] << 16) : 0u;
      unsigned long long nz = __ballot(mw != 0);        // the non-zero words of this group: the same in every wave
      // four non-zero words a round: their 24 loads leave together (the stream's registers are free by now)
#pragma unroll 1
      while (nz != 0) {
        int wi[4];
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool has = nz != 0;
          const int i = has ? (int)__builtin_ctzll(nz) : 0;
          w[u] = has ? __builtin_amdgcn_readlane(mw, i) : 0u;
          wi[u] = has ? base + i : -1;
          nz &= nz - 1;
        }
        Seg sg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) load_seg(sg[u], wi[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (w[u] == 0) continue;                      // wave-uniform, as is every test of a bit below
          const Seg& c = sg[u];
          const uint32_t aw[16] = {c.a[0].x, c.a[0].y, c.a[0].z, c.a[0].w, c.a[1].x, c.a[1].y, c.a[1].z, c.a[1].w,
                                   c.a[2].x, c.a[2].y, c.a[2].z, c.a[2].w, c.a[3].x, c.a[3].y, c.a[3].z, c.a[3].w};
          const uint32_t bw[8] = {c.b[0].x, c.b[0].y, c.b[0].z, c.b[0].w, c.b[1].x, c.b[1].y, c.b[1].z, c.b[1].w};
#pragma unroll
          for (int b = 0; b < 32; ++b) {
            if ((w[u] >> b) & 1u) {
              const float av = (float)__builtin_bit_cast(fp16_t, (uint16_t)(aw[b >> 1] >> (16 * (b & 1))));
              const float bv = (float)(int8_t)(uint8_t)(bw[b >> 2] >> (8 * (b & 3)));
              side = __fadd_rn(side, __fmul_rn(av, bv));
            }
          }
        }
      }
    }
  }

  if (e_live) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < GV_WAVES; ++w) sum += s_part[w][e_mt][e_r][lane];
    const float rs = s_stat[e_token], cs = __uint_as_float(e_cs_bits);
    const float bv = (float)__builtin_bit_cast(fp16_t, e_bias_bits);
    fp16_t o;
    if (n_outl == 0) {
      o = mm_dequant_value((int32_t)sum, rs, cs, bv);
    } else {
      float v = __fmul_rn((float)(int32_t)sum, 6.200012e-05f);
      v = __fmul_rn(v, rs);
      v = opaque(__fmul_rn(v, cs));
      v = opaque(__fadd_rn(v, bv));
      const float t = opaque(__fmul_rn(side, __fdiv_rn(cs, 127.0f)));
      o = Io<fp16_t>::from_f32(__fadd_rn(v, t));
    }
    out[(long long)e_token * ldc + e_col] = o;
  }
}

}  // namespace bnb

extern "C" {

// [additive] cint8_linear_rows_fp16 with an outlier threshold (> 0, finite): the columns of A holding a value with
// |a| >= threshold leave the int8 product and their fp16 x int8 product is added in fp32 inside the same launch.
// rowStats_out (m floats) and outlier_cols_out (one int, the number of outlier columns) may be NULL.
// 0 = launched (or nothing to do), 1 = launch error, 2 = not covered or cigemv_set_mode(-1): nothing launched
int cint8_linear_rows_outlier_fp16(int m, int n, int k, const fp16_t* A, const int8_t* B, fp16_t* out,
                                   float* rowStats_out, int* outlier_cols_out, const float* colStats,
                                   const fp16_t* bias, float threshold, int lda, int ldb, int ldc) {
  using namespace bnb;
  BNB_RANGE("cint8_linear_rows_outlier_fp16");
  if (igemv_mode() < 0) return 2;
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  if (!igemv8_covers(m, k, A, B, lda, ldb, ldc, n, 2) || k > GVO_MAX_K) return 2;
  if (!std::isfinite(threshold) || !(threshold > 0.0f)) return 2;
  const dim3 grid((unsigned)((n + GV_ROWS - 1) / GV_ROWS)), block(GV_THREADS);
  if (m <= 16)
    hipLaunchKernelGGL((k_igemv8_outl<1>), grid, block, 0, current_stream(), m, n, k, A, lda, B, ldb, out, ldc,
                       rowStats_out, outlier_cols_out, colStats, bias, threshold);
  else
    hipLaunchKernelGGL((k_igemv8_outl<2>), grid, block, 0, current_stream(), m, n, k, A, lda, B, ldb, out, ldc,
                       rowStats_out, outlier_cols_out, colStats, bias, threshold);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error((int)e, "int8_linear_rows_outlier launch"); return 1; }
  return 0;
}

}  // extern "C"
