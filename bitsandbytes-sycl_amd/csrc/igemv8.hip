// LLM.int8 decode: the row-major int8 product with the mm_dequant epilogue for 1..32 activation rows, as a weight
// stream (gfx950).  One launch, no workspace, no transform: the weight B [N, K] (Int8Params' CB) is read once, in place.
//
//   out[r, c] = mm_dequant_value(sum_k A[r, k] * B[c, k], rowStats[r], colStats[c], bias[c])          (fp16)
//
// The int32 sum is exact in any order, so the result has the bits of the tile kernels behind cigemmlt_row_dequant_fp16
// (same epilogue function, int8_common.hpp), whatever the k order or split chosen here.
//
// Shape of the work: a workgroup of 8 waves owns 16 weight rows and all of K; its waves take K in eighths of whole
// 256-B steps and the eight int32 partial tiles meet in LDS (no atomics, deterministic).  A step of a wave is
// 16 rows x 256 B of weight: lane (n, g) = (l & 15, l >> 4) loads 16 B at k = 256 s + 64 j + 16 g of row n for
// j = 0..3 -- the v_mfma_i32_16x16x64_i8 fragment of k_igemm (int8.hip), four of them back to back, so that the four
// loads of a step sweep 256 contiguous bytes of each row (two whole 128-B lines), non-temporal.  The activations are
// the other MFMA operand (rows = tokens, one or two 16-row fragments), read with the same k mapping through a buffer
// resource over rows 0..M-1: lanes of rows >= M and chunks past the wave's K share get an out-of-range offset, which
// returns zeros without a memory access.  The weight goes through a buffer resource over the workgroup's rows as well,
// so rows >= N and k >= K are never read.  Activations are not assumed resident (K = 28672 x 32 rows is 0.9 MB): each
// wave reads the chunks of its own K share from L2 as it goes.
//
// FUSED: the activations arrive as fp16 and are quantised on the way into the MFMA operand with k_row_quant's
// expressions (int8.hip): every workgroup first computes the row maxima itself (max is exact in any order; the first
// weight loads are already in flight), m = max |a| or -50000 when no |a| compares >= 0, q = rint_i8(a * (127 / m)),
// and m is the row statistic of the epilogue.  Workgroup 0 writes the statistics when asked to; CA is never written.
//
// Each wave keeps two steps in flight, double buffered in registers (one buffer's loads leave before the other's
// MFMAs wait); more would cost the second resident workgroup per CU, which is what overlaps one workgroup's start and
// epilogue with another's stream.  The epilogue's statistics and bias are fetched at the start for the same reason.
#include "igemv8_common.hpp"

namespace bnb {

// The automatic route of cigemmlt_row_dequant{,_ws}_fp16 (mode 0), from tools/int8_decode_ab.py on weights rotating
// through HBM (profiles/int8_decode_ab.json): up to 8 rows this kernel beats the tile kernels at all
// four measured weights beyond the run-to-run spread; weights up to the 11008 x 4096 class (45 MB, the largest of the
// three measured to win there) win at every covered row count, while 8192 x 28672 loses from 16 rows on.
constexpr int GV_AUTO_ROWS = 8;
constexpr long long GV_SMALL_WEIGHT = 11008LL * 4096;   // N * K up to which all 32 rows are routed here

static Knob<int> g_igemv_mode{0};        // cigemv_set_mode: 0 = auto, 1 = wherever covered, -1 = never
int igemv_mode() { return g_igemv_mode; }

// MT: 16-row activation fragments (1: M <= 16, 2: M <= 32).  FUSED: Av is fp16 [M, K] (lda in elements), quantised
// here; otherwise int8 [M, K] with its statistics in rowStats.
template <int MT, bool FUSED>
__global__ void __launch_bounds__(GV_THREADS)
k_igemv8(int M, int N, int K, const void* __restrict__ Av, int lda, const int8_t* __restrict__ B, int ldb,
         fp16_t* __restrict__ out, int ldc, const float* __restrict__ rowStats, float* __restrict__ rowStats_out,
         const float* __restrict__ colStats, const fp16_t* __restrict__ bias) {
  constexpr int NS = 1;                   // steps per register buffer
  constexpr int AE = FUSED ? 2 : 1;       // bytes per activation element; 16-B loads per fragment chunk
  __shared__ uint32_t s_part[GV_WAVES][MT][4][64];
  __shared__ float s_stat[GV_MAX_M];
  __shared__ float s_wmax[FUSED ? GV_WAVES : 1][GV_MAX_M];

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
      const_cast<void*>(Av), (short)0, (int)(((long long)(M - 1) * lda + K) * AE), 0x00020000);
  const uint32_t wrow = n < nrows ? (uint32_t)(n * ldb) : GV_OOB;
  uint32_t arow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int t = 16 * mt + n;
    arow[mt] = t < M ? (uint32_t)(t * lda * AE) : GV_OOB;
  }

  struct Frag {
    uint4 w[NS][4];
    uint4 a[NS][4][MT][AE];
  };
  auto issue = [&](Frag& F, int s) {
#pragma unroll
    for (int ss = 0; ss < NS; ++ss)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = (s + ss) * GV_STEP + 64 * j + 16 * g;
        const bool in = k < kend;                       // K % 16 == 0: a chunk is wholly inside or outside
        F.w[ss][j] = gv_load16_nt(wr, in ? wrow + (uint32_t)k : GV_OOB);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int h = 0; h < AE; ++h)
            F.a[ss][j][mt][h] = gv_load16(ar, in ? arow[mt] + (uint32_t)(k * AE + 16 * h) : GV_OOB);
      }
  };

  gv_i32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = gv_i32x4_t{0, 0, 0, 0};
  float rsc[MT];
  auto consume = [&](const Frag& F) {
#pragma unroll
    for (int ss = 0; ss < NS; ++ss)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const gv_i32x4_t b = __builtin_bit_cast(gv_i32x4_t, F.w[ss][j]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          uint4 a;
          if constexpr (FUSED) {
            const uint4 lo = F.a[ss][j][mt][0], hi = F.a[ss][j][mt][AE - 1];
            a = make_uint4(gv_quant4(lo.x, lo.y, rsc[mt]), gv_quant4(lo.z, lo.w, rsc[mt]),
                           gv_quant4(hi.x, hi.y, rsc[mt]), gv_quant4(hi.z, hi.w, rsc[mt]));
          } else {
            a = F.a[ss][j][mt][0];
          }
          acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(gv_i32x4_t, a), b, acc[mt], 0, 0, 0);
        }
      }
  };

  Frag f0, f1;
  issue(f0, s0);                                        // the stream starts before everything else

  // the epilogue's operands, fetched now: thread tid finishes accumulator register r of lane l of tile mt, i.e. token
  // 16 mt + 4 (l >> 4) + r and weight row l & 15 -- their latency would otherwise follow the last barrier
  const int e_mt = tid >> 8, e_r = (tid >> 6) & 3;
  const int e_token = 16 * e_mt + 4 * (lane >> 4) + e_r, e_col = r0 + (lane & 15);
  const bool e_live = tid < MT * 256 && e_token < M && e_col < N;
  // (branch-free through buffer resources -- dead threads and a NULL bias read zeros -- and converted only in the
  // epilogue, so nothing up here waits for a load)
  const __amdgpu_buffer_rsrc_t csr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(colStats), (short)0, N * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t bsr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<fp16_t*>(bias), (short)0, bias != nullptr ? N * 2 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rowStats), (short)0, FUSED ? 0 : M * 4, 0x00020000);
  const uint32_t e_cs_bits = __builtin_amdgcn_raw_buffer_load_b32(csr, e_live ? e_col * 4 : (int)GV_OOB, 0, 0);
  const uint16_t e_bias_bits = __builtin_amdgcn_raw_buffer_load_b16(bsr, e_live ? e_col * 2 : (int)GV_OOB, 0, 0);
  const uint32_t e_rs_bits = __builtin_amdgcn_raw_buffer_load_b32(rsr, e_live ? e_token * 4 : (int)GV_OOB, 0, 0);
  __builtin_amdgcn_sched_barrier(0);

  if constexpr (FUSED) {
    // row maxima: wave w takes its eighth of every row's 16-B vectors (one row's maximum is then a few loads deep for
    // any M), the eight partial maxima meet in LDS; rows >= M get a harmless 1 (their activations are zeros)
    const fp16_t* A = reinterpret_cast<const fp16_t*>(Av);
    const int nvec = K >> 3;
    const int c0 = wave * nvec / GV_WAVES, c1 = (wave + 1) * nvec / GV_WAVES;
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
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
          for (int j = 0; j < 8; ++j)
            m[i] = fmaxf(m[i], fabsf((float)__builtin_bit_cast(fp16_t, (uint16_t)(w[j >> 1] >> (16 * (j & 1))))));
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
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) rsc[mt] = __fdiv_rn(127.0f, s_stat[16 * mt + n]);
    if (blockIdx.x == 0 && rowStats_out != nullptr && tid < M) rowStats_out[tid] = s_stat[tid];
  }

#pragma unroll 1
  for (int s = s0; s < s1; s += 2 * NS) {
    // the next buffer's loads leave before this buffer's MFMAs wait (the scheduler otherwise sinks them below).
    // Steps past s1 are issued all the same, with out-of-range offsets (zeros, no memory access): a branch around
    // them would merge paths with different counts of loads in flight, and the wait before the MFMAs would have to
    // assume the smaller one, i.e. drain the buffer just issued
    issue(f1, s + NS);
    __builtin_amdgcn_sched_barrier(0);
    consume(f0);
    issue(f0, s + 2 * NS);
    __builtin_amdgcn_sched_barrier(0);
    consume(f1);
  }

  // the eight partial tiles meet in LDS: accumulator register r of lane l is token 4 (l >> 4) + r, weight row l & 15
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[wave][mt][r][lane] = (uint32_t)acc[mt][r];
  __syncthreads();
  if (e_live) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < GV_WAVES; ++w) sum += s_part[w][e_mt][e_r][lane];
    const float rs = FUSED ? s_stat[e_token] : __uint_as_float(e_rs_bits);
    out[(long long)e_token * ldc + e_col] = mm_dequant_value(
        (int32_t)sum, rs, __uint_as_float(e_cs_bits), (float)__builtin_bit_cast(fp16_t, e_bias_bits));
  }
}

// 0 = launched (or nothing to do), 1 = launch error, 2 = not covered (nothing launched)
template <bool FUSED>
static int launch_igemv8(int m, int n, int k, const void* A, const int8_t* B, fp16_t* out, const float* rowStats,
                         float* rowStats_out, const float* colStats, const fp16_t* bias, int lda, int ldb, int ldc) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  if (!igemv8_covers(m, k, A, B, lda, ldb, ldc, n, FUSED ? 2 : 1)) return 2;
  const dim3 grid((unsigned)((n + GV_ROWS - 1) / GV_ROWS)), block(GV_THREADS);
  if (m <= 16)
    hipLaunchKernelGGL((k_igemv8<1, FUSED>), grid, block, 0, current_stream(), m, n, k, A, lda, B, ldb, out, ldc,
                       rowStats, rowStats_out, colStats, bias);
  else
    hipLaunchKernelGGL((k_igemv8<2, FUSED>), grid, block, 0, current_stream(), m, n, k, A, lda, B, ldb, out, ldc,
                       rowStats, rowStats_out, colStats, bias);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error((int)e, FUSED ? "int8_linear_rows launch" : "igemv launch"); return 1; }
  return 0;
}

int igemv_route(int m, int n, int k, const int8_t* A, const int8_t* B, fp16_t* out, const float* rowStats,
                const float* colStats, const fp16_t* bias, long long lda, long long ldb, long long ldc) {
  const int mode = g_igemv_mode;
  if (mode < 0) return 2;
  if (mode == 0 && m > ((long long)n * k <= GV_SMALL_WEIGHT ? GV_MAX_M : GV_AUTO_ROWS)) return 2;
  if (lda > 0x7fffffffLL || ldb > 0x7fffffffLL || ldc > 0x7fffffffLL) return 2;
  return launch_igemv8<false>(m, n, k, A, B, out, rowStats, nullptr, colStats, bias, (int)lda, (int)ldb, (int)ldc);
}

}  // namespace bnb

extern "C" {

// [additive] the decode kernel directly: int8 A [m, k] (1 <= m <= 32), int8 B [n, k], fp16 out [m, n].
// 0 = launched, 1 = error, 2 = not covered (or mode -1): nothing launched, nothing written
int cigemv_row_dequant_fp16(int m, int n, int k, const int8_t* A, const int8_t* B, fp16_t* out, const float* rowStats,
                            const float* colStats, const fp16_t* bias, int lda, int ldb, int ldc) {
  BNB_RANGE("cigemv_row_dequant_fp16");
  if (bnb::g_igemv_mode < 0) return 2;
  return bnb::launch_igemv8<false>(m, n, k, A, B, out, rowStats, nullptr, colStats, bias, lda, ldb, ldc);
}

// [additive] cint8_row_quant_fp16 + cigemv_row_dequant_fp16 in one launch: fp16 A [m, k] is quantised inside the
// kernel; rowStats_out (NULL: not wanted) receives the m row statistics.  CA is never written.  Same return codes.
int cint8_linear_rows_fp16(int m, int n, int k, const fp16_t* A, const int8_t* B, fp16_t* out, float* rowStats_out,
                           const float* colStats, const fp16_t* bias, int lda, int ldb, int ldc) {
  BNB_RANGE("cint8_linear_rows_fp16");
  if (bnb::g_igemv_mode < 0) return 2;
  return bnb::launch_igemv8<true>(m, n, k, A, B, out, nullptr, rowStats_out, colStats, bias, lda, ldb, ldc);
}

// [additive, testing] 0 = auto, 1 = the decode kernel wherever it covers, -1 = never; returns the previous value
int cigemv_set_mode(int mode) {
  return bnb::g_igemv_mode.exchange(mode > 0 ? 1 : (mode < 0 ? -1 : 0));
}

// the largest row count that currently reaches the decode kernel at every covered shape without being asked for by
// name: 0 in mode -1, the measured all-shapes limit of the automatic route in mode 0 (weights up to 11008 x 4096
// elements are routed up to 32 rows), the kernel's own 32 in mode 1
int cigemv_max_rows(void) {
  const int mode = bnb::g_igemv_mode;
  return mode < 0 ? 0 : (mode > 0 ? bnb::GV_MAX_M : bnb::GV_AUTO_ROWS);
}

}  // extern "C"
