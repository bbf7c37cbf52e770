// Fused 4-bit (NF4/FP4) weight GEMM for M > 1 (prefill) on gfx950 MFMA.
//
// Slot in the reference: cgemm_4bit_inference          ref:sycl/pythonInterface.cpp:377-378
//   -> gemm_4bit_inference<T>                          ref:sycl/sycl_code/op_gemm.cpp:843-889
//   -> kgemm_4bit_inference<T,96> (broken, Q7)         ref:sycl/sycl_code/kernel_gemm.cpp:1015-1265
// and the path it replaces for M > 1: MatMul4Bit.forward = dequantize_4bit + F.linear
//   ref:python_src_quants/autograd/_functions.py:491-507, functional.py:1291-1424.
//
// Argument convention (same as the gemv ABI, functional.py:1992-1997): m = out_features
// (rows of the packed weight W), n = activation rows (tokens), k = in_features;
//   out[t, r] = sum_k A[t*lda + k] * code[q(r,k)] * absmax[(2*ldb*r + k) / blocksize]
// A is [n, k] (row stride lda), out is [n, m] (row stride ldc), W rows are ldb bytes apart.
// Numerics = the reference M>1 path: each weight element is dequantised in fp32 and rounded
// once to T (bf16/fp16) exactly like dequantize_4bit, then multiplied on the bf16/fp16 MFMA
// with fp32 accumulation.
//
// Design (MI355X): 128x128 output tile per 256-thread workgroup (4 waves, 2x2, 64x64 per wave,
// v_mfma_f32_16x16x32_{bf16,f16}), BK = 64, two LDS stages.  Activations are staged by
// global_load_lds (16 B per lane, XOR-swizzled via the source address); the packed weight
// tile (4 KiB per stage: a quarter of the bf16 bytes) is loaded to registers, dequantised once
// per workgroup through a 256-entry LDS pair table and written to LDS as T in the same
// swizzled layout, so both MFMA operands are read with conflict-free ds_read_b128.
// XCD-aware tile order keeps the tiles that share activation panels on one XCD's L2.
#include "gemm_common.hpp"

#include <algorithm>

namespace bnb {

constexpr int G_BM = 128, G_BN = 128, G_BK = 64, G_THREADS = 256;
constexpr int G_TILE_BYTES = G_BM * G_BK * 2;        // 16 KiB per operand per stage
constexpr int G_LDS_BYTES = 4 * G_TILE_BYTES + 256 * 8;

template <typename T>
__global__ void __launch_bounds__(G_THREADS, 2)
k_gemm_4bit(int N, int M, int K, const T* __restrict__ A, const uint8_t* __restrict__ B,
            const float* __restrict__ absmax, const float* __restrict__ datatype, T* __restrict__ out,
            int lda, int ldb, int ldc, int blocksize) {
  // here: M = tokens (rows of A/out), N = out features (rows of W)
  __shared__ __attribute__((aligned(16))) uint8_t smem[G_LDS_BYTES];
  uint8_t* Xs = smem;                                  // [2][128][64] T
  uint8_t* Ws = smem + 2 * G_TILE_BYTES;               // [2][128][64] T
  float2* lut = reinterpret_cast<float2*>(smem + 4 * G_TILE_BYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  lut[tid] = make_float2(datatype[tid >> 4], datatype[tid & 15]);

  // ---- XCD-aware tile mapping (bijective for any grid size)
  const int tilesN = (N + G_BN - 1) / G_BN;
  const int tilesM = (M + G_BM - 1) / G_BM;
  const int nwg = tilesN * tilesM;
  int wg = blockIdx.x;
  {
    const int xcd = wg & 7, q = nwg >> 3, r = nwg & 7;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wg >> 3);
  }
  // group 8 token-tiles together so an XCD's consecutive tiles share weight panels too
  constexpr int GROUP = 8;
  const int group_span = GROUP * tilesN;
  const int gidx = wg / group_span;
  const int first_m = gidx * GROUP;
  const int gsize = min(tilesM - first_m, GROUP);
  const int tm = first_m + (wg % group_span) % gsize;
  const int tn = (wg % group_span) / gsize;
  const int m0 = tm * G_BM, n0 = tn * G_BN;

  // ---- per-thread staging roles
  // activations: 4 glds per wave per stage; wave-instruction i covers rows 8*(4*wave+i) .. +7
  const T* xsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * (4 * wave + i) + (lane >> 3);
    const int grow = min(m0 + row, M - 1);
    const int gslot = (lane & 7) ^ (row & 7);
    xsrc[i] = A + (long long)grow * lda + 8 * gslot;
  }
  // weights: thread t -> row t>>1, half h (32 elements = 16 packed bytes)
  const int wrow = tid >> 1, wh = tid & 1;
  const int gwrow = min(n0 + wrow, N - 1);
  const uint8_t* wsrc = B + (long long)gwrow * ldb + 16 * wh;
  const long long am_base = 2LL * ldb * gwrow + 32 * wh;

  const int wm = wave >> 1, wn = wave & 1;
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = K / G_BK;

  // prologue: stage 0 activations, weights of k-tile 0 to registers
#pragma unroll
  for (int i = 0; i < 4; ++i) glds16(xsrc[i], Xs + (4 * wave + i) * 1024);
  uint4 wq = ld_nt16(wsrc);
  float wam = absmax[am_base / blocksize];
  __syncthreads();   // lut ready

  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    uint8_t* xs = Xs + cur * G_TILE_BYTES;
    uint8_t* ws = Ws + cur * G_TILE_BYTES;
    // dequantise this k-tile's weights into LDS (each element once per workgroup)
    {
      const uint32_t w[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        uint32_t pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float2 c = lut[(w[s] >> (8 * j)) & 0xFF];
          pk[j] = Mfma<T>::pack2(__fmul_rn(c.x, wam), __fmul_rn(c.y, wam));
        }
        *reinterpret_cast<uint4*>(ws + swz(wrow, 4 * wh + s)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < nk) {
      const int k1 = (t + 1) * G_BK;
      uint8_t* xn = Xs + (cur ^ 1) * G_TILE_BYTES;
#pragma unroll
      for (int i = 0; i < 4; ++i) glds16(xsrc[i] + k1, xn + (4 * wave + i) * 1024);
      wq = ld_nt16(wsrc + k1 / 2);
      wam = absmax[(am_base + k1) / blocksize];
    }
    // MFMA on the current stage
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 a[4], b[4];
      const int slot = 4 * ks + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const uint4*>(xs + swz(64 * wm + 16 * i + (lane & 15), slot));
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const uint4*>(ws + swz(64 * wn + 16 * j + (lane & 15), slot));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = Mfma<T>::mma(a[i], b[j], acc[i][j]);
    }
  }

  // epilogue: C/D map of 16x16x32: col = lane&15, row = 4*(lane>>4) + r
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + 64 * wn + 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + 64 * wm + 16 * i + 4 * (lane >> 4) + r;
        if (row < M && col < N) out[(long long)row * ldc + col] = Io<T>::from_f32(acc[i][j][r]);
      }
    }
  }
}

Knob<int> g_tile_override{0};

// Split-K factor for the 256-tile kernel: enough workgroups to cover the 256 CUs when the output has
// fewer than ~200 256x256 tiles (narrow column shards, e.g. N/8 = 512 features at M = 4096, or few
// tokens: 16 x 4096 x 11008 ran 176 us on the 32-workgroup 128-tile grid), with at least 8 k-tiles
// per split.  Below 256 weight rows (the 70B k/v shard 128 x 8192 at 4096 tokens: 16 half-empty tiles) the split
// form still beats the 128-tile kernel's 32 whole-K workgroups (151 us there; profiles/lab/r02_narrow_weight.txt).
// Needs a caller-supplied fp32 workspace of ksplit * m * n floats.
static int splitk_factor(int m, int n, int k) {
  if (m < 64) return 1;
  const long long tiles = (long long)((m + 255) / 256) * ((n + 255) / 256);
  if (tiles >= 200) return 1;
  int ks = (int)((256 + tiles / 2) / tiles);
  ks = std::min(ks, std::max(1, (k / G_BK) / 8));
  return std::max(1, std::min(ks, 16));
}
static long long splitk_bytes(int ks, int m, int n) { return ks > 1 ? (long long)ks * m * n * (long long)sizeof(float) : 0; }

// The plan's last stage, the tile kernels (plain statistics only).  Large problems: 256x256 tiles (split-K when the
// tile grid is too small and a workspace is given); small: 128x128.
static FtPlan tile_plan(const FtKnobs& kn, const FtProblem& p) {
  FtPlan pl;
  if (p.nested) return pl;
  const int m = p.m, n = p.n, k = p.k;
  if (k <= 0 || k % G_BK != 0 || !ft_aligned(p) || p.blocksize < 64 || p.blocksize % 32 != 0) {
    pl.kernel = FT_BAD_ARGS;
    return pl;
  }
  const long long tiles256 = (long long)((m + 255) / 256) * ((n + 255) / 256);
  int ks = splitk_factor(m, n, k);
  if (!p.ws_fits(splitk_bytes(ks, m, n))) ks = 1;
  // 256x256 (with split-K) when its grid fills the chip (>= 128 workgroups), and also when it still has at
  // least half the workgroups of the 128x128 grid, which then run the full K each (e.g. 512 features x
  // 256 tokens: 8 workgroups of 128x128 took 174 us where 2 x 16-way split 256x256 tiles take ~25)
  const long long tiles128 = (long long)((m + G_BN - 1) / G_BN) * ((n + G_BM - 1) / G_BM);
  const bool use256 = ft_pow2(p.blocksize) &&
                      (kn.tile_override == 256 || (kn.tile_override != 128 && (m >= 256 || ks > 1) &&
                                                   (tiles256 * ks >= 128 || 2 * tiles256 * ks >= tiles128)));
  pl.kernel = use256 ? FT_TILE256 : FT_TILE128;
  pl.splits = use256 ? ks : 1;
  pl.kchunk = k / G_BK;
  pl.grid = (int)(use256 ? tiles256 * ks : tiles128);
  pl.threads = use256 ? 512 : G_THREADS;
  pl.waves = pl.threads / 64;
  pl.reduce = pl.splits > 1;
  pl.ws_bytes = splitk_bytes(pl.splits, m, n);
  return pl;
}

// The stages in order; the first that takes the problem runs it.
//   * the multi-row GEMV (only where the caller allows it): 2..4 rows that the whole-K MFMA kernel does not take;
//   * 33..64 tokens: the split-K tile kernel that shares the token rows across 192 weight rows (gemm4bit_t64.hip);
//   * then the whole-K MFMA kernel (gemm4bit_fewtok.hip) -- neither where a lab / test knob selects one of the older
//     kernels (g_fewtoken_kernel, a forced split-K geometry);
//   * the older weight-streaming kernels (gemm4bit_wk.hip, gemm4bit_skinny.hip);
//   * the tile kernels, alone when g_tile_override names one.
FtPlan fewtoken_plan(const FtKnobs& kn, const FtProblem& p) {
  if (kn.tile_override == 0) {
    const bool newer = kn.fewtoken_kernel == 0 && kn.skinny_cfg < 0;
    const FtPlan ft = newer ? fewtok_plan(kn, p) : FtPlan{};
    FtPlan pl;
    if (p.allow_gemv && ft.kernel == FT_NONE && (pl = gemv_tok_plan(p)).kernel != FT_NONE) return pl;
    if (newer && (pl = t64_plan(kn, p)).kernel != FT_NONE) return pl;
    if (ft.kernel != FT_NONE) return ft;
    if ((pl = wk_plan(kn, p)).kernel != FT_NONE) return pl;
    if ((pl = skinny_plan(kn, p)).kernel != FT_NONE) return pl;
  }
  return tile_plan(kn, p);
}

// room for the partials of whichever kernel the plan picks, under any knob setting
long long gemm_4bit_workspace_bytes(int m, int n, int k) {
  return std::max({splitk_bytes(splitk_factor(m, n, k), m, n), skinny_workspace_bytes(m, n, k),
                   t64_workspace_bytes(FtKnobs::load(), m, n, k)});
}

// 0 launched, 1 only a kernel that needs plain statistics is left (nothing launched), 2 error (recorded)
template <typename T>
static int gemm_4bit(int m, int n, int k, const FtArgs<T>& a, int lda, int ldb, int blocksize, int blocksize2,
                     long long ws_bytes, bool allow_gemv) {
  if (m <= 0 || n <= 0) return 0;
  const FtProblem p = ft_problem(m, n, k, lda, ldb, blocksize, blocksize2, a, ws_bytes, allow_gemv);
  const FtPlan pl = fewtoken_plan(FtKnobs::load(), p);
  switch (pl.kernel) {
    case FT_NONE: return 1;
    case FT_BAD_ARGS:
      set_error(1, "gemm_4bit: requires k % 64 == 0, lda % 8 == 0, ldb % 16 == 0, 16-B aligned A/B, blocksize >= 64");
      return 2;
    case FT_GEMV_TOK: gemv_tok_launch<T>(p, a, pl); break;
    case FT_T64:
    case FT_T64R: t64_launch<T>(p, a, pl); break;
    case FT_FEWTOK: fewtok_launch<T>(p, a, pl); break;
    case FT_WK: wk_launch<T>(p, a, pl); break;
    case FT_SKINNY: launch_gemm_4bit_skinny<T>(p, a, pl); break;
    case FT_TILE256:
      launch_gemm_4bit_256<T>(m, n, k, a.A, a.B, a.absmax, a.code, a.out, lda, ldb, a.ldc, blocksize, a.ws, pl.splits);
      break;
    default:
      hipLaunchKernelGGL((k_gemm_4bit<T>), dim3(pl.grid), dim3(G_THREADS), 0, current_stream(), m, n, k, a.A, a.B,
                         a.absmax, a.code, a.out, lda, ldb, a.ldc, blocksize);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error((int)e, "gemm_4bit");
    return 2;
  }
  return 0;
}
// plain statistics, no workspace, never the multi-row GEMV: the reference slots
template <typename T>
static void gemm_4bit_plain(int m, int n, int k, const T* A, const uint8_t* B, const float* absmax, const float* datatype,
                            T* out, int lda, int ldb, int ldc, int blocksize) {
  gemm_4bit<T>(m, n, k, FtArgs<T>{A, B, absmax, nullptr, nullptr, nullptr, nullptr, datatype, out, ldc, nullptr}, lda, ldb,
               blocksize, 0, 0, false);
}

static __device__ float g_nf4_table[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
    0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

static const float* nf4_table_device() {
  void* p = nullptr;
  hipGetSymbolAddress(&p, HIP_SYMBOL(g_nf4_table));
  return (const float*)p;
}

}  // namespace bnb

using namespace bnb;

extern "C" {

// Reference ABI slot (NF4 hard-coded, fp16), ref:sycl/pythonInterface.cpp:377-378.
void cgemm_4bit_inference(int m, int n, int k, fp16_t* A, unsigned char* B, float* absmax, fp16_t* out, int lda,
                          int ldb, int ldc, int blocksize) {
  BNB_RANGE("cgemm_4bit_inference");
  gemm_4bit_plain<fp16_t>(m, n, k, A, B, absmax, nf4_table_device(), out, lda, ldb, ldc, blocksize);
}
// bf16 sibling and table-driven variants (any 16-entry code: NF4/FP4).
void cgemm_4bit_inference_bf16(int m, int n, int k, bf16_t* A, unsigned char* B, float* absmax, bf16_t* out, int lda,
                               int ldb, int ldc, int blocksize) {
  BNB_RANGE("cgemm_4bit_inference_bf16");
  gemm_4bit_plain<bf16_t>(m, n, k, A, B, absmax, nf4_table_device(), out, lda, ldb, ldc, blocksize);
}
void cgemm_4bit_inference_code_fp16(int m, int n, int k, fp16_t* A, unsigned char* B, float* absmax, float* datatype,
                                    fp16_t* out, int lda, int ldb, int ldc, int blocksize) {
  BNB_RANGE("cgemm_4bit_inference_code_fp16");
  gemm_4bit_plain<fp16_t>(m, n, k, A, B, absmax, datatype, out, lda, ldb, ldc, blocksize);
}
void cgemm_4bit_inference_code_bf16(int m, int n, int k, bf16_t* A, unsigned char* B, float* absmax, float* datatype,
                                    bf16_t* out, int lda, int ldb, int ldc, int blocksize) {
  BNB_RANGE("cgemm_4bit_inference_code_bf16");
  gemm_4bit_plain<bf16_t>(m, n, k, A, B, absmax, datatype, out, lda, ldb, ldc, blocksize);
}
// [additive] the 4-bit GEMM of the Python layer, any number of activation rows, with a caller-owned fp32 workspace
// (cgemm_4bit_workspace_bytes; a smaller or NULL workspace only rules out the kernels that split K): plain fp32
// statistics (absmax_q = NULL) or compressed ones decoded in-kernel (absmax = NULL).  The one entry that may run 2..4
// rows on the multi-row GEMV: up to gemv_rows of them (0: never).  Returns 0 when launched, 1 when only a kernel that needs plain statistics is left
// (nothing launched: decode them and call again), 2 on error.
int cgemm_4bit_inference_ws_fp16(int m, int ntok, int k, fp16_t* A, int lda, unsigned char* B, int ldb, float* absmax,
                                 unsigned char* absmax_q, float* code2, float* absmax2, float* offset, float* datatype,
                                 fp16_t* out, int ldc, int blocksize, int blocksize2, float* workspace,
                                 long long workspace_bytes, int gemv_rows) {
  BNB_RANGE("cgemm_4bit_inference_ws_fp16");
  return gemm_4bit<fp16_t>(m, ntok, k, FtArgs<fp16_t>{A, B, absmax, absmax_q, code2, absmax2, offset, datatype, out, ldc, workspace},
                           lda, ldb, blocksize, blocksize2, workspace_bytes, ntok <= gemv_rows);
}
int cgemm_4bit_inference_ws_bf16(int m, int ntok, int k, bf16_t* A, int lda, unsigned char* B, int ldb, float* absmax,
                                 unsigned char* absmax_q, float* code2, float* absmax2, float* offset, float* datatype,
                                 bf16_t* out, int ldc, int blocksize, int blocksize2, float* workspace,
                                 long long workspace_bytes, int gemv_rows) {
  BNB_RANGE("cgemm_4bit_inference_ws_bf16");
  return gemm_4bit<bf16_t>(m, ntok, k, FtArgs<bf16_t>{A, B, absmax, absmax_q, code2, absmax2, offset, datatype, out, ldc, workspace},
                           lda, ldb, blocksize, blocksize2, workspace_bytes, ntok <= gemv_rows);
}
long long cgemm_4bit_workspace_bytes(int m, int n, int k) { return gemm_4bit_workspace_bytes(m, n, k); }
// [additive, testing] the launch plan of cgemm_4bit_inference_ws_* for contiguous, aligned operands (lda = k,
// ldb = k / 2) and a workspace of cgemm_4bit_workspace_bytes: out[0..15] = {kernel (FtKernel, gemm_common.hpp), grid,
// threads, splits, kchunk, mt, rg, waves, s4, x8, cfg, lds, reduce launch follows, workspace bytes used (low, high 32
// bits), 0}
void cgemm_4bit_plan(int m, int ntok, int k, int blocksize, int blocksize2, int nested, int* out) {
  BNB_RANGE("cgemm_4bit_plan");
  const FtProblem p{m, ntok, k, k, k / 2, blocksize, blocksize2, nested != 0, true, true, true, true,
                    gemm_4bit_workspace_bytes(m, ntok, k), true};
  const FtPlan pl = fewtoken_plan(FtKnobs::load(), p);
  const int v[16] = {pl.kernel, pl.grid, pl.threads, pl.splits, pl.kchunk, pl.mt, pl.rg, pl.waves, pl.s4, pl.x8, pl.cfg,
                     pl.lds, pl.reduce ? 1 : 0, (int)(pl.ws_bytes & 0xFFFFFFFFLL), (int)(pl.ws_bytes >> 32), 0};
  std::copy(v, v + 16, out);
}
// [additive, testing] force the tile kernel used by the 4-bit GEMM (0 = auto, 128 = 128x128 kernel)
void cgemm_4bit_set_tile(int tile) { bnb::g_tile_override = tile; }

}  // extern "C"
