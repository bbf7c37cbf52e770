// Shared MFMA / LDS helpers for the 4-bit GEMM kernels (gfx950).
#pragma once

#include "common.hpp"

namespace bnb {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// v_mfma_f32_16x16x32_{bf16,f16}: lane l holds A[row l&15][k 8(l>>4)..+7], B[k ..][col l&15];
// C/D: col = l&15, row = 4(l>>4) + reg.
template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
  __device__ static __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
  __device__ static __forceinline__ uint32_t pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
};
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
// 32x32x16 (gfx950): lane l holds A[row l&31][k 8(l>>5)..+8] and B[k 8(l>>5)..+8][col l&31];
// D[r]: row 8(r>>2) + 4(l>>5) + (r&3), col l&31.  An MFMA holds the SIMD's vector issue for 8 of
// its 32 cycles (vs 8 of 16 for 16x16x32), leaving 3x the issue slots for the in-loop dequant.
template <typename T> struct Mfma32;
template <> struct Mfma32<bf16_t> {
  __device__ static __forceinline__ f32x16_t mma(const uint4& a, const uint4& b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
};
template <> struct Mfma32<fp16_t> {
  __device__ static __forceinline__ f32x16_t mma(const uint4& a, const uint4& b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};

template <> struct Mfma<fp16_t> {
  __device__ static __forceinline__ f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
  __device__ static __forceinline__ uint32_t pack2(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, Io<fp16_t>::from_f32(lo)) |
           ((uint32_t)__builtin_bit_cast(uint16_t, Io<fp16_t>::from_f32(hi)) << 16);
  }
};

// LDS-DMA: 16 B (or 4 B) per lane from a per-lane global address to lds_base + lane*size.
// Issued from inline asm on purpose: with __builtin_amdgcn_global_load_lds, hipcc (ROCm 7.2) treats
// every later ds_read of the same __shared__ array as aliasing the in-flight DMA and drains it with
// s_waitcnt vmcnt(0) right there, serialising the prefetch.  The asm form is invisible to that
// bookkeeping, so the caller owns the wait: `s_waitcnt vmcnt(0)` before the barrier that publishes
// the stage.  lds_base must be wave-uniform (it goes to M0; M0 is saved/restored in the statement).
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_base) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds_base);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, void* lds_base) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds_base);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}
__device__ __forceinline__ void wait_vmcnt0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// byte offset of 16-B slot s (0..7) of row r in a [rows][64] 16-bit tile, XOR swizzled so that
// 16 lanes reading one slot of 16 consecutive rows (MFMA fragment) hit distinct banks
__device__ __forceinline__ int swz(int r, int s) { return r * 128 + ((s ^ (r & 7)) << 4); }

// bijective XCD-aware remap of the workgroup id (consecutive ids land on one XCD's L2)
__device__ __forceinline__ int xcd_remap(int wg, int nwg) {
  const int xcd = wg & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wg >> 3);
}

// ---------------------------------------------------------------- the 4-bit GEMM launch plan
// Which kernel runs m weight rows x n activation rows x k, and in what geometry, is decided in one place:
// fewtoken_plan (gemm4bit.hip) asks each kernel file's X_plan in a fixed order, gemm_4bit<T> switches on the result
// and cgemm_4bit_plan reports it to tests (the shape of hgemm.hip's HgKnobs / hgemm_plan / chgemm_tn_plan).  A kernel
// file keeps its kernel, its measured rule (X_plan: a geometry, or "does not take it") and its launch (X_launch:
// consumes the geometry, re-tests nothing).

// The A/B and test knobs, each defined beside its setter (cgemm_4bit_set_*)
extern Knob<int> g_tile_override;     // gemm4bit.hip: 0 = auto, 128 / 256 = that tile kernel, no few-token kernel
extern Knob<int> g_fewtoken_kernel;   // gemm4bit_wk.hip
extern Knob<int> g_skinny_cfg;        // gemm4bit_skinny.hip
extern Knob<int> g_fewtok_mode;       // gemm4bit_fewtok.hip
extern Knob<int> g_t64_mode, g_t64_ks, g_t64_kp, g_t64r, g_t64_combine, g_t64_pstore;   // gemm4bit_t64.hip

// One launch's view of the knobs: each is loaded once, when the launch (or a plan query) starts, and nothing below
// reads a global again -- a setter on another thread changes the next launch, never the middle of this one.
struct FtKnobs {
  int fewtoken_kernel, skinny_cfg, fewtok_mode, t64_mode, t64_ks, t64_kp, t64r, t64_combine, t64_pstore, tile_override;
  static FtKnobs load() {
    return FtKnobs{g_fewtoken_kernel, g_skinny_cfg, g_fewtok_mode, g_t64_mode, g_t64_ks,
                   g_t64_kp,          g_t64r,       g_t64_combine, g_t64_pstore, g_tile_override};
  }
};

// m = out features (weight rows), n = activation rows (tokens), k = in features; A rows lda elements apart, packed
// weight rows ldb bytes apart.  Statistics are plain fp32 (one per blocksize weights) or nested (8-bit codes, decoded
// in the kernel; blocksize2 codes per second-level absmax).
struct FtProblem {
  int m, n, k, lda, ldb, blocksize, blocksize2;
  bool nested;
  bool a16, b16;          // A / B 16-B aligned
  bool stats16;           // the statistics take vector loads: plain absmax 16-B aligned, nested codes 4-B aligned
  bool ws16;              // a workspace is given and 16-B aligned
  long long ws_bytes;
  bool allow_gemv;        // the multi-row GEMV may be chosen (its rows are bit-identical to gemv_4bit's, the MFMA kernels' not)
  bool ws_fits(long long bytes) const { return ws16 && bytes <= ws_bytes; }
};
inline bool ft_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }
// what every weight-streaming kernel loads by: 16-B pieces of A and B rows
inline bool ft_aligned(const FtProblem& p) { return p.lda % 8 == 0 && p.ldb % 16 == 0 && p.a16 && p.b16; }
// ... and indexes its statistics by: shifts (power-of-two blocks of >= 64 weights, power-of-two nested groups)
inline bool ft_stream_ok(const FtProblem& p) {
  return ft_aligned(p) && p.blocksize >= 64 && ft_pow2(p.blocksize) && (!p.nested || ft_pow2(p.blocksize2));
}

enum FtKernel {
  FT_NONE = 0,      // a stage: does not take it; the plan: only the tile kernels are left and they need plain statistics
  FT_BAD_ARGS,      // the tile kernels' argument contract is not met (an error)
  FT_GEMV_TOK,      // k_gemv_4bit_tok      gemv4bit_tok.hip     mt = TOK, rg = R, cfg = U, lds
  FT_T64,           // k_gemm_4bit_t64      gemm4bit_t64.hip     waves 4 / 8 (KP 1 / 2), splits, kchunk
  FT_T64R,          // k_gemm_4bit_t64r                          kchunk
  FT_FEWTOK,        // k_gemm_4bit_fewtok   gemm4bit_fewtok.hip  rg = RG, mt = MT, s4, waves, x8
  FT_WK,            // k_gemm_4bit_wk       gemm4bit_wk.hip      mt = MT, waves, rg = D
  FT_SKINNY,        // k_gemm_4bit_skinny   gemm4bit_skinny.hip  mt = MT, rg = NB, waves, cfg, splits
  FT_TILE128,       // k_gemm_4bit          gemm4bit.hip
  FT_TILE256,       // k_gemm_4bit_256      gemm4bit_256.hip     splits
};
struct FtPlan {
  int kernel = FT_NONE;
  int grid = 0, threads = 0;     // workgroups, threads per workgroup
  int splits = 1, kchunk = 0;    // K splits; the k-chunk of one split in the kernel's own unit
  int mt = 0, rg = 0, waves = 0, s4 = 0, x8 = 0, cfg = 0;   // the template choice, per kernel as listed above
  int lds = 0;                   // dynamic LDS bytes
  int pstore = 0, combine = 0;   // t64: partial-store policy, in-kernel combine wanted
  int lab = 0;                   // lab build: the ablation mode that picks the instance
  bool reduce = false;           // a reduce launch over the fp32 split partials follows
  long long ws_bytes = 0;        // workspace the launch uses
};
FtPlan fewtoken_plan(const FtKnobs& kn, const FtProblem& p);

// statistics as the kernels take them
struct SkStats {
  const float* absmax;
  const uint8_t* q8;
  const float* code2;
  const float* absmax2;
  const float* offset;
  int bs_shift, bs2_shift;
};
// the operands of one launch
template <typename T> struct FtArgs {
  const T* A;
  const uint8_t* B;
  const float* absmax;      // plain statistics, or
  const uint8_t* q8;        // nested: codes, code2, absmax2, offset
  const float* code2;
  const float* absmax2;
  const float* offset;
  const float* code;        // the 16-entry 4-bit data type
  T* out;
  int ldc;
  float* ws;
};
template <typename S, typename T> inline S ft_stats(const FtProblem& p, const FtArgs<T>& a) {
  return S{a.absmax, a.q8, a.code2, a.absmax2, a.offset, __builtin_ctz(p.blocksize),
           p.nested ? __builtin_ctz(p.blocksize2) : 0};
}
template <typename T>
inline FtProblem ft_problem(int m, int n, int k, int lda, int ldb, int blocksize, int blocksize2, const FtArgs<T>& a,
                            long long ws_bytes, bool allow_gemv) {
  const bool nested = a.q8 != nullptr;
  return FtProblem{m, n, k, lda, ldb, blocksize, blocksize2, nested,
                   ((uintptr_t)a.A & 15) == 0, ((uintptr_t)a.B & 15) == 0,
                   nested ? ((uintptr_t)a.q8 & 3) == 0 : ((uintptr_t)a.absmax & 15) == 0,
                   a.ws != nullptr && ((uintptr_t)a.ws & 15) == 0, ws_bytes, allow_gemv};
}

// Multi-row GEMV (gemv4bit_tok.hip): 2..4 activation rows, whole K per workgroup, no workspace
FtPlan gemv_tok_plan(const FtProblem& p);
template <typename T> void gemv_tok_launch(const FtProblem& p, const FtArgs<T>& a, const FtPlan& pl);
// The 33..64-token kernel (gemm4bit_t64.hip): K % 256 == 0, blocksize 64; fp32 split partials when K is split
FtPlan t64_plan(const FtKnobs& kn, const FtProblem& p);
long long t64_workspace_bytes(const FtKnobs& kn, int m, int n, int k);
template <typename T> void t64_launch(const FtProblem& p, const FtArgs<T>& a, const FtPlan& pl);
// Few-token kernel on the 32x32x16 MFMA, whole K per workgroup, no workspace (gemm4bit_fewtok.hip): 1..32 rows,
// K % 64 == 0
FtPlan fewtok_plan(const FtKnobs& kn, const FtProblem& p);
template <typename T> void fewtok_launch(const FtProblem& p, const FtArgs<T>& a, const FtPlan& pl);
// Few-token kernel with whole K per workgroup (gemm4bit_wk.hip): 1..32 rows, K % 128 == 0, no workspace
FtPlan wk_plan(const FtKnobs& kn, const FtProblem& p);
template <typename T> void wk_launch(const FtProblem& p, const FtArgs<T>& a, const FtPlan& pl);
// Split-K few-token kernel (gemm4bit_skinny.hip): 1..64 rows (SK_MAX_TOKENS), K % 128 == 0
FtPlan skinny_plan(const FtKnobs& kn, const FtProblem& p);
long long skinny_workspace_bytes(int m, int n, int k);
template <typename T> void launch_gemm_4bit_skinny(const FtProblem& p, const FtArgs<T>& a, const FtPlan& pl);
// out[t, n] = T(sum_s ws[s][t][n]) (fp32 split partials, row-major [rows][cols] per split), splits summed in order
template <typename T>
void launch_splitk_rows_reduce(const float* ws, int nsplit, int rows, int cols, T* out, int ldc);
// The 256 x 256 tile kernel (gemm4bit_256.hip).  ws/ksplit: split-K over ksplit workgroups per tile with fp32 partials
// in ws[ksplit][n][m] (ksplit == 1: ws unused, direct T output)
template <typename T>
void launch_gemm_4bit_256(int m, int n, int k, const T* A, const uint8_t* B, const float* absmax, const float* datatype,
                          T* out, int lda, int ldb, int ldc, int blocksize, float* ws, int ksplit);

}  // namespace bnb
