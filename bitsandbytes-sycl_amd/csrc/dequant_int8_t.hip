// Transposing int8 row dequantise for gfx950: the LLM.int8 weight CB (int8, row-major [N, K]) with its row absmax SCB
// (fp32 [N]) -> out[k * ldo + n] in bf16 / fp16, the W^T [K, N] operand image of the input-gradient product
// grad[M, N] @ W[N, K] (chgemm_tn_* with m = rows, n = K, k = N).  [additive] cdequantize_int8_rows_t_{bf16,fp16}.
//
// Values: the bits of CB.to(T).mul_(SCB.unsqueeze(1).mul(1.0 / 127.0)) as torch computes it on this device, so the
// result equals that tensor's .t().contiguous() bit for bit.  The row scale s = fmul_rn(SCB[n], (float)(1.0 / 127.0))
// is formed first, in fp32.  bf16: RNE(fmul_rn(float(CB[n, k]), s)).  fp16: the exact product float(CB[n, k]) * s
// rounded once to fp16 (one fused multiply-convert, dq8t_value below).  The build has -ffp-contract=off; the two
// multiplies are never fused with each other.
//
// Shape: one workgroup (256 lanes) owns a 64 (n) x 128 (k) tile.
//   load     lane (rp, kc) = (t >> 3, t & 7) reads the 16-B chunk kc (16 weights along k) of rows 2 rp and 2 rp + 1:
//            each load instruction reads 128 contiguous bytes of 8 rows; both loads and both row scales are issued
//            before any is consumed (non-temporal: the weight is read once);
//   LDS      the tile is stored k-major, 64 16-bit values = 32 dwords = 8 16-B chunks per k row, no padding.  A lane
//            packs the values of its two rows (n, n + 1) at one k into one 32-bit write: dword rp & 3 of chunk rp >> 2.
//            The chunks of row k are placed at chunk ^ ((k >> 4) & 7): a 32-lane write group is 4 rp's (the 4 dwords
//            of one chunk) x 8 kc's, which the XOR sends to 8 different chunks -- 32 different banks, conflict-free
//            under the (a / 4) mod 32 rule of ds_write_b32;
//   read-out lane (kr, c) = (t >> 3, t & 7) reads the chunk c of row k, one ds_read_b128 at c ^ ((k >> 4) & 7).  A
//            16-lane group of ds_read_b128 covers 4 consecutive rows that share k >> 4: the two even rows (one half of
//            the 256-B bank row) are read at chunks {0..3} ^ x and {4..7} ^ x, the two odd rows likewise --
//            conflict-free under (a / 4) mod 64;
//   store    one 16-B store per lane, 8 lanes = one 128-B run of an output row; device-scope write-through through a
//            buffer resource (the policy of the 4-bit transposing kernel), 32-bit byte offsets.
// Ragged tiles: load addresses are clamped inside CB (row min(n, N - 1), chunk min(k, K - 16)), stores are masked to
// columns [0, N) of rows [0, K) and bounded by the buffer resource.  No atomics.
#include "common.hpp"

namespace bnb {

typedef uint32_t dq8t_u32x4 __attribute__((ext_vector_type(4)));

// one weight: float(cb) * s into T's bits.  bf16: the fp32 product (one __fmul_rn), then one RNE cast.
template <typename T> __device__ __forceinline__ uint32_t dq8t_value(float cb, float s) {
  return (uint32_t)Io<T>::from_f32(__fmul_rn(cb, s));
}
// fp16: torch's elementwise kernel computes this product and its conversion as ONE v_fma_mixlo_f16 with a +0 addend
// on gfx950 -- the exact product rounded once to fp16, not the fp32 product rounded again (they differ where the fp32
// product falls on the midpoint of two fp16 values: measured 0-31 of 67,200-327,680 elements), and a product of
// exactly -0 (a negative weight under a zero row statistic) becomes +0.  The explicit fma + conversion selects the same
// instruction (checked: every conversion of this kernel is a v_fma_mixlo/mixhi_f16); Io<fp16_t>'s barrier, which
// exists to keep that instruction away, is not used here.
template <> __device__ __forceinline__ uint32_t dq8t_value<fp16_t>(float cb, float s) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (fp16_t)__builtin_fmaf(cb, s, 0.0f));
}

constexpr int DQ8T_TN = 64, DQ8T_TK = 128;

template <typename T>
__global__ void __launch_bounds__(256)
k_dequantize_int8_t(const int8_t* __restrict__ CB, const float* __restrict__ SCB, T* __restrict__ out, int N, int K,
                    int ldo, int n_tiles) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tile[DQ8T_TK * DQ8T_TN / 2];
  constexpr int TN = DQ8T_TN;
  const int t = threadIdx.x;
  // n tiles run fastest: workgroups in flight together fill whole output rows
  const int n0 = (int)(blockIdx.x % (unsigned)n_tiles) * TN;
  const int k0 = (int)(blockIdx.x / (unsigned)n_tiles) * DQ8T_TK;
  const int kc = t & 7, rp = t >> 3;

  // rows past N and chunks past K are clamped to bytes inside CB (K % 16 == 0, K >= 16); never stored
  const int kld = min(k0 + 16 * kc, K - 16);
  dq8t_u32x4 w[2];
  float sc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = min(n0 + 2 * rp + j, N - 1);
    w[j] = __builtin_nontemporal_load(reinterpret_cast<const dq8t_u32x4*>(CB + ((long long)n * K + kld)));
    sc[j] = SCB[n];
  }
  const float s0 = __fmul_rn(sc[0], (float)(1.0 / 127.0));
  const float s1 = __fmul_rn(sc[1], (float)(1.0 / 127.0));

  // rows (n, n + 1) of one k pack into one dword of the k-major tile
  const int col = (((rp >> 2) ^ kc) << 2) | (rp & 3);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float v0 = (float)(int)(int8_t)(w[0][d] >> (8 * b));
      const float v1 = (float)(int)(int8_t)(w[1][d] >> (8 * b));
      s_tile[(16 * kc + 4 * d + b) * (TN / 2) + col] = dq8t_value<T>(v0, s0) | (dq8t_value<T>(v1, s1) << 16);
    }
  }
  __syncthreads();

  // read-out: 16-B chunks along n, 8 lanes per output row
  constexpr int CH = TN / 8, RPP = 256 / CH;         // chunks per row, rows per pass
  const int c = t % CH;
  const int n = n0 + 8 * c;
  // (bytes up to the last element of the last row: the launcher keeps them below 2 GiB)
  const uint32_t out_bytes = (uint32_t)(((long long)(K - 1) * ldo + N) * 2);
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(out, (short)0, (int)out_bytes, 0x00020000);
#pragma unroll
  for (int p = 0; p < DQ8T_TK / RPP; ++p) {
    const int kl = RPP * p + t / CH;
    const uint4 v = reinterpret_cast<const uint4*>(s_tile)[kl * CH + (c ^ ((kl >> 4) & 7))];
    const dq8t_u32x4 o = {v.x, v.y, v.z, v.w};
    const int k = k0 + kl;
    if (k < K && n < N)
      __builtin_amdgcn_raw_buffer_store_b128(o, r, (int)(((long long)k * ldo + n) * 2), 0, 16);
  }
}

// 0 launched (or nothing to do), 1 shape / alignment not supported (nothing launched), 2 launch error
template <typename T>
static int dequantize_int8_t(const int8_t* CB, const float* SCB, T* out, int rows, int cols, int ldo, const char* name) {
  const int N = rows, K = cols;
  if (N < 0 || K < 0) return 1;
  if (N == 0 || K == 0) return 0;
  if (N % 8 || K % 16 || ldo < N || ldo % 8) return 1;
  if (((uintptr_t)CB & 15) || ((uintptr_t)SCB & 3) || ((uintptr_t)out & 15)) return 1;
  // every input and output byte offset is a 32-bit offset below 2 GiB
  if ((long long)N * K > 0x7FFFFFFFLL) return 1;
  if (((long long)(K - 1) * ldo + N) * 2 > 0x7FFFFFFFLL) return 1;
  const int n_tiles = (N + DQ8T_TN - 1) / DQ8T_TN;
  const long long tiles = (long long)n_tiles * ((K + DQ8T_TK - 1) / DQ8T_TK);
  if (tiles > 0x7FFFFFFFLL) return 1;
  hipLaunchKernelGGL((k_dequantize_int8_t<T>), dim3((unsigned)tiles), dim3(256), 0, current_stream(), CB, SCB, out, N,
                     K, ldo, n_tiles);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error((int)e, name);
    return 2;
  }
  return 0;
}

}  // namespace bnb

using namespace bnb;

extern "C" {

int cdequantize_int8_rows_t_bf16(const signed char* CB, const float* SCB, bf16_t* out, int rows, int cols, int ldo) {
  BNB_RANGE("cdequantize_int8_rows_t_bf16");
  return dequantize_int8_t<bf16_t>(reinterpret_cast<const int8_t*>(CB), SCB, out, rows, cols, ldo,
                                   "cdequantize_int8_rows_t_bf16");
}
int cdequantize_int8_rows_t_fp16(const signed char* CB, const float* SCB, fp16_t* out, int rows, int cols, int ldo) {
  BNB_RANGE("cdequantize_int8_rows_t_fp16");
  return dequantize_int8_t<fp16_t>(reinterpret_cast<const int8_t*>(CB), SCB, out, rows, cols, ldo,
                                   "cdequantize_int8_rows_t_fp16");
}

}  // extern "C"
