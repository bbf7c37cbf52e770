// Transposing 4-bit dequantise for gfx950: packed NF4 / FP4 weight of logical shape [N, K] -> out[k * ldo + n] in
// bf16 / fp16, the W^T [K, N] operand image of the input-gradient product grad[M, N] @ W[N, K] (chgemm_tn_* with
// m = rows, n = K, k = N).  [additive] cdequantize_blockwise_t_* / cdequantize_blockwise_nested_t_*.
//
// Values: fp32 code4_value(q) * absmax (one __fmul_rn), then one RNE cast -- the bits of k_dequantize_4bit_stream
// (quant.hip), so the result equals dequantize_4bit(...).t().contiguous() bit for bit.  The packing is flat: element
// e = n * K + k sits in byte e / 2 (high nibble = even element), its statistics block is e >> bs_shift; blocks may
// straddle rows (K % blocksize != 0) or span several (blocksize > K), nothing here assumes a block lies inside a row.
// Nested statistics are decoded in the kernel: absmax = code2[q8[b]] * absmax2[b >> bs2_shift] + offset in fp32.
//
// Shape: one workgroup (256 lanes) owns a 64 (n) x 128 (k) tile.
//   load     lane (rp, kd) = (t >> 4, t & 15) reads the packed dword kd (8 weights along k) of rows 2 rp, 2 rp + 1 and
//            of rows 2 (rp + 16), 2 (rp + 16) + 1: each load instruction reads 64 contiguous bytes of 4 rows; all four
//            loads and their statistics are issued before any is consumed (non-temporal, as the stream kernel);
//   decode   through the 256-entry byte -> (hi, lo) pair table in LDS, as the stream kernel;
//   LDS      the tile is stored k-major, 64 16-bit values = 32 dwords per k row, no padding.  A lane packs the values
//            of its two rows (n, n + 1) at one k into one 32-bit write.  The 8-byte units (4 n's) of row k are placed
//            at unit ^ ((k >> 3) & 15): the 16 kd's of a 32-lane write group then hit 16 different units, two dwords
//            each -- 32 different banks, conflict-free under the (a / 4) mod 32 rule of ds_write_b32;
//   read-out lane (kr, c) = (t >> 3, t & 7) reads the 16-B chunk c of row k: the XOR keeps the two units of a chunk
//            in one aligned 16-B chunk, c ^ (s >> 1), with its halves swapped when s is odd; one ds_read_b128;
//   store    one 16-B store per lane, 8 lanes = one 128-B run of an output row; device-scope write-through through a
//            buffer resource (the stream kernel's default policy for the dequantised weight), 32-bit byte offsets.
// Ragged tiles: load addresses are clamped to the last packed dword (never past N * K / 2 bytes), stores are masked to
// columns [0, N) of rows [0, K).  No atomics.
#include "common.hpp"

namespace bnb {

struct DqtNested {
  const uint8_t* q8;
  const float* code2;
  const float* absmax2;
  const float* offset;
  int bs2_shift;
};

typedef uint32_t dqt_u32x4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ uint32_t dqt_bits(float v) {
  return (uint32_t)__builtin_bit_cast(uint16_t, Io<T>::from_f32(v));
}

constexpr int DQT_TN = 64, DQT_TK = 128;

template <typename T, int DT, bool NESTED>
__global__ void __launch_bounds__(256)
k_dequantize_4bit_t(const uint8_t* __restrict__ A, const float* __restrict__ absmax, T* __restrict__ out, int bs_shift,
                    int N, int K, int ldo, int n_tiles, DqtNested ns) {
  __shared__ float2 s_pair[256];
  __shared__ float s_code2[NESTED ? 256 : 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_tile[DQT_TK * DQT_TN / 2];
  constexpr int TN = DQT_TN;
  const int t = threadIdx.x;
  s_pair[t] = make_float2(code4_value<DT>((uint32_t)t >> 4), code4_value<DT>((uint32_t)t & 15));
  float off = 0.0f;
  if constexpr (NESTED) {
    s_code2[t] = ns.code2[t];
    off = *ns.offset;
  }
  // n tiles run fastest: workgroups in flight together fill whole output rows
  const int n0 = (int)(blockIdx.x % (unsigned)n_tiles) * TN;
  const int k0 = (int)(blockIdx.x / (unsigned)n_tiles) * DQT_TK;
  const long long ndw = ((long long)N * K) >> 3;
  const uint32_t* Aw = reinterpret_cast<const uint32_t*>(A);
  const int kd = t & 15, rp = t >> 4;

  constexpr int P = TN / 16;                         // packed dwords per lane: TN / 32 row pairs
  uint32_t w[P];
  float am[P];                                       // NESTED: the second-level scale until the tables are in LDS
  uint32_t qc[NESTED ? P : 1];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int n = n0 + 2 * (rp + 16 * (j >> 1)) + (j & 1);
    // rows past N and dwords past K land on (or are clamped to) packed dwords inside the weight; never stored
    const long long d = min(((long long)n * K + k0 + 8 * kd) >> 3, ndw - 1);
    w[j] = __builtin_nontemporal_load(Aw + d);
    const long long blk = (8 * d) >> bs_shift;
    if constexpr (NESTED) {
      qc[j] = ns.q8[blk];
      am[j] = ns.absmax2[blk >> ns.bs2_shift];
    } else {
      am[j] = absmax[blk];
    }
  }
  __syncthreads();
  if constexpr (NESTED) {
#pragma unroll
    for (int j = 0; j < P; ++j) am[j] = __fadd_rn(__fmul_rn(s_code2[qc[j]], am[j]), off);
  }

  // decode: rows (n, n + 1) of one k pack into one dword of the k-major tile
  const int s = kd;                                  // ((8 kd + i) >> 3) & 15
#pragma unroll
  for (int it = 0; it < P / 2; ++it) {
    const int nl = 2 * (rp + 16 * it);               // even local n of the pair
    const int col = ((((nl >> 2) ^ s) << 1) | ((nl >> 1) & 1));
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float2 p0 = s_pair[(w[2 * it] >> (8 * b)) & 0xFF];
      const float2 p1 = s_pair[(w[2 * it + 1] >> (8 * b)) & 0xFF];
      const uint32_t e0 = dqt_bits<T>(__fmul_rn(p0.x, am[2 * it])) | (dqt_bits<T>(__fmul_rn(p1.x, am[2 * it + 1])) << 16);
      const uint32_t e1 = dqt_bits<T>(__fmul_rn(p0.y, am[2 * it])) | (dqt_bits<T>(__fmul_rn(p1.y, am[2 * it + 1])) << 16);
      s_tile[(8 * kd + 2 * b) * (TN / 2) + col] = e0;
      s_tile[(8 * kd + 2 * b + 1) * (TN / 2) + col] = e1;
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
  for (int p = 0; p < DQT_TK / RPP; ++p) {
    const int kl = RPP * p + t / CH;
    const int sk = (kl >> 3) & 15;
    const uint4 v = reinterpret_cast<const uint4*>(s_tile)[kl * CH + (c ^ (sk >> 1))];
    const dqt_u32x4 o = (sk & 1) ? (dqt_u32x4){v.z, v.w, v.x, v.y} : (dqt_u32x4){v.x, v.y, v.z, v.w};
    const int k = k0 + kl;
    if (k < K && n < N)
      __builtin_amdgcn_raw_buffer_store_b128(o, r, (int)(((long long)k * ldo + n) * 2), 0, 16);
  }
}

static inline bool dqt_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// 0 launched (or nothing to do), 1 shape / alignment / blocksize not supported (nothing launched), 2 launch error
template <typename T, int DT, bool NESTED>
static int dequantize_4bit_t(const uint8_t* A, const float* absmax, const DqtNested& ns, T* out, int blocksize, int rows,
                             int cols, int ldo, const char* name) {
  const int N = rows, K = cols;
  if (N < 0 || K < 0) return 1;
  if (N == 0 || K == 0) return 0;
  if (blocksize < 64 || !dqt_pow2(blocksize)) return 1;
  if (N % 8 || K % 8 || ldo < N || ldo % 8) return 1;
  if (((uintptr_t)A & 3) || ((uintptr_t)out & 15)) return 1;
  // every output byte offset is a 32-bit buffer offset below 2 GiB
  if (((long long)(K - 1) * ldo + N) * 2 > 0x7FFFFFFFLL) return 1;
  const int n_tiles = (N + DQT_TN - 1) / DQT_TN;
  const long long tiles = (long long)n_tiles * ((K + DQT_TK - 1) / DQT_TK);
  if (tiles > 0x7FFFFFFFLL) return 1;
  hipLaunchKernelGGL((k_dequantize_4bit_t<T, DT, NESTED>), dim3((unsigned)tiles), dim3(256), 0, current_stream(), A,
                     absmax, out, __builtin_ctz(blocksize), N, K, ldo, n_tiles, ns);
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

#define BNB_DEQUANT_T_ABI(fname, T, DT)                                                                        \
  int fname(unsigned char* A, float* absmax, T* out, int blocksize, int rows, int cols, int ldo) {             \
    BNB_RANGE(#fname);                                                                                          \
    return dequantize_4bit_t<T, DT, false>(A, absmax, DqtNested{}, out, blocksize, rows, cols, ldo, #fname);    \
  }
BNB_DEQUANT_T_ABI(cdequantize_blockwise_t_bf16_nf4, bf16_t, NF4)
BNB_DEQUANT_T_ABI(cdequantize_blockwise_t_bf16_fp4, bf16_t, FP4)
BNB_DEQUANT_T_ABI(cdequantize_blockwise_t_fp16_nf4, fp16_t, NF4)
BNB_DEQUANT_T_ABI(cdequantize_blockwise_t_fp16_fp4, fp16_t, FP4)

#define BNB_DEQUANT_NESTED_T_ABI(fname, T, DT)                                                                  \
  int fname(unsigned char* A, unsigned char* absmax_q, float* code2, float* absmax2, float* offset, T* out,      \
            int blocksize, int blocksize2, int rows, int cols, int ldo) {                                        \
    BNB_RANGE(#fname);                                                                                            \
    if (!dqt_pow2(blocksize2)) return 1;                                                                          \
    const DqtNested ns{absmax_q, code2, absmax2, offset, __builtin_ctz(blocksize2)};                              \
    return dequantize_4bit_t<T, DT, true>(A, nullptr, ns, out, blocksize, rows, cols, ldo, #fname);               \
  }
BNB_DEQUANT_NESTED_T_ABI(cdequantize_blockwise_nested_t_bf16_nf4, bf16_t, NF4)
BNB_DEQUANT_NESTED_T_ABI(cdequantize_blockwise_nested_t_bf16_fp4, bf16_t, FP4)
BNB_DEQUANT_NESTED_T_ABI(cdequantize_blockwise_nested_t_fp16_nf4, fp16_t, NF4)
BNB_DEQUANT_NESTED_T_ABI(cdequantize_blockwise_nested_t_fp16_fp4, fp16_t, FP4)

}  // extern "C"
