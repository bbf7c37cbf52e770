// What the int8 decode kernels share (igemv8.hip, igemv8_outlier.hip): the workgroup geometry, the 16-B buffer loads of
// the weight stream and the activations, the in-register activation quantisation and the host's coverage predicate.
#pragma once

#include "int8_common.hpp"

namespace bnb {

typedef __attribute__((ext_vector_type(4))) int gv_i32x4_t;

constexpr int GV_WAVES = 8;
constexpr int GV_THREADS = 64 * GV_WAVES;
constexpr int GV_ROWS = 16;              // weight rows per workgroup
constexpr int GV_STEP = 256;             // k per wave step: 4 MFMAs of 64
constexpr int GV_MAX_M = 32;             // activation rows covered
constexpr uint32_t GV_OOB = 0x80000000u; // buffer offset beyond any resource here: the load returns zeros

__device__ __forceinline__ uint4 gv_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
// the weight stream: read once, non-temporal (aux 2 = nt on gfx950)
__device__ __forceinline__ uint4 gv_load16_nt(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 2);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// four fp16 (two dwords) -> four int8 in one dword, k_row_quant's expressions
__device__ __forceinline__ uint32_t gv_quant4(uint32_t w0, uint32_t w1, float rsc) {
  const uint32_t w[2] = {w0, w1};
  uint32_t q = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = (float)__builtin_bit_cast(fp16_t, (uint16_t)(w[j >> 1] >> (16 * (j & 1))));
    q |= (uint32_t)(uint8_t)rint_i8(__fmul_rn(a, rsc)) << (8 * j);
  }
  return q;
}

// what the kernels cover, from the call's numbers alone (m, n, k > 0 here)
static inline bool igemv8_covers(int m, int k, const void* A, const void* B, long long lda, long long ldb,
                                 long long ldc, int n, int a_bytes) {
  if (m > GV_MAX_M || k % 16 != 0 || n >= (1 << 28)) return false;
  if (lda < k || ldb < k || ldc < n) return false;
  if ((((uintptr_t)A | (uintptr_t)B) & 15) != 0 || (lda * a_bytes) % 16 != 0 || ldb % 16 != 0) return false;
  // 32-bit buffer offsets with the top bit free for GV_OOB
  if ((long long)GV_ROWS * ldb >= (1LL << 31) || (long long)GV_MAX_M * lda * a_bytes >= (1LL << 31)) return false;
  return true;
}

// cigemv_set_mode's current value (igemv8.hip): 0 = auto, 1 = wherever covered, -1 = never
int igemv_mode();

}  // namespace bnb
