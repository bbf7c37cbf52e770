// Batched int8 GEMM whose operands are each K-contiguous or K-strided (cigemm / cbatched_igemm, int8.hip).
//
//   Out[b][r][c] = sum_k X_b(r, k) * Y_b(c, k)      int8 in, exact int32 out, row-major Out with ldc
//   K-contiguous (KS = false): element (r, k) at P[r * ld + k]
//   K-strided    (KS = true):  element (r, k) at P[k * ld + r]
//
// Geometry of k_igemm (int8.hip): 128 x 128 output tile per 256-thread workgroup (2 x 2 waves, 64 x 64 per wave,
// v_mfma_i32_16x16x64_i8), BK = 128, two LDS stages with register staging, one barrier per k-tile.  The LDS image
// is [128 rows][128 k-bytes] with the 16-B slots of a row XOR-swizzled; a lane reads 16 consecutive k of row
// (lane & 15), chunk (lane >> 4), with ds_read_b128 -- the same k for X and Y, so the sum is exact whatever the
// instruction's internal k order.
//
// A K-strided operand is loaded 16 B along the row index, one k per load (coalesced: 8 lanes cover 128 B of one k),
// four consecutive k per thread; the 4 x 16 bytes are transposed in registers, 4 x 4 byte blocks on v_perm_b32
// (8 per block), and written as 16 dwords: row r, k-bytes 4q .. 4q+3.  So the image, and the whole MFMA phase, is the
// same for both kinds of operand.  The swizzle term (row >> 4) & 7 is what keeps those dword stores conflict-free:
// the 32 lanes of a store group hold 8 row groups x 4 k-quads of one row-in-group, and without it the 8 row groups
// would land on the same 4 banks.  It is constant over the 16 rows a ds_read_b128 group touches and over the rows of
// a K-contiguous ds_write_b128 group, so those accesses keep the conflict-free pattern of k_igemm's image.
//
// An operand whose base or ld is not a multiple of 16 B is read through load16_any: two aligned 16-B loads and a funnel
// shift per 16 bytes.  Units (a thread's 16 B x 4) that are ragged -- partly outside rows/K -- are fetched bytewise with
// guards and zero fill; units wholly outside are zeros without a load.
#include "int8_common.hpp"

namespace bnb {

typedef __attribute__((ext_vector_type(4))) int i32x4s_t;

constexpr int S_BM = 128, S_BN = 128, S_BK = 128, S_THREADS = 256;
constexpr int S_TILE = S_BM * S_BK;   // 16 KiB

// byte offset of 16-B slot s (0..7) of row r (0..127)
__device__ __forceinline__ int sswz(int r, int s) { return r * 128 + ((s ^ (r & 7) ^ ((r >> 4) & 7)) << 4); }

// 16 bytes from any byte address, all 16 inside the operand: the two 16-B aligned granules that hold them are loaded
// whole and funnel-shifted (the second only when the address is not aligned).  A granule read this way holds at least
// one byte of the operand, so the load stays inside the operand's first / last 16-B aligned granule -- it never
// touches another page -- and the bytes outside the operand are shifted out, never used.
__device__ __forceinline__ uint4 load16_any(const int8_t* a) {
  const uint32_t mis = (uint32_t)((uintptr_t)a & 15);
  const uint4 lo = *reinterpret_cast<const uint4*>(a - mis);
  uint4 hi = make_uint4(0, 0, 0, 0);
  if (mis) hi = *reinterpret_cast<const uint4*>(a - mis + 16);
  // dword shift by selects on named values (arrays here end up indexed through scratch), then the byte shift
  const bool s2 = mis & 8, s1 = mis & 4;
  const uint32_t v0 = s2 ? lo.z : lo.x, v1 = s2 ? lo.w : lo.y, v2 = s2 ? hi.x : lo.z, v3 = s2 ? hi.y : lo.w,
                 v4 = s2 ? hi.z : hi.x, v5 = s2 ? hi.w : hi.y;
  const uint32_t u0 = s1 ? v1 : v0, u1 = s1 ? v2 : v1, u2 = s1 ? v3 : v2, u3 = s1 ? v4 : v3, u4 = s1 ? v5 : v4;
  const uint32_t sh = 8 * (mis & 3);
  return make_uint4((uint32_t)((((uint64_t)u1 << 32) | u0) >> sh), (uint32_t)((((uint64_t)u2 << 32) | u1) >> sh),
                    (uint32_t)((((uint64_t)u3 << 32) | u2) >> sh), (uint32_t)((((uint64_t)u4 << 32) | u3) >> sh));
}

// ---- K-contiguous: thread t -> row t>>1, k-half (t&1)*64, 4 x 16 B (k_igemm's load_tile, with row / alignment guards)
__device__ __forceinline__ void load_kc(const int8_t* __restrict__ P, long long ld, bool al, int row0, int nrows, int k0,
                                        int K, uint4 (&v)[4]) {
  const int tr = threadIdx.x >> 1, th = threadIdx.x & 1;
  const int r = row0 + tr;
  const int8_t* p = P + (long long)r * ld;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = k0 + 64 * th + 16 * s;
    if (r >= nrows || k >= K) {
      v[s] = make_uint4(0, 0, 0, 0);
    } else if (al && k + 16 <= K) {
      v[s] = *reinterpret_cast<const uint4*>(p + k);
    } else if (k + 16 <= K) {
      v[s] = load16_any(p + k);
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (k + b < K) w[b >> 2] |= (uint32_t)(uint8_t)p[k + b] << (8 * (b & 3));
      v[s] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

__device__ __forceinline__ void store_kc(uint8_t* lds, const uint4 (&v)[4]) {
  const int tr = threadIdx.x >> 1, th = threadIdx.x & 1;
#pragma unroll
  for (int s = 0; s < 4; ++s) *reinterpret_cast<uint4*>(lds + sswz(tr, 4 * th + s)) = v[s];
}

// ---- K-strided: thread t -> rows 16*(t&7) .. +15, k = 4*(t>>3) .. +3; v[j] = the 16 rows at k + j
__device__ __forceinline__ void load_ks(const int8_t* __restrict__ P, long long ld, bool al, int row0, int nrows, int k0,
                                        int K, uint4 (&v)[4]) {
  const int r = row0 + 16 * (threadIdx.x & 7);
  const int k = k0 + 4 * (threadIdx.x >> 3);
  if (r >= nrows || k >= K) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = make_uint4(0, 0, 0, 0);
  } else if (al && r + 16 <= nrows && k + 4 <= K) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const uint4*>(P + (long long)(k + j) * ld + r);
  } else if (r + 16 <= nrows && k + 4 <= K) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = load16_any(P + (long long)(k + j) * ld + r);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t w[4] = {0, 0, 0, 0};
      if (k + j < K) {
        const int8_t* p = P + (long long)(k + j) * ld + r;
#pragma unroll
        for (int b = 0; b < 16; ++b)
          if (r + b < nrows) w[b >> 2] |= (uint32_t)(uint8_t)p[b] << (8 * (b & 3));
      }
      v[j] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

// 4 x 4 byte transpose: in w[j] = bytes (row 0..3) at k j; out o[b] = bytes (k 0..3) of row b.
// v_perm_b32 D = bytes of {S0, S1} picked by the selector: 0..3 = bytes of S1, 4..7 = bytes of S0.
__device__ __forceinline__ void transpose4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&o)[4]) {
  const uint32_t t01l = __builtin_amdgcn_perm(w1, w0, 0x05010400u);   // w0.b0 w1.b0 w0.b1 w1.b1
  const uint32_t t01h = __builtin_amdgcn_perm(w1, w0, 0x07030602u);   // w0.b2 w1.b2 w0.b3 w1.b3
  const uint32_t t23l = __builtin_amdgcn_perm(w3, w2, 0x05010400u);
  const uint32_t t23h = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
  o[0] = __builtin_amdgcn_perm(t23l, t01l, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(t23l, t01l, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(t23h, t01h, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(t23h, t01h, 0x07060302u);
}

__device__ __forceinline__ void store_ks(uint8_t* lds, const uint4 (&v)[4]) {
  const int rg = 16 * (threadIdx.x & 7), kq = threadIdx.x >> 3;
  const uint32_t w[4][4] = {{v[0].x, v[0].y, v[0].z, v[0].w},
                            {v[1].x, v[1].y, v[1].z, v[1].w},
                            {v[2].x, v[2].y, v[2].z, v[2].w},
                            {v[3].x, v[3].y, v[3].z, v[3].w}};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t o[4];
    transpose4(w[0][d], w[1][d], w[2][d], w[3][d], o);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      *reinterpret_cast<uint32_t*>(lds + sswz(rg + 4 * d + b, kq >> 2) + 4 * (kq & 3)) = o[b];
  }
}

template <bool KS>
__device__ __forceinline__ void load_op(const int8_t* __restrict__ P, long long ld, bool al, int row0, int nrows, int k0,
                                        int K, uint4 (&v)[4]) {
  if constexpr (KS) load_ks(P, ld, al, row0, nrows, k0, K, v);
  else load_kc(P, ld, al, row0, nrows, k0, K, v);
}
template <bool KS>
__device__ __forceinline__ void store_op(uint8_t* lds, const uint4 (&v)[4]) {
  if constexpr (KS) store_ks(lds, v);
  else store_kc(lds, v);
}

// X: R rows, Y: Cn rows, K deep.  grid = (tiles, batches)
template <bool XKS, bool YKS>
__global__ void __launch_bounds__(S_THREADS, 2)
k_igemm_strided(int R, int Cn, int K, const int8_t* __restrict__ X, const int8_t* __restrict__ Y,
                int32_t* __restrict__ Out, long long ldx, long long ldy, long long ldc, long long sx, long long sy,
                long long sc) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[4 * S_TILE];
  uint8_t* Xs = smem;
  uint8_t* Ys = smem + 2 * S_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  X += (long long)blockIdx.y * sx;
  Y += (long long)blockIdx.y * sy;
  Out += (long long)blockIdx.y * sc;
  const bool alx = (((uintptr_t)X | (uintptr_t)ldx) & 15) == 0;
  const bool aly = (((uintptr_t)Y | (uintptr_t)ldy) & 15) == 0;

  // XCD-aware tile order, groups of 8 row tiles (as k_igemm)
  const int tilesC = (Cn + S_BN - 1) / S_BN, tilesR = (R + S_BM - 1) / S_BM;
  const int nwg = tilesC * tilesR;
  int wg = blockIdx.x;
  {
    const int xcd = wg & 7, q = nwg >> 3, r = nwg & 7;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wg >> 3);
  }
  constexpr int GROUP = 8;
  const int group_span = GROUP * tilesC;
  const int first_r = (wg / group_span) * GROUP;
  const int gsize = min(tilesR - first_r, GROUP);
  const int tr = first_r + (wg % group_span) % gsize;
  const int tc = (wg % group_span) / gsize;
  const int r0 = tr * S_BM, c0 = tc * S_BN;

  const int wm = wave >> 1, wn = wave & 1;
  i32x4s_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = i32x4s_t{0, 0, 0, 0};

  const int nk = (K + S_BK - 1) / S_BK;
  uint4 rx[4], ry[4];
  load_op<XKS>(X, ldx, alx, r0, R, 0, K, rx);
  load_op<YKS>(Y, ldy, aly, c0, Cn, 0, K, ry);
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    uint8_t* xs = Xs + cur * S_TILE;
    uint8_t* ys = Ys + cur * S_TILE;
    store_op<XKS>(xs, rx);
    store_op<YKS>(ys, ry);
    __syncthreads();
    if (t + 1 < nk) {
      load_op<XKS>(X, ldx, alx, r0, R, (t + 1) * S_BK, K, rx);
      load_op<YKS>(Y, ldy, aly, c0, Cn, (t + 1) * S_BK, K, ry);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 a[4], b[4];
      const int slot = 4 * ks + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const uint4*>(xs + sswz(64 * wm + 16 * i + (lane & 15), slot));
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const uint4*>(ys + sswz(64 * wn + 16 * j + (lane & 15), slot));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4s_t, a[i]),
                                                            __builtin_bit_cast(i32x4s_t, b[j]), acc[i][j], 0, 0, 0);
    }
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 64 * wm + 16 * i + 4 * (lane >> 4) + r;
      if (row >= R) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = c0 + 64 * wn + 16 * j + (lane & 15);
        if (col < Cn) Out[(long long)row * ldc + col] = acc[i][j][r];
      }
    }
  }
}

template <bool XKS, bool YKS>
static void launch_one(int R, int Cn, int K, const int8_t* X, const int8_t* Y, int32_t* Out, long long ldx,
                       long long ldy, long long ldc, long long sx, long long sy, long long sc, int batch) {
  const unsigned tiles = (unsigned)(((R + S_BM - 1) / S_BM) * ((Cn + S_BN - 1) / S_BN));
  // the batch index is grid.y (at most 65535 per launch)
  for (int b0 = 0; b0 < batch; b0 += 65535) {
    const int nb = min(batch - b0, 65535);
    hipLaunchKernelGGL((k_igemm_strided<XKS, YKS>), dim3(tiles, (unsigned)nb), dim3(S_THREADS), 0, current_stream(), R, Cn,
                       K, X + b0 * sx, Y + b0 * sy, Out + b0 * sc, ldx, ldy, ldc, sx, sy, sc);
  }
}

int launch_igemm_strided(bool x_kstrided, bool y_kstrided, int R, int Cn, int K, const int8_t* X, const int8_t* Y,
                         int32_t* Out, long long ldx, long long ldy, long long ldc, long long sx, long long sy,
                         long long sc, int batch) {
  if (R <= 0 || Cn <= 0 || K <= 0 || batch <= 0) return 0;
  if (ldx < (x_kstrided ? R : K) || ldy < (y_kstrided ? Cn : K) || ldc < Cn) {
    set_error((int)hipErrorInvalidValue, "igemm: leading dimension smaller than the matrix extent");
    return 1;
  }
  if (x_kstrided) {
    if (y_kstrided) launch_one<true, true>(R, Cn, K, X, Y, Out, ldx, ldy, ldc, sx, sy, sc, batch);
    else launch_one<true, false>(R, Cn, K, X, Y, Out, ldx, ldy, ldc, sx, sy, sc, batch);
  } else {
    if (y_kstrided) launch_one<false, true>(R, Cn, K, X, Y, Out, ldx, ldy, ldc, sx, sy, sc, batch);
    else launch_one<false, false>(R, Cn, K, X, Y, Out, ldx, ldy, ldc, sx, sy, sc, batch);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error((int)e, "igemm launch"); return 1; }
  return 0;
}

}  // namespace bnb
