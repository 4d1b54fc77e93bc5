// Language-guided head of Point Prompt Training in eval ("PPT-v1m1", point_prompt_training_v1m1_language_guided.py:
// 98-107): seg_logits = exp(logit_scale) * normalize(W x + b) . E_v^T, with the D-wide projection collapsed away on the
// host (ptv3_hip.ops.ppt_head_collapse): W = Q R, so |W x + b|^2 = |R x + q|^2 + beta and
// (W x + b) . e_k = (M^T x + c)_k.  One (n, C) x (C, C + K) product with a row-norm epilogue; reads n x C, writes n x K.
//   ppt_head_kernel<KC>   C = 16 * KC.  A workgroup of 4 waves stages B = [R^T | M] transposed (a column's C values
//                         contiguous, rows padded to C + 4 floats; a thread takes a column, 16 loads in flight, coalesced
//                         across the threads) and the bias [q | c] in LDS once, then walks blocks of
//                         128 rows; a wave owns 2 x 16 rows, whose x fragments it loads from global memory straight in
//                         operand layout and keeps in registers over all column tiles.  First the C / 16 tiles of R: add
//                         q, square, sum in the accumulator layout, then across the 16 lanes of a row; then the K tiles:
//                         add c, scale by s / sqrt(sum + beta), store the K real columns.  Column tiles past the LDS
//                         budget (C >= 112 with more than 144 classes) take their B fragments from global memory.
// LDS reads are ds_read_b128 at (column * (C + 4) + k) floats: within one 16-lane group of that instruction the sixteen
// columns are distinct but the two k groups differ by one 16-byte slot, so one pair of lanes shares a slot (2-way on one
// slot of sixteen); not conflict-free, and not the limit - the fp32 matrix-core rate is.
// No atomics, no hand-off between workgroups: two runs are bitwise equal.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int PPT_THREADS = 256;
constexpr int PPT_WG_ROWS = 128;                 // 4 waves x 2 row tiles x 16 rows
constexpr int PPT_MAX_C = 128, PPT_MAX_K = 256;
constexpr int PPT_MAX_GRID = 512;
constexpr size_t PPT_MAX_LDS = 144 * 1024;

static inline int ppt_ktiles(int K) { return (K + 15) / 16; }
// column tiles of B kept in LDS: all of them, or as many as the budget holds (never fewer than the C / 16 of R)
static inline int ppt_lds_tiles(int C, int K) {
  const int nt = C / 16 + ppt_ktiles(K);
  const size_t per_tile = (size_t)16 * (C + 4) * sizeof(float);
  const size_t room = PPT_MAX_LDS - (size_t)nt * 16 * sizeof(float);
  const int fit = (int)(room / per_tile);
  return fit < nt ? fit : nt;
}
static inline size_t ppt_lds_bytes(int C, int K) {
  const int nt = C / 16 + ppt_ktiles(K);
  return ((size_t)ppt_lds_tiles(C, K) * 16 * (C + 4) + (size_t)nt * 16) * sizeof(float);
}

template <int KC>
__global__ __launch_bounds__(PPT_THREADS) void ppt_head_kernel(const float* __restrict__ x, const float* __restrict__ B,
                                                               const float* __restrict__ bias, float beta, float s,
                                                               int64_t n, int K, int lds_tiles, float* __restrict__ out) {
  constexpr int C = KC * 16, LD = C + 4;
  extern __shared__ float ppt_smem[];
  const int nb = C + K;                         // row length of B and of the bias
  const int nt = KC + (K + 15) / 16;            // column tiles in all
  float* sb = ppt_smem;                         // [lds_tiles * 16][LD]: column-major B
  float* sbias = ppt_smem + (size_t)lds_tiles * 16 * LD;   // [nt * 16]
  const int tid = threadIdx.x;
  const int ncol = lds_tiles * 16;
  // a thread stages whole columns: 16 independent loads (coalesced across the threads), then 64 contiguous LDS bytes
  for (int col = tid; col < ncol; col += PPT_THREADS) {
    const bool real = col < nb;
    const float* bp = B + (real ? col : 0);
    float* sp = sb + col * LD;
#pragma unroll 1
    for (int k0 = 0; k0 < C; k0 += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = bp[(size_t)(k0 + u) * nb];
#pragma unroll
      for (int u = 0; u < 16; ++u) sp[k0 + u] = real ? v[u] : 0.f;
    }
  }
  for (int col = tid; col < nt * 16; col += PPT_THREADS) sbias[col] = col < nb ? bias[col] : 0.f;
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  for (int64_t blk = blockIdx.x; blk * PPT_WG_ROWS < n; blk += gridDim.x) {
    const int64_t row0 = blk * PPT_WG_ROWS + wave * 32;
    if (row0 >= n) continue;                    // wave-uniform; no barrier below
    f32x4 a[2][KC];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int64_t row = row0 + rt * 16 + i;
      row = row < n ? row : n - 1;              // rows past the end repeat the last one and are never stored
      const f32x4* xp = reinterpret_cast<const f32x4*>(x + row * C + 4 * g);
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) a[rt][kc] = xp[kc * 4];
    }
    auto tile = [&](int t, f32x4& acc0, f32x4& acc1) {
      acc0 = acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < lds_tiles) {
        const f32x4* bp = reinterpret_cast<const f32x4*>(sb + (t * 16 + i) * LD + 4 * g);
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          const f32x4 b = bp[kc * 4];
          acc0 = mma16<float>(a[0][kc], b, acc0);
          acc1 = mma16<float>(a[1][kc], b, acc1);
        }
      } else {
        int col = t * 16 + i;
        col = col < nb ? col : nb - 1;          // padding columns repeat the last one and are never stored
        const float* bp = B + (size_t)(4 * g) * nb + col;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          const float* p = bp + (size_t)(kc * 16) * nb;
          const f32x4 b = {p[0], p[nb], p[2 * (size_t)nb], p[3 * (size_t)nb]};
          acc0 = mma16<float>(a[0][kc], b, acc0);
          acc1 = mma16<float>(a[1][kc], b, acc1);
        }
      }
    };
    // |R x + q|^2 of the rows 4g + r of both row tiles
    float ss[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
    for (int t = 0; t < KC; ++t) {
      f32x4 acc0, acc1;
      tile(t, acc0, acc1);
      const float q = sbias[t * 16 + i];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z0 = acc0[r] + q, z1 = acc1[r] + q;
        ss[0][r] = fmaf(z0, z0, ss[0][r]);
        ss[1][r] = fmaf(z1, z1, ss[1][r]);
      }
    }
    float sc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = ss[rt][r];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);   // the 16 lanes of a row share g
        sc[rt][r] = s / sqrtf(v + beta);          // no guard: a zero projection gives the reference's NaN
      }
#pragma unroll 1
    for (int t = KC; t < nt; ++t) {
      f32x4 acc0, acc1;
      tile(t, acc0, acc1);
      const int col = (t - KC) * 16 + i;
      const float c = sbias[t * 16 + i];
      if (col < K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t r0 = row0 + 4 * g + r, r1 = r0 + 16;
          if (r0 < n) out[r0 * K + col] = (acc0[r] + c) * sc[0][r];
          if (r1 < n) out[r1 * K + col] = (acc1[r] + c) * sc[1][r];
        }
      }
    }
  }
}

template <int KC>
static void ppt_launch(const float* x, const float* B, const float* bias, float beta, float s, int64_t n, int K,
                       float* out, hipStream_t stream) {
  const int C = KC * 16;
  const size_t lds = ppt_lds_bytes(C, K);
  int64_t grid = cdiv(n, PPT_WG_ROWS);
  if (grid > PPT_MAX_GRID) grid = PPT_MAX_GRID;
  ensure_dynamic_lds((const void*)ppt_head_kernel<KC>, (int)lds);
  hipLaunchKernelGGL(ppt_head_kernel<KC>, dim3((unsigned)grid), dim3(PPT_THREADS), lds, stream, x, B, bias, beta, s, n, K,
                     ppt_lds_tiles(C, K), out);
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_ppt_head_capable(int C, int K) {
  return C >= 16 && C <= PPT_MAX_C && C % 16 == 0 && K >= 1 && K <= PPT_MAX_K;
}

extern "C" int ptv3_ppt_head_fwd(const float* x, const float* B, const float* bias, float beta, float s, int64_t n, int C,
                                 int K, float* out, void* stream) {
  PTV3_REQUIRE(ptv3_ppt_head_capable(C, K),
               "ppt_head_fwd: C=%d, K=%d outside the limits (C a multiple of 16 in [16, 128], K in [1, 256])", C, K);
  PTV3_REQUIRE(n >= 0 && n < (1ll << 40), "ppt_head_fwd: n=%lld unsupported", (long long)n);
  PTV3_REQUIRE(B && bias && (n == 0 || (x && out)), "ppt_head_fwd: a pointer is NULL");
  PTV3_REQUIRE(((uintptr_t)x & 15) == 0, "ppt_head_fwd: x must be 16-byte aligned");
  if (n == 0) return PTV3_OK;
  hipStream_t st = (hipStream_t)stream;
  by_value<1, 2, 3, 4, 5, 6, 7, 8>(C / 16, [&](auto NT) { ppt_launch<NT()>(x, B, bias, beta, s, n, K, out, st); });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
