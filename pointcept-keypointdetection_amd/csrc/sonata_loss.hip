// Self-distillation loss of "Sonata-v1m1" (sonata_v1m1_base.py: sinkhorn_knopp :267-291 and the cross entropy
// :443-454) without the (M, K) matrices.  With E = exp(x / T) the Sinkhorn-Knopp assignment is a column scaling
// followed by a row normalisation: target[m, k] = E[m, k] u[k] / d[m], d[m] = sum_k E[m, k] u[k],
// and u comes out of three sweeps over the teacher logits that each end in a K-vector.
//   sn_sk_partial_kernel   a workgroup per SN_ROWS matched pairs, a wavefront per row: the gathered teacher row is read
//                          once into registers (64 lanes x KPL entries, pairs of columns per lane when K is even),
//                          d[m] reduced over the wavefront, the weighted row added to per-lane float64 column
//                          accumulators; the four wavefronts are added in order through LDS and the chunk's K sums
//                          stored as fp32 in the slab
//   sn_sk_finish_kernel    A[k] = the chunks in increasing order in float64 (four runs of chunks side by side, added
//                          in order), and u = 1 / (K A) when nothing has to be reduced across ranks
//   sn_ce_fwd_kernel       a wavefront per pair: d, logsumexp(s / tau) and -sum_k target (s / tau - lse), in float64
//   sn_ce_finish_kernel    one workgroup: per-scene means in scene order, their mean, and the backward's 1 / (count B)
//   sn_ce_bwd_kernel       a wavefront per student row: zeros for a row without a pair (binary search in idx_s), else
//                          g (softmax(s / tau) sum_k target - target) / tau with the target recomputed
// exp(x / T) is taken without a shift as the reference does: the logits are cosines and T >= 0.04, so |x / T| <= 25.
// The argument x * (1 / T) is formed as a two-float product (1 / T split into hi + lo on the host), which leaves expf's
// own rounding as the only error of E.  No atomics: every hand-off is a kernel boundary, two runs are bitwise equal.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int SN_THREADS = 256;
constexpr int SN_WAVES = SN_THREADS / 64;
constexpr int SN_ROWS = 64;                     // matched pairs per workgroup of a Sinkhorn sweep
constexpr int SN_MAX_K = 4096;
constexpr int SN_FIN_COLS = 64;                 // columns per workgroup of the slab sum
constexpr int SN_MAX_SCENES = 4096;

__device__ __forceinline__ double sn_wsum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float sn_wmax(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// x * (hi + lo) as a + r with a = fl(x * hi) and r the rest (|r| <= ulp(a) / 2 + |x lo|)
__device__ __forceinline__ void sn_arg(float x, float hi, float lo, float* a, float* r) {
  const float p = x * hi;
  *a = p;
  *r = fmaf(x, lo, fmaf(x, hi, -p));
}
__device__ __forceinline__ float sn_exp(float x, float hi, float lo) {
  float a, r;
  sn_arg(x, hi, lo, &a, &r);
  const float e = expf(a);
  return fmaf(e, r, e);
}

__device__ __forceinline__ int64_t sn_index(const void* __restrict__ idx, int is32, int64_t m, int64_t rows) {
  int64_t v = is32 ? (int64_t)((const int32_t*)idx)[m] : ((const int64_t*)idx)[m];
  v = v < 0 ? 0 : v;
  return v < rows ? v : rows - 1;                // an index outside the matrix reads its last row, never past it
}

// Which column a lane's j-th register holds.  `vec` (K even and every matrix and vector of the launch starting on a pair
// boundary, sn_pairs_ok): lanes take PAIRS of neighbouring columns, so that a row is read with 4-byte (bf16) or 8-byte
// (fp32) loads - every row of an even K then starts on such a boundary; otherwise one column each.
__device__ __forceinline__ int sn_k(int j, int lane, bool vec) {
  return vec ? ((((j >> 1) << 6) + lane) << 1) + (j & 1) : (j << 6) + lane;
}

// a pointer through which pairs of T may be read at once (NULL counts as one); a view that starts on an odd element of its
// storage is not, and the kernel then takes one column per load
template <typename T>
__device__ __forceinline__ bool sn_pairs_ok(const T* p) { return ((uintptr_t)p & (2 * sizeof(T) - 1)) == 0; }

// v[j] = row[sn_k(j)], 0 from K on
template <int KPL>
__device__ __forceinline__ void sn_load(const float* __restrict__ row, int K, int lane, bool vec, float (&v)[KPL]) {
  if (vec) {
#pragma unroll
    for (int jj = 0; jj < KPL / 2; ++jj) {
      const int p = jj * 64 + lane;
      const f32x2 w = 2 * p < K ? ((const f32x2*)row)[p] : f32x2{0.f, 0.f};
      v[2 * jj] = w[0];
      v[2 * jj + 1] = w[1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = j * 64 + lane;
      v[j] = k < K ? row[k] : 0.f;
    }
  }
}
template <int KPL>
__device__ __forceinline__ void sn_load(const __bf16* __restrict__ row, int K, int lane, bool vec, float (&v)[KPL]) {
  if (vec) {
#pragma unroll
    for (int jj = 0; jj < KPL / 2; ++jj) {
      const int p = jj * 64 + lane;
      const unsigned w = 2 * p < K ? ((const unsigned*)row)[p] : 0u;
      v[2 * jj] = __builtin_bit_cast(float, w << 16);
      v[2 * jj + 1] = __builtin_bit_cast(float, w & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = j * 64 + lane;
      v[j] = k < K ? (float)row[k] : 0.f;
    }
  }
}

// row[sn_k(j)] = v[j] below K
template <int KPL>
__device__ __forceinline__ void sn_store(float* __restrict__ row, int K, int lane, bool vec, const float (&v)[KPL]) {
  if (vec) {
#pragma unroll
    for (int jj = 0; jj < KPL / 2; ++jj) {
      const int p = jj * 64 + lane;
      if (2 * p < K) ((f32x2*)row)[p] = f32x2{v[2 * jj], v[2 * jj + 1]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = j * 64 + lane;
      if (k < K) row[k] = v[j];
    }
  }
}
template <int KPL>
__device__ __forceinline__ void sn_store(__bf16* __restrict__ row, int K, int lane, bool vec, const float (&v)[KPL]) {
  if (vec) {
#pragma unroll
    for (int jj = 0; jj < KPL / 2; ++jj) {
      const int p = jj * 64 + lane;
      const bf16x2 w = __builtin_convertvector(f32x2{v[2 * jj], v[2 * jj + 1]}, bf16x2);
      if (2 * p < K) ((unsigned*)row)[p] = __builtin_bit_cast(unsigned, w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = j * 64 + lane;
      if (k < K) row[k] = (__bf16)v[j];
    }
  }
}

// this lane's part of sum_k e[k] u[k], u read as it is used: it stays in the cache, while the sweep's accumulators and
// the row fill the registers (e is 0 from K on)
template <int KPL>
__device__ __forceinline__ double sn_dot_u(const float* __restrict__ u, int K, int lane, bool vec, const float (&e)[KPL]) {
  double dl = 0.0;
  if (vec) {
#pragma unroll
    for (int jj = 0; jj < KPL / 2; ++jj) {
      const int p = jj * 64 + lane;
      const f32x2 w = 2 * p < K ? ((const f32x2*)u)[p] : f32x2{0.f, 0.f};
      dl += (double)e[2 * jj] * (double)w[0];
      dl += (double)e[2 * jj + 1] * (double)w[1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int k = j * 64 + lane;
      dl += (double)e[j] * (double)(k < K ? u[k] : 0.f);
    }
  }
  return dl;
}

// e[j] = exp(x[row, sn_k(j)] / T), 0 from K on
template <typename T, int KPL>
__device__ __forceinline__ void sn_exp_row(const T* __restrict__ xr, int K, int lane, bool vec, float hi, float lo,
                                           float (&e)[KPL]) {
  float raw[KPL];
  sn_load<KPL>(xr, K, lane, vec, raw);
#pragma unroll
  for (int j = 0; j < KPL; ++j) e[j] = sn_k(j, lane, vec) < K ? sn_exp(raw[j], hi, lo) : 0.f;
}

template <typename T, int KPL>
__global__ void __launch_bounds__(SN_THREADS) sn_sk_partial_kernel(
    const T* __restrict__ x, const void* __restrict__ idx_t, int idx32, int64_t nt, int64_t M, int K, float hi, float lo,
    const float* __restrict__ u, double inv_n, float* __restrict__ slab) {
  __shared__ double comb[64 * KPL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool vec = (K & 1) == 0 && sn_pairs_ok(x) && sn_pairs_ok(u);
  const int64_t r0 = (int64_t)blockIdx.x * SN_ROWS;
  const int cnt = (int)(M - r0 < SN_ROWS ? M - r0 : SN_ROWS);
  double acc[KPL];
#pragma unroll
  for (int j = 0; j < KPL; ++j) acc[j] = 0.0;
  for (int i = wave; i < cnt; i += SN_WAVES) {
    const int64_t src = sn_index(idx_t, idx32, r0 + i, nt);
    float e[KPL];
    sn_exp_row<T, KPL>(x + src * K, K, lane, vec, hi, lo, e);
    double w = 1.0;
    if (u != nullptr) {
      w = inv_n / sn_wsum(sn_dot_u<KPL>(u, K, lane, vec, e));
    }
#pragma unroll
    for (int j = 0; j < KPL; ++j) acc[j] += (double)e[j] * w;
  }
  for (int wv = 0; wv < SN_WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int j = 0; j < KPL; ++j) {
        const int k = sn_k(j, lane, vec);
        if (k < K) comb[k] = wv == 0 ? acc[j] : comb[k] + acc[j];
      }
    }
    __syncthreads();
  }
  for (int k = tid; k < K; k += SN_THREADS) slab[(int64_t)blockIdx.x * K + k] = (float)comb[k];
}

__global__ void __launch_bounds__(SN_THREADS) sn_sk_finish_kernel(const float* __restrict__ slab, int64_t chunks, int K,
                                                                 float* __restrict__ A, float* __restrict__ u_next) {
  __shared__ double part[SN_WAVES][SN_FIN_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * SN_FIN_COLS + lane;
  const int64_t per = (chunks + SN_WAVES - 1) / SN_WAVES;
  const int64_t c0 = wave * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  double s = 0.0;
  if (k < K) {
#pragma unroll 8
    for (int64_t c = c0; c < c1; ++c) s += (double)slab[c * K + k];
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && k < K) {
    double t = part[0][lane];
#pragma unroll
    for (int w = 1; w < SN_WAVES; ++w) t += part[w][lane];
    A[k] = (float)t;
    if (u_next != nullptr) u_next[k] = (float)(1.0 / ((double)K * t));
  }
}

// the shared front of the loss and its gradient for one pair: tv[j] = E u (the target times d), the student's arguments
// a[j] = s / tau (0 from K on; callers mask by k < K), and *sum = d in float64 (FWD) or sum_k tv[k] (the backward, which
// takes d from the forward)
template <typename TX, typename TS, int KPL, bool FWD>
__device__ __forceinline__ void sn_pair(const TX* __restrict__ xr, const TS* __restrict__ sr, int K, int lane, bool vec,
                                        float thi, float tlo, float shi, float slo, const float (&uk)[KPL], float (&tv)[KPL],
                                        float (&a)[KPL], double* sum) {
  float sraw[KPL];
  sn_load<KPL>(sr, K, lane, vec, sraw);
  sn_exp_row<TX, KPL>(xr, K, lane, vec, thi, tlo, tv);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    if (FWD) acc += (double)tv[j] * (double)uk[j];
    tv[j] *= uk[j];
    if (!FWD) acc += (double)tv[j];
    float p, r;
    sn_arg(sraw[j], shi, slo, &p, &r);
    a[j] = p + r;
  }
  *sum = sn_wsum(acc);
}

template <typename TX, typename TS, int KPL>
__global__ void __launch_bounds__(SN_THREADS) sn_ce_fwd_kernel(
    const TX* __restrict__ x, const void* __restrict__ idx_t, int t32, int64_t nt, const TS* __restrict__ s,
    const void* __restrict__ idx_s, int s32, int64_t ns, int64_t M, int K, float thi, float tlo, float shi, float slo,
    const float* __restrict__ u, double* __restrict__ loss_m, float* __restrict__ d_out, float* __restrict__ lse_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool vec = (K & 1) == 0 && sn_pairs_ok(x) && sn_pairs_ok(s) && sn_pairs_ok(u);
  float uk[KPL];
  sn_load<KPL>(u, K, lane, vec, uk);
  for (int64_t m = (int64_t)blockIdx.x * SN_WAVES + wave; m < M; m += (int64_t)gridDim.x * SN_WAVES) {
    const int64_t rt = sn_index(idx_t, t32, m, nt), rs = sn_index(idx_s, s32, m, ns);
    float tv[KPL], a[KPL];
    double d;
    sn_pair<TX, TS, KPL, true>(x + rt * K, s + rs * K, K, lane, vec, thi, tlo, shi, slo, uk, tv, a, &d);
    float mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < KPL; ++j) mx = sn_k(j, lane, vec) < K ? fmaxf(mx, a[j]) : mx;
    mx = sn_wmax(mx);
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < KPL; ++j) se += sn_k(j, lane, vec) < K ? (double)expf(a[j] - mx) : 0.0;
    const double lse = (double)mx + log(sn_wsum(se));
    double lo = 0.0;
#pragma unroll
    for (int j = 0; j < KPL; ++j) lo += (double)tv[j] * ((double)a[j] - lse);     // tv is 0 from K on
    lo = sn_wsum(lo);
    if (lane == 0) {
      loss_m[m] = -lo / d;
      d_out[m] = (float)d;
      lse_out[m] = (float)lse;
    }
  }
}

// first m with idx_s[m] >= row
__device__ __forceinline__ int64_t sn_lower(const void* __restrict__ idx_s, int s32, int64_t M, int64_t row) {
  int64_t lo = 0, hi = M;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int64_t v = s32 ? (int64_t)((const int32_t*)idx_s)[mid] : ((const int64_t*)idx_s)[mid];
    if (v < row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// scene of a student row: the number of scene ends at or below it (nb for a row behind the last scene)
__device__ __forceinline__ int sn_scene(const int64_t* __restrict__ offset, int nb, int64_t row) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offset[mid] <= row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// loss = mean over the scenes 0 .. B - 1 of the mean of a scene's pairs, B = 1 + the scene of the last pair; a scene
// without a pair below B counts with mean 0 (segment_coo(reduce="mean") with dim_size = index.max() + 1).
// gscale[b] = 1 / (count_b B), 0 for an empty scene and from B on.
__global__ void __launch_bounds__(SN_THREADS) sn_ce_finish_kernel(const double* __restrict__ loss_m,
                                                                 const void* __restrict__ idx_s, int s32, int64_t M,
                                                                 const int64_t* __restrict__ offset, int nb,
                                                                 float* __restrict__ loss, float* __restrict__ gscale) {
  __shared__ double red[SN_THREADS];
  const int tid = threadIdx.x;
  const int64_t last = s32 ? (int64_t)((const int32_t*)idx_s)[M - 1] : ((const int64_t*)idx_s)[M - 1];
  int B = sn_scene(offset, nb, last);           // scene of the last pair
  B = B < nb ? B + 1 : nb;
  double total = 0.0;
  for (int b = 0; b < nb; ++b) {
    if (b >= B) {
      if (tid == 0) gscale[b] = 0.f;
      continue;
    }
    const int64_t m0 = sn_lower(idx_s, s32, M, b == 0 ? 0 : offset[b - 1]);
    const int64_t m1 = sn_lower(idx_s, s32, M, offset[b]);
    double sum = 0.0;
    for (int64_t m = m0 + tid; m < m1; m += SN_THREADS) sum += loss_m[m];
    red[tid] = sum;
    for (int d = SN_THREADS >> 1; d >= 1; d >>= 1) {
      __syncthreads();
      if (tid < d) red[tid] += red[tid + d];
    }
    __syncthreads();
    const int64_t cnt = m1 - m0;
    if (cnt > 0) total += red[0] / (double)cnt;
    if (tid == 0) gscale[b] = cnt > 0 ? (float)(1.0 / ((double)cnt * (double)B)) : 0.f;
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(total / (double)B);
}

template <typename TX, typename TS, int KPL>
__global__ void __launch_bounds__(SN_THREADS) sn_ce_bwd_kernel(
    const float* __restrict__ dloss, const TX* __restrict__ x, const void* __restrict__ idx_t, int t32, int64_t nt,
    const TS* __restrict__ s, const void* __restrict__ idx_s, int s32, int64_t ns, int64_t M, int K, float thi, float tlo,
    float shi, float slo, const float* __restrict__ u, const float* __restrict__ d_in, const float* __restrict__ lse_in,
    const int64_t* __restrict__ offset, int nb, const float* __restrict__ gscale, TS* __restrict__ ds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool vec = (K & 1) == 0 && sn_pairs_ok(x) && sn_pairs_ok(s) && sn_pairs_ok(u) && sn_pairs_ok(ds);
  float uk[KPL];
  sn_load<KPL>(u, K, lane, vec, uk);
  const float g0 = dloss[0] * (shi + slo);
  for (int64_t row = (int64_t)blockIdx.x * SN_WAVES + wave; row < ns; row += (int64_t)gridDim.x * SN_WAVES) {
    TS* out = ds + row * K;
    const int64_t m = sn_lower(idx_s, s32, M, row);
    const bool hit = m < M && (s32 ? (int64_t)((const int32_t*)idx_s)[m] : ((const int64_t*)idx_s)[m]) == row;
    if (!hit) {
      float zero[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) zero[j] = 0.f;
      sn_store<KPL>(out, K, lane, vec, zero);
      continue;
    }
    const int b = sn_scene(offset, nb, row);
    const float g = b < nb ? g0 * gscale[b] : 0.f;
    const int64_t rt = sn_index(idx_t, t32, m, nt);
    float tv[KPL], a[KPL];
    double tsum;
    sn_pair<TX, TS, KPL, false>(x + rt * K, s + row * K, K, lane, vec, thi, tlo, shi, slo, uk, tv, a, &tsum);
    const float dm = d_in[m], lse = lse_in[m];
    const float rd = 1.f / dm, st = (float)tsum * rd;
#pragma unroll
    for (int j = 0; j < KPL; ++j) a[j] = g * (expf(a[j] - lse) * st - tv[j] * rd);
    sn_store<KPL>(out, K, lane, vec, a);
  }
}

static bool sn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static void sn_split(double v, float* hi, float* lo) {
  *hi = (float)v;
  *lo = (float)(v - (double)*hi);
}
static bool sn_finite(double v) { return v == v && v - v == 0.0; }

}  // namespace ptv3

using namespace ptv3;

// KPL = entries per lane: 64 * KPL >= K
static int sn_kpl(int K) { return K <= 128 ? 2 : K <= 1024 ? 16 : 64; }

extern "C" int ptv3_sonata_capable(int K) { return K >= 2 && K <= SN_MAX_K; }

extern "C" size_t ptv3_sonata_sk_workspace_bytes(int64_t M, int K) {
  if (M <= 0 || K <= 0) return 0;
  return (size_t)cdiv(M, SN_ROWS) * (size_t)K * sizeof(float);
}

extern "C" int ptv3_sonata_sk_pass(const void* x, int x_dtype, const void* idx_t, int idx_i32, int64_t nt, int64_t M,
                                   int K, double inv_temp, const float* u, double n_total, float* A, float* u_next,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  PTV3_REQUIRE(ptv3_sonata_capable(K), "sonata_sk_pass: K=%d unsupported (2 to %d prototypes)", K, SN_MAX_K);
  PTV3_REQUIRE(x_dtype == PTV3_F32 || x_dtype == PTV3_BF16, "sonata_sk_pass: x must be fp32 or bf16");
  PTV3_REQUIRE(M > 0 && M < (1ll << 31) && nt > 0, "sonata_sk_pass: M=%lld / nt=%lld unsupported", (long long)M,
               (long long)nt);
  PTV3_REQUIRE(sn_finite(inv_temp) && inv_temp > 0, "sonata_sk_pass: 1 / T must be finite and positive");
  PTV3_REQUIRE(u == nullptr || n_total >= 1.0, "sonata_sk_pass: n_total must count the rows of all ranks");
  PTV3_REQUIRE(x && idx_t && A, "sonata_sk_pass: a pointer is NULL");
  PTV3_REQUIRE(workspace && sn_aligned16(workspace) && workspace_bytes >= ptv3_sonata_sk_workspace_bytes(M, K),
               "sonata_sk_pass: workspace missing, unaligned or too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = cdiv(M, SN_ROWS);
  float hi, lo;
  sn_split(inv_temp, &hi, &lo);
  const double inv_n = u ? 1.0 / n_total : 1.0;
  float* slab = (float*)workspace;
  by_dtype(x_dtype, [&](auto tx) {
    using X = typename decltype(tx)::type;
    by_value<2, 16, 64>(sn_kpl(K), [&](auto KPL) {
      hipLaunchKernelGGL((sn_sk_partial_kernel<X, KPL()>), dim3((unsigned)chunks), dim3(SN_THREADS), 0, st, (const X*)x,
                         idx_t, idx_i32, nt, M, K, hi, lo, u, inv_n, slab);
    });
  });
  PTV3_LAUNCH_CHECK();
  hipLaunchKernelGGL(sn_sk_finish_kernel, dim3((unsigned)cdiv(K, SN_FIN_COLS)), dim3(SN_THREADS), 0, st, slab, chunks, K,
                     A, u_next);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" size_t ptv3_sonata_ce_workspace_bytes(int64_t M) { return M > 0 ? (size_t)M * sizeof(double) : 0; }

static int sn_ce_args(const char* who, int K, int x_dtype, int s_dtype, int64_t nt, int64_t ns, int64_t M, int nb,
                      double inv_temp, double inv_tau) {
  PTV3_REQUIRE(ptv3_sonata_capable(K), "%s: K=%d unsupported (2 to %d prototypes)", who, K, SN_MAX_K);
  PTV3_REQUIRE((x_dtype == PTV3_F32 || x_dtype == PTV3_BF16) && (s_dtype == PTV3_F32 || s_dtype == PTV3_BF16),
               "%s: logits must be fp32 or bf16", who);
  PTV3_REQUIRE(M > 0 && M < (1ll << 31) && nt > 0 && ns > 0 && M <= ns, "%s: M=%lld / nt=%lld / ns=%lld unsupported", who,
               (long long)M, (long long)nt, (long long)ns);
  PTV3_REQUIRE(nb >= 1 && nb <= SN_MAX_SCENES, "%s: nb=%d unsupported (1 to %d scenes)", who, nb, SN_MAX_SCENES);
  PTV3_REQUIRE(sn_finite(inv_temp) && inv_temp > 0 && sn_finite(inv_tau) && inv_tau > 0,
               "%s: 1 / T and 1 / tau must be finite and positive", who);
  return PTV3_OK;
}

extern "C" int ptv3_sonata_ce_fwd(const void* x, int x_dtype, const void* idx_t, int idx_t_i32, int64_t nt, const void* s,
                                  int s_dtype, const void* idx_s, int idx_s_i32, int64_t ns, int64_t M, int K,
                                  double inv_temp, double inv_tau, const float* u, const int64_t* offset_s, int nb,
                                  float* loss, float* d, float* lse, float* gscale, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  const int rc = sn_ce_args("sonata_ce_fwd", K, x_dtype, s_dtype, nt, ns, M, nb, inv_temp, inv_tau);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(x && idx_t && s && idx_s && u && offset_s && loss && d && lse && gscale, "sonata_ce_fwd: a pointer is NULL");
  PTV3_REQUIRE(workspace && sn_aligned16(workspace) && workspace_bytes >= ptv3_sonata_ce_workspace_bytes(M),
               "sonata_ce_fwd: workspace missing, unaligned or too small");
  hipStream_t st = (hipStream_t)stream;
  float thi, tlo, shi, slo;
  sn_split(inv_temp, &thi, &tlo);
  sn_split(inv_tau, &shi, &slo);
  double* loss_m = (double*)workspace;
  const int64_t want = cdiv(M, SN_WAVES);
  const dim3 grid((unsigned)(want < 8192 ? want : 8192));
  by_dtype(x_dtype, [&](auto tx) {
    using X = typename decltype(tx)::type;
    by_dtype(s_dtype, [&](auto ts) {
      using S = typename decltype(ts)::type;
      by_value<2, 16, 64>(sn_kpl(K), [&](auto KPL) {
        hipLaunchKernelGGL((sn_ce_fwd_kernel<X, S, KPL()>), grid, dim3(SN_THREADS), 0, st, (const X*)x, idx_t, idx_t_i32,
                           nt, (const S*)s, idx_s, idx_s_i32, ns, M, K, thi, tlo, shi, slo, u, loss_m, d, lse);
      });
    });
  });
  PTV3_LAUNCH_CHECK();
  hipLaunchKernelGGL(sn_ce_finish_kernel, dim3(1), dim3(SN_THREADS), 0, st, loss_m, idx_s, idx_s_i32, M, offset_s, nb,
                     loss, gscale);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_sonata_ce_bwd(const float* dloss, const void* x, int x_dtype, const void* idx_t, int idx_t_i32,
                                  int64_t nt, const void* s, int s_dtype, const void* idx_s, int idx_s_i32, int64_t ns,
                                  int64_t M, int K, double inv_temp, double inv_tau, const float* u, const float* d,
                                  const float* lse, const int64_t* offset_s, int nb, const float* gscale, void* ds,
                                  void* stream) {
  const int rc = sn_ce_args("sonata_ce_bwd", K, x_dtype, s_dtype, nt, ns, M, nb, inv_temp, inv_tau);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(dloss && x && idx_t && s && idx_s && u && d && lse && offset_s && gscale && ds,
               "sonata_ce_bwd: a pointer is NULL");
  hipStream_t st = (hipStream_t)stream;
  float thi, tlo, shi, slo;
  sn_split(inv_temp, &thi, &tlo);
  sn_split(inv_tau, &shi, &slo);
  const int64_t want = cdiv(ns, SN_WAVES);
  const dim3 grid((unsigned)(want < 8192 ? want : 8192));
  by_dtype(x_dtype, [&](auto tx) {
    using X = typename decltype(tx)::type;
    by_dtype(s_dtype, [&](auto ts) {
      using S = typename decltype(ts)::type;
      by_value<2, 16, 64>(sn_kpl(K), [&](auto KPL) {
        hipLaunchKernelGGL((sn_ce_bwd_kernel<X, S, KPL()>), grid, dim3(SN_THREADS), 0, st, dloss, (const X*)x, idx_t,
                           idx_t_i32, nt, (const S*)s, idx_s, idx_s_i32, ns, M, K, thi, tlo, shi, slo, u, d, lse, offset_s,
                           nb, gscale, (S*)ds);
      });
    });
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
