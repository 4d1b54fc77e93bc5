// Image branch of "Concerto-v1m1" (concerto_v1m1_base.py: pool_corr :529-573, the patch mean and the cosine loss
// :781-845) without the gathered (pairs, C) copy and without the dense (images * patches, C) matrix.
//   cc_pool_corr_kernel    a thread per (cluster, view): the children of the cluster in the pooling's own order, count of
//                          the children with both entries set, elementwise sums with -1 read as 0, in float64
//   cc_pair_keys_kernel    a thread per (row, view): the patch of a valid pair as a sort key, NO_PATCH otherwise
//   cc_plan_finish_kernel  the patch of every run and the feature row of every sorted pair
//   cc_mean_fwd_kernel     a wavefront per occupied patch: its pairs' feature rows are gathered and added in order, the
//                          lanes across the columns (4 per lane and load when the rows allow it)
//   cc_mean_bwd_kernel     a wavefront per feature row, the one owner of that row of the gradient: zeros for a row that
//                          is not among the principal views (bisection in `rows`), else the V slots of the row in order
//   cc_cos_fwd_kernel      a wavefront per occupied patch: both rows are read once into registers, means, centred dot
//                          product and norms reduced over the wavefront in float64
//   cc_cos_finish_kernel   one workgroup: 1 - cos added per thread in row order, then the threads in order, in float64
//   cc_cos_bwd_kernel      a wavefront per occupied patch: one pass over the two rows, the statistics formed again in
//                          float64 from the registers (fp32 statistics lose the gradient of a row whose centred norm
//                          is small), da = g (y - (x . y / |x|^2) x) / (|x| |y|)
// No atomics: every hand-off is a kernel boundary, two runs are bitwise equal.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_MAX_D = 2048;
constexpr float CC_EPS = 1e-6f;

__device__ __forceinline__ double cc_wsum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ float cc_ld(const float* p) { return *p; }
__device__ __forceinline__ float cc_ld(const __bf16* p) { return (float)*p; }
__device__ __forceinline__ void cc_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void cc_st(__bf16* p, float v) { *p = (__bf16)v; }

// ---- correspondence pooling ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS)
cc_pool_corr_kernel(const float* __restrict__ in, const int64_t* __restrict__ order, const int32_t* __restrict__ seg_start,
                    int64_t n_in, int64_t n_out, int V, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (t >= n_out * V) return;
  const int64_t c = t / V;
  const int v = (int)(t - c * V);
  int64_t lo = seg_start[c], hi = seg_start[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_in ? n_in : hi;                      // `order` holds n_in entries
  double s0 = 0.0, s1 = 0.0;
  int64_t count = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t child = order[i];
    if (child < 0 || child >= n_in) continue;
    const f32x2 p = *(const f32x2*)(in + (child * V + v) * 2);
    count += (p[0] != -1.f && p[1] != -1.f) ? 1 : 0;
    s0 += p[0] == -1.f ? 0.0 : (double)p[0];
    s1 += p[1] == -1.f ? 0.0 : (double)p[1];
  }
  f32x2 r = {-1.f, -1.f};
  if (count > 0) r = f32x2{(float)(s0 / (double)count), (float)(s1 / (double)count)};
  *(f32x2*)(out + t * 2) = r;
}

// ---- patch plan ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS)
cc_pair_keys_kernel(const float* __restrict__ corr, int64_t n, const int64_t* __restrict__ rows,
                    const int64_t* __restrict__ scene, int64_t R, int V, const int64_t* __restrict__ img_base, int ns,
                    int patch_h, int patch_w, int64_t n_patches, int64_t* __restrict__ key) {
  const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  const int64_t P = R * V;
  if (t > P) return;
  int64_t k = PTV3_CONCERTO_NO_PATCH;
  if (t < P) {
    const int64_t r = t / V;
    const int v = (int)(t - r * V);
    const int64_t row = rows[r];
    const int64_t sc = scene[r];
    if (row >= 0 && row < n && sc >= 0 && sc < ns) {
      const f32x2 p = *(const f32x2*)(corr + (row * V + v) * 2);
      if (p[0] != -1.f || p[1] != -1.f) {
        // float -> int64 as Tensor.long(): towards zero; a coordinate that is no number or far outside is out of range
        const bool sane = fabsf(p[0]) < 1e9f && fabsf(p[1]) < 1e9f;
        const int64_t patch = sane ? (img_base[sc] + v) * (int64_t)patch_h * patch_w + (int64_t)p[0] * patch_w + (int64_t)p[1]
                                   : -1;
        k = (patch >= 0 && patch < n_patches) ? patch : n_patches;
      }
    }
  }
  key[t] = k;
}

__global__ void __launch_bounds__(CC_THREADS)
cc_plan_finish_kernel(const int64_t* __restrict__ key, const int64_t* __restrict__ order,
                      const int32_t* __restrict__ seg_start, const int64_t* __restrict__ rows, int64_t R, int V, int64_t U,
                      int64_t* __restrict__ patch_ids, int64_t* __restrict__ pair_row) {
  const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  const int64_t P = R * V;
  if (t < P) {
    const int64_t o = order[t];
    pair_row[t] = (o >= 0 && o < P) ? rows[o / V] : 0;
  }
  if (t < U) {
    const int64_t s = seg_start[t];
    const int64_t o = (s >= 0 && s <= P) ? order[s] : P;
    patch_ids[t] = (o >= 0 && o <= P) ? key[o] : 0;
  }
}

// ---- patch mean ------------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ void __launch_bounds__(CC_THREADS)
cc_mean_fwd_kernel(const T* __restrict__ feat, int64_t n, int C, const int64_t* __restrict__ pair_row,
                   const int32_t* __restrict__ seg_start, int64_t U, float* __restrict__ mean) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
  if (j >= U) return;
  const int64_t lo = seg_start[j], hi = seg_start[j + 1];
  const float cnt = (float)(hi - lo);
  float* out = mean + j * C;
  for (int c0 = lane * VEC; c0 < C; c0 += 64 * VEC) {
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
    for (int64_t i = lo; i < hi; ++i) {
      int64_t row = pair_row[i];
      row = row < 0 ? 0 : (row < n ? row : n - 1);
      const T* src = feat + row * C + c0;
      if (VEC == 4) {
        float w[4];
        unpack4<T>(*(const typename Vec4<T>::type*)src, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += w[q];
      } else {
        acc[0] += cc_ld(src);
      }
    }
    if (VEC == 4) {
      *(f32x4*)(out + c0) = f32x4{acc[0] / cnt, acc[1] / cnt, acc[2] / cnt, acc[3] / cnt};
    } else {
      out[c0] = acc[0] / cnt;
    }
  }
}

template <typename T, int VEC>
__global__ void __launch_bounds__(CC_THREADS)
cc_mean_bwd_kernel(const float* __restrict__ dmean, const int64_t* __restrict__ rows, const int64_t* __restrict__ slot,
                   const int32_t* __restrict__ seg_start, int64_t n, int64_t R, int V, int64_t U, int C,
                   T* __restrict__ dfeat) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
  if (row >= n) return;
  // rows is ascending: the position of this feature row among the principal views, if it is one of them
  int64_t lo = 0, hi = R;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rows[mid] < row) lo = mid + 1; else hi = mid;
  }
  const bool mine = lo < R && rows[lo] == row;
  T* out = dfeat + row * C;
  for (int c0 = lane * VEC; c0 < C; c0 += 64 * VEC) {
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
    if (mine) {
      for (int v = 0; v < V; ++v) {
        const int64_t s = slot[lo * V + v];
        if (s < 0 || s >= U) continue;
        const float cnt = (float)(seg_start[s + 1] - seg_start[s]);
        const float* src = dmean + s * C + c0;
        if (VEC == 4) {
          const f32x4 w = *(const f32x4*)src;
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] += w[q] / cnt;
        } else {
          acc[0] += *src / cnt;
        }
      }
    }
    if (VEC == 4) {
      *(typename Vec4<T>::type*)(out + c0) = pack4<T>(acc[0], acc[1], acc[2], acc[3]);
    } else {
      cc_st(out + c0, acc[0]);
    }
  }
}

// ---- centred cosine loss ---------------------------------------------------------------------------------------------
// v[q] = row[q * 64 + lane], 0 from D on
template <typename T, int DPL>
__device__ __forceinline__ void cc_row(const T* __restrict__ row, int D, int lane, double (&v)[DPL]) {
#pragma unroll
  for (int q = 0; q < DPL; ++q) {
    const int d = q * 64 + lane;
    v[q] = d < D ? (double)cc_ld(row + d) : 0.0;
  }
}

__device__ __forceinline__ int64_t cc_brow(const int64_t* __restrict__ patch_ids, int64_t j, int64_t nb) {
  const int64_t p = patch_ids[j];
  return p < 0 ? 0 : (p < nb ? p : nb - 1);
}

// The statistics of row j, every lane holding all of them: the rows' means over D (0 without the shift), the centred rows
// x = a - mean, y = b - mean left in va / vb as float64 (0 from D on), their dot product and norms.  All in float64: a row
// whose centred norm is small against its entries (a0 ~ a1 at D = 2, a nearly constant row) loses its cosine and, twice
// over, its gradient when the mean is rounded to fp32 first.
template <int DPL>
__device__ __forceinline__ void cc_centre(double (&va)[DPL], double (&vb)[DPL], int D, int lane, int shift, double* ma,
                                          double* mb, double* dot, double* norm_a, double* norm_b) {
  *ma = 0.0;
  *mb = 0.0;
  if (shift) {
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int q = 0; q < DPL; ++q) { sa += va[q]; sb += vb[q]; }
    *ma = cc_wsum(sa) / (double)D;
    *mb = cc_wsum(sb) / (double)D;
  }
  double d = 0.0, na = 0.0, nbq = 0.0;
#pragma unroll
  for (int q = 0; q < DPL; ++q) {
    const bool in = q * 64 + lane < D;
    va[q] = in ? va[q] - *ma : 0.0;
    vb[q] = in ? vb[q] - *mb : 0.0;
    d += va[q] * vb[q];
    na += va[q] * va[q];
    nbq += vb[q] * vb[q];
  }
  *dot = cc_wsum(d);
  *norm_a = sqrt(cc_wsum(na));
  *norm_b = sqrt(cc_wsum(nbq));
}

template <typename TA, typename TB, int DPL>
__global__ void __launch_bounds__(CC_THREADS)
cc_cos_fwd_kernel(const TA* __restrict__ a, const TB* __restrict__ b, const int64_t* __restrict__ patch_ids, int64_t U,
                  int64_t nb, int D, int shift, float* __restrict__ cosv, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
  if (j >= U) return;
  double va[DPL], vb[DPL];
  cc_row<TA, DPL>(a + j * D, D, lane, va);
  cc_row<TB, DPL>(b + cc_brow(patch_ids, j, nb) * D, D, lane, vb);
  double ma, mb, dot, norm_a, norm_b;
  cc_centre<DPL>(va, vb, D, lane, shift, &ma, &mb, &dot, &norm_a, &norm_b);
  const double ca = norm_a > (double)CC_EPS ? norm_a : (double)CC_EPS;
  const double cb = norm_b > (double)CC_EPS ? norm_b : (double)CC_EPS;
  const double c = dot / (ca * cb);
  if (lane == 0) {
    cosv[j] = (float)c;
    stats[j * 4 + 0] = (float)ma;
    stats[j * 4 + 1] = (float)mb;
    stats[j * 4 + 2] = (float)norm_a;
    stats[j * 4 + 3] = (float)norm_b;
  }
}

__global__ void __launch_bounds__(CC_THREADS)
cc_cos_finish_kernel(const float* __restrict__ cosv, int64_t U, float* __restrict__ loss) {
  __shared__ double part[CC_THREADS];
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < U; j += CC_THREADS) s += 1.0 - (double)cosv[j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int t = 0; t < CC_THREADS; ++t) total += part[t];
    loss[0] = (float)(10.0 * total / (double)U);
  }
}

template <typename TA, typename TB, int DPL>
__global__ void __launch_bounds__(CC_THREADS)
cc_cos_bwd_kernel(const float* __restrict__ dloss, const TA* __restrict__ a, const TB* __restrict__ b,
                  const int64_t* __restrict__ patch_ids, int64_t U, int64_t nb, int D, int shift, TA* __restrict__ da) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
  if (j >= U) return;
  double va[DPL], vb[DPL];
  cc_row<TA, DPL>(a + j * D, D, lane, va);
  cc_row<TB, DPL>(b + cc_brow(patch_ids, j, nb) * D, D, lane, vb);
  double ma, mb, dot, norm_a, norm_b;
  cc_centre<DPL>(va, vb, D, lane, shift, &ma, &mb, &dot, &norm_a, &norm_b);
  const double ca = norm_a > (double)CC_EPS ? norm_a : (double)CC_EPS;
  const double cb = norm_b > (double)CC_EPS ? norm_b : (double)CC_EPS;
  // d cos / d x = (y - (x . y / |x|^2) x) / (|x| |y|); on the eps branch the clamped norm is a constant.  The mean of this
  // over D, which the shift's own backward would take off, is 0 up to float64 rounding and is not subtracted.
  const double g = -10.0 * (double)dloss[0] / (double)U / (ca * cb);
  const double r = norm_a > (double)CC_EPS ? dot / (norm_a * norm_a) : 0.0;
  TA* out = da + j * D;
#pragma unroll
  for (int q = 0; q < DPL; ++q) {
    const int d = q * 64 + lane;
    if (d < D) cc_st(out + d, (float)(g * (vb[q] - r * va[q])));
  }
}

static bool cc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_concerto_pool_corr(const float* corr_in, const int64_t* order, const int32_t* seg_start, int64_t n_in,
                                       int64_t n_out, int V, float* out, void* stream) {
  PTV3_REQUIRE(n_in > 0 && n_out > 0 && V > 0 && n_out * V < (1ll << 31) && n_in < (1ll << 31),
               "concerto_pool_corr: n_in=%lld / n_out=%lld / V=%d unsupported", (long long)n_in, (long long)n_out, V);
  PTV3_REQUIRE(corr_in && order && seg_start && out, "concerto_pool_corr: a pointer is NULL");
  PTV3_REQUIRE((((uintptr_t)corr_in | (uintptr_t)out) & 7) == 0, "concerto_pool_corr: correspondences must be 8-byte aligned");
  hipLaunchKernelGGL(cc_pool_corr_kernel, dim3((unsigned)cdiv(n_out * V, CC_THREADS)), dim3(CC_THREADS), 0,
                     (hipStream_t)stream, corr_in, order, seg_start, n_in, n_out, V, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_concerto_pair_keys(const float* corr, int64_t n, const int64_t* rows, const int64_t* scene, int64_t R,
                                       int V, const int64_t* img_base, int ns, int patch_h, int patch_w, int64_t n_patches,
                                       int64_t* key, void* stream) {
  PTV3_REQUIRE(n > 0 && R > 0 && V > 0 && ns > 0 && R * V < (1ll << 31) - 1,
               "concerto_pair_keys: n=%lld / R=%lld / V=%d / ns=%d unsupported", (long long)n, (long long)R, V, ns);
  PTV3_REQUIRE(patch_h > 0 && patch_w > 0 && n_patches > 0 && n_patches < PTV3_CONCERTO_NO_PATCH,
               "concerto_pair_keys: patch grid %d x %d, %lld patches unsupported", patch_h, patch_w, (long long)n_patches);
  PTV3_REQUIRE(corr && rows && scene && img_base && key, "concerto_pair_keys: a pointer is NULL");
  PTV3_REQUIRE(((uintptr_t)corr & 7) == 0, "concerto_pair_keys: correspondences must be 8-byte aligned");
  hipLaunchKernelGGL(cc_pair_keys_kernel, dim3((unsigned)cdiv(R * V + 1, CC_THREADS)), dim3(CC_THREADS), 0,
                     (hipStream_t)stream, corr, n, rows, scene, R, V, img_base, ns, patch_h, patch_w, n_patches, key);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_concerto_plan_finish(const int64_t* key, const int64_t* order, const int32_t* seg_start,
                                         const int64_t* rows, int64_t R, int V, int64_t U, int64_t* patch_ids,
                                         int64_t* pair_row, void* stream) {
  PTV3_REQUIRE(R > 0 && V > 0 && R * V < (1ll << 31) - 1 && U >= 0 && U <= R * V,
               "concerto_plan_finish: R=%lld / V=%d / U=%lld unsupported", (long long)R, V, (long long)U);
  PTV3_REQUIRE(key && order && seg_start && rows && pair_row && (patch_ids || U == 0),
               "concerto_plan_finish: a pointer is NULL");
  hipLaunchKernelGGL(cc_plan_finish_kernel, dim3((unsigned)cdiv(R * V, CC_THREADS)), dim3(CC_THREADS), 0,
                     (hipStream_t)stream, key, order, seg_start, rows, R, V, U, patch_ids, pair_row);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_concerto_patch_mean_fwd(const void* feat, int dtype, int64_t n, int C, const int64_t* pair_row,
                                            const int32_t* seg_start, int64_t U, float* mean, void* stream) {
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "concerto_patch_mean_fwd: feat must be fp32 or bf16");
  PTV3_REQUIRE(n > 0 && C > 0 && U > 0 && cdiv(U, CC_WAVES) < (1ll << 31),
               "concerto_patch_mean_fwd: n=%lld / C=%d / U=%lld unsupported", (long long)n, C, (long long)U);
  PTV3_REQUIRE(feat && pair_row && seg_start && mean, "concerto_patch_mean_fwd: a pointer is NULL");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(U, CC_WAVES));
  const bool vec = C % 4 == 0 && cc_aligned16(feat) && cc_aligned16(mean);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_value<1, 4>(vec ? 4 : 1, [&](auto VEC) {
      hipLaunchKernelGGL((cc_mean_fwd_kernel<T, VEC()>), grid, dim3(CC_THREADS), 0, st, (const T*)feat, n, C, pair_row,
                         seg_start, U, mean);
    });
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_concerto_patch_mean_bwd(const float* dmean, const int64_t* rows, const int64_t* slot,
                                            const int32_t* seg_start, int64_t n, int64_t R, int V, int64_t U, int C,
                                            void* dfeat, int dtype, void* stream) {
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "concerto_patch_mean_bwd: dfeat must be fp32 or bf16");
  PTV3_REQUIRE(n > 0 && C > 0 && U > 0 && R > 0 && V > 0 && cdiv(n, CC_WAVES) < (1ll << 31),
               "concerto_patch_mean_bwd: n=%lld / C=%d / U=%lld / R=%lld / V=%d unsupported", (long long)n, C,
               (long long)U, (long long)R, V);
  PTV3_REQUIRE(dmean && rows && slot && seg_start && dfeat, "concerto_patch_mean_bwd: a pointer is NULL");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(n, CC_WAVES));
  const bool vec = C % 4 == 0 && cc_aligned16(dmean) && cc_aligned16(dfeat);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_value<1, 4>(vec ? 4 : 1, [&](auto VEC) {
      hipLaunchKernelGGL((cc_mean_bwd_kernel<T, VEC()>), grid, dim3(CC_THREADS), 0, st, dmean, rows, slot, seg_start, n,
                         R, V, U, C, (T*)dfeat);
    });
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_concerto_cos_capable(int D) { return D >= 1 && D <= CC_MAX_D; }

// entries per lane: 2 (D <= 128), 8 (<= 512), 24 (<= 1536), 32 (<= 2048)
static int cc_dpl(int D) { return D <= 128 ? 2 : D <= 512 ? 8 : D <= 1536 ? 24 : 32; }

static int cc_cos_args(const char* who, int a_dtype, int b_dtype, int64_t U, int64_t nb, int D) {
  PTV3_REQUIRE(ptv3_concerto_cos_capable(D), "%s: D=%d unsupported (1 to %d channels)", who, D, CC_MAX_D);
  PTV3_REQUIRE((a_dtype == PTV3_F32 || a_dtype == PTV3_BF16) && (b_dtype == PTV3_F32 || b_dtype == PTV3_BF16),
               "%s: rows must be fp32 or bf16", who);
  PTV3_REQUIRE(U > 0 && nb > 0 && cdiv(U, CC_WAVES) < (1ll << 31), "%s: U=%lld / nb=%lld unsupported", who, (long long)U,
               (long long)nb);
  return PTV3_OK;
}

extern "C" int ptv3_concerto_cos_fwd(const void* a, int a_dtype, const void* b, int b_dtype, const int64_t* patch_ids,
                                     int64_t U, int64_t nb, int D, int shift, float* cosv, float* stats, float* loss,
                                     void* stream) {
  const int rc = cc_cos_args("concerto_cos_fwd", a_dtype, b_dtype, U, nb, D);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(a && b && patch_ids && cosv && stats && loss, "concerto_cos_fwd: a pointer is NULL");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(U, CC_WAVES));
  by_dtype(a_dtype, [&](auto ta) {
    using A = typename decltype(ta)::type;
    by_dtype(b_dtype, [&](auto tb) {
      using B = typename decltype(tb)::type;
      by_value<2, 8, 24, 32>(cc_dpl(D), [&](auto DPL) {
        hipLaunchKernelGGL((cc_cos_fwd_kernel<A, B, DPL()>), grid, dim3(CC_THREADS), 0, st, (const A*)a, (const B*)b,
                           patch_ids, U, nb, D, shift, cosv, stats);
      });
    });
  });
  PTV3_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_cos_finish_kernel, dim3(1), dim3(CC_THREADS), 0, st, cosv, U, loss);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_concerto_cos_bwd(const float* dloss, const void* a, int a_dtype, const void* b, int b_dtype,
                                     const int64_t* patch_ids, int64_t U, int64_t nb, int D, int shift, void* da,
                                     void* stream) {
  const int rc = cc_cos_args("concerto_cos_bwd", a_dtype, b_dtype, U, nb, D);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(dloss && a && b && patch_ids && da, "concerto_cos_bwd: a pointer is NULL");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(U, CC_WAVES));
  by_dtype(a_dtype, [&](auto ta) {
    using A = typename decltype(ta)::type;
    by_dtype(b_dtype, [&](auto tb) {
      using B = typename decltype(tb)::type;
      by_value<2, 8, 24, 32>(cc_dpl(D), [&](auto DPL) {
        hipLaunchKernelGGL((cc_cos_bwd_kernel<A, B, DPL()>), grid, dim3(CC_THREADS), 0, st, dloss, (const A*)a,
                           (const B*)b, patch_ids, U, nb, D, shift, (A*)da);
      });
    });
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
