// Global-regression keypoint heads (KeypointPTv3 / KeypointSwin3D): per-scene column mean of the backbone features,
// the small MLP on the pooled rows, and the backward of the mean.
//   scene_mean_partial_kernel  fixed row chunks that never straddle a scene boundary -> one fp32 slab row per chunk
//   scene_mean_finish_kernel   one workgroup per scene: its slabs summed in a fixed order, / row count (0 if empty);
//                              HEAD: then Linear + folded BatchNorm + ReLU -> Linear + ReLU -> Linear, fp32
//   scene_mean_bwd_kernel      dfeat[i, :] = dg[scene(i), :] / n_scene(i)
// Deterministic: no atomics, and the hand-off between the two halves is a kernel boundary.
#include "common.h"
#include "scene_chunks.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int SM_THREADS = 256;     // partial / backward workgroups
constexpr int SF_THREADS = 1024;    // finishing workgroup (one per scene)
constexpr int SM_MAX_C = 1024;      // pooled row held in LDS by the finishing kernel
constexpr int SM_MAX_H = 1024;      // hidden / output width of a head layer

template <typename T>
__global__ void __launch_bounds__(SM_THREADS) scene_mean_partial_kernel(const T* __restrict__ x,
                                                                         const int64_t* __restrict__ offset, int nb,
                                                                         int64_t n, int c, int64_t rb,
                                                                         float* __restrict__ slab) {
  constexpr int VE = 16 / sizeof(T);   // elements per 16-byte load
  typedef float VF __attribute__((ext_vector_type(VE)));
  __shared__ float red[SM_THREADS * VE];
  const int64_t j = blockIdx.x;
  const int b = scene_of_chunk<SM_THREADS>(offset, nb, n, rb, j);
  int64_t s, e;
  scene_bounds(offset, b, n, &s, &e);
  const int64_t blk = j - b;
  int64_t r0 = blk * rb, r1 = r0 + rb;
  r0 = r0 < s ? s : r0;
  r1 = r1 > e ? e : r1;
  if (r0 >= r1) return;   // an unused id: the finishing kernel never reads its slab row
  const int vpr = c / VE, lanes = SM_THREADS / vpr;
  const int cv = (int)threadIdx.x % vpr, rl = (int)threadIdx.x / vpr;
  float acc[VE];
#pragma unroll
  for (int q = 0; q < VE; ++q) acc[q] = 0.f;
  if (rl < lanes) {
    const T* base = x + (int64_t)cv * VE;
    int64_t r = r0 + rl;
    // four 16-byte loads in flight per lane; added in row order (the same chain as a plain loop)
    for (; r + 3 * lanes < r1; r += 4 * lanes) {
      typename Vec4<T>::type v[4][VE / 4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int h = 0; h < VE / 4; ++h)
          v[u][h] = *reinterpret_cast<const typename Vec4<T>::type*>(base + (r + (int64_t)u * lanes) * c + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int h = 0; h < VE / 4; ++h) {
          float f[4];
          unpack4<T>(v[u][h], f);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[4 * h + q] += f[q];
        }
    }
    for (; r < r1; r += lanes) {
#pragma unroll
      for (int h = 0; h < VE / 4; ++h) {
        float f[4];
        unpack4<T>(*reinterpret_cast<const typename Vec4<T>::type*>(base + r * c + 4 * h), f);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[4 * h + q] += f[q];
      }
    }
  }
  // fixed tree over the row lanes
  float* mine = red + (int64_t)rl * c + cv * VE;
  if (rl < lanes) {
#pragma unroll
    for (int q = 0; q < VE; ++q) mine[q] = acc[q];
  }
  int p2 = 1;
  while (p2 < lanes) p2 <<= 1;
  for (int d = p2 >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if (rl < d && rl + d < lanes) {
      const float* other = mine + (int64_t)d * c;
#pragma unroll
      for (int q = 0; q < VE; ++q) { acc[q] += other[q]; mine[q] = acc[q]; }
    }
  }
  if (rl == 0) {
    VF o;
#pragma unroll
    for (int q = 0; q < VE; ++q) o[q] = acc[q];
    *reinterpret_cast<VF*>(slab + j * c + cv * VE) = o;
  }
}

// y[o] = act((sum_k x[k] wt[k][o] + bias[o]) * sc[o] + sh[o]) for o < outs: x in LDS, wt (K, outs) fp32 (coalesced over
// o).  P threads per output split K into contiguous slices; the slices are added in slice order (deterministic).
__device__ __forceinline__ void head_layer(const float* x, int K, const float* __restrict__ wt,
                                           const float* __restrict__ bias, const float* __restrict__ sc,
                                           const float* __restrict__ sh, int outs, bool relu, float* y, float* part) {
  const int t = threadIdx.x;
  int P = 1;
  while (P * 2 * outs <= SF_THREADS) P *= 2;
  for (int o0 = 0; o0 < outs; o0 += SF_THREADS) {        // more than one round only when outs > SF_THREADS / 2
    const int span = outs - o0 < SF_THREADS ? outs - o0 : SF_THREADS;
    const int q = t / span, o = o0 + t % span;
    if (q < P) {
      const int kc = (K + P - 1) / P, k0 = q * kc, k1 = k0 + kc < K ? k0 + kc : K;
      float a = 0.f;
#pragma unroll 16
      for (int k = k0; k < k1; ++k) a = fmaf(x[k], wt[(int64_t)k * outs + o], a);
      part[q * span + t % span] = a;
    }
    __syncthreads();
    if (t < span) {
      float a = part[t];
      for (int p = 1; p < P; ++p) a += part[p * span + t];
      a += bias[o0 + t];
      if (sc) a = a * sc[o0 + t] + sh[o0 + t];
      if (relu) a = fmaxf(a, 0.f);
      y[o0 + t] = a;
    }
    __syncthreads();
  }
}

template <bool HEAD>
__global__ void __launch_bounds__(SF_THREADS) scene_mean_finish_kernel(
    const float* __restrict__ slab, const int64_t* __restrict__ offset, int64_t n, int c, int64_t rb,
    float* __restrict__ mean_out, const float* __restrict__ w1t, const float* __restrict__ b1,
    const float* __restrict__ s1, const float* __restrict__ t1, int hidden, const float* __restrict__ w2t,
    const float* __restrict__ b2, const float* __restrict__ w3t, const float* __restrict__ b3, int out_dim,
    float* __restrict__ head_out) {
  __shared__ f32x4 red[SF_THREADS];
  __shared__ float g[SM_MAX_C], h1[SM_MAX_H], h2[SM_MAX_H], part[SF_THREADS];
  const int b = blockIdx.x;
  int64_t s, e;
  scene_bounds(offset, b, n, &s, &e);
  const int64_t first = s / rb + b, nblk = scene_nblk(s, e, rb);
  const int cv4 = c / 4, lanes = SF_THREADS / cv4;
  const int cv = (int)threadIdx.x % cv4, z = (int)threadIdx.x / cv4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (z < lanes) {
    int64_t k = z;
    for (; k + 3 * lanes < nblk; k += 4 * lanes) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(slab + (first + k + u * lanes) * c + 4 * cv);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += v[u];
    }
    for (; k < nblk; k += lanes) acc += *reinterpret_cast<const f32x4*>(slab + (first + k) * c + 4 * cv);
    red[z * cv4 + cv] = acc;
  }
  int p2 = 1;
  while (p2 < lanes) p2 <<= 1;
  for (int d = p2 >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if (z < d && z + d < lanes) {
      acc += red[(z + d) * cv4 + cv];
      red[z * cv4 + cv] = acc;
    }
  }
  if (z == 0) {
    const float cnt = (float)(e - s);
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    if (e > s) m = acc / cnt;
    if (HEAD) {
#pragma unroll
      for (int q = 0; q < 4; ++q) g[4 * cv + q] = m[q];
    } else {
      *reinterpret_cast<f32x4*>(mean_out + (int64_t)b * c + 4 * cv) = m;
    }
  }
  if (!HEAD) return;
  __syncthreads();
  head_layer(g, c, w1t, b1, s1, t1, hidden, true, h1, part);
  head_layer(h1, hidden, w2t, b2, nullptr, nullptr, hidden, true, h2, part);
  head_layer(h2, hidden, w3t, b3, nullptr, nullptr, out_dim, false, head_out + (int64_t)b * out_dim, part);
}

template <typename T>
__global__ void __launch_bounds__(SM_THREADS) scene_mean_bwd_kernel(const float* __restrict__ dg,
                                                                     const int64_t* __restrict__ offset, int nb,
                                                                     int64_t n, int c, T* __restrict__ dx) {
  constexpr int VE = 16 / sizeof(T);
  const int vpr = c / VE;
  const int64_t total = n * vpr;
  for (int64_t v = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; v < total; v += (int64_t)gridDim.x * SM_THREADS) {
    const int64_t i = v / vpr;
    const int cv = (int)(v - i * vpr);
    int lo = 0, hi = nb;   // scene = first b with offset[b] > i
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (offset[mid] > i) hi = mid; else lo = mid + 1;
    }
    float f[VE];
    if (lo < nb) {
      int64_t s, e;
      scene_bounds(offset, lo, n, &s, &e);
      const float cnt = (float)(e - s);
#pragma unroll
      for (int q = 0; q < VE; ++q) f[q] = dg[(int64_t)lo * c + cv * VE + q] / cnt;
    } else {
#pragma unroll
      for (int q = 0; q < VE; ++q) f[q] = 0.f;   // rows past offset[B-1]: no scene
    }
#pragma unroll
    for (int h = 0; h < VE / 4; ++h)
      *reinterpret_cast<typename Vec4<T>::type*>(dx + i * c + cv * VE + 4 * h) =
          pack4<T>(f[4 * h], f[4 * h + 1], f[4 * h + 2], f[4 * h + 3]);
  }
}

int64_t scene_rows_per_chunk(int64_t n) {
  // ~1024 chunks at any size (4 partial workgroups per CU); at least 64 rows so a chunk is worth a workgroup
  int64_t r = cdiv(cdiv(n, 1024), 16) * 16;
  return r < 64 ? 64 : r;
}
static int64_t scene_chunks(int64_t n, int b) { return cdiv(n, scene_rows_per_chunk(n)) + b; }

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int scene_mean_check(const char* who, const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype,
                            void* workspace, size_t workspace_bytes) {
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "%s: dtype %d (0 = fp32, 1 = bf16)", who, dtype);
  PTV3_REQUIRE(n >= 0 && b >= 0, "%s: bad shape n=%lld b=%d", who, (long long)n, b);
  PTV3_REQUIRE(c >= 8 && c <= SM_MAX_C && c % 8 == 0, "%s: c=%d unsupported (multiple of 8 in [8, %d])", who, c,
               SM_MAX_C);
  PTV3_REQUIRE(b == 0 || offset, "%s: offset is NULL", who);
  PTV3_REQUIRE(n == 0 || (feat && aligned16(feat)), "%s: feat must be 16-byte aligned", who);
  PTV3_REQUIRE(b == 0 || (workspace && aligned16(workspace)), "%s: workspace must be 16-byte aligned", who);
  PTV3_REQUIRE(workspace_bytes >= (size_t)scene_chunks(n, b) * c * sizeof(float), "%s: workspace too small", who);
  return PTV3_OK;
}

void scene_mean_partial(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype, float* slab,
                        hipStream_t s) {
  const int64_t rb = scene_rows_per_chunk(n);
  const dim3 grid((unsigned)scene_chunks(n, b));
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(scene_mean_partial_kernel<T>, grid, dim3(SM_THREADS), 0, s, (const T*)feat, offset, b, n, c, rb,
                       slab);
  });
}

}  // namespace ptv3

using namespace ptv3;

extern "C" size_t ptv3_scene_mean_workspace_bytes(int64_t n, int c, int b) {
  return (size_t)scene_chunks(n < 0 ? 0 : n, b < 0 ? 0 : b) * (c < 0 ? 0 : c) * sizeof(float);
}

extern "C" int ptv3_scene_mean(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype, float* out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = scene_mean_check("scene_mean", feat, offset, n, c, b, dtype, workspace, workspace_bytes);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(b == 0 || (out && aligned16(out)), "scene_mean: out must be 16-byte aligned");
  if (b == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  scene_mean_partial(feat, offset, n, c, b, dtype, (float*)workspace, s);
  hipLaunchKernelGGL(scene_mean_finish_kernel<false>, dim3((unsigned)b), dim3(SF_THREADS), 0, s,
                     (const float*)workspace, offset, n, c, scene_rows_per_chunk(n), out, nullptr, nullptr, nullptr,
                     nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_scene_mean_head(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype,
                                    const float* w1t, const float* b1, const float* s1, const float* t1, int hidden,
                                    const float* w2t, const float* b2, const float* w3t, const float* b3, int out_dim,
                                    float* out, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = scene_mean_check("scene_mean_head", feat, offset, n, c, b, dtype, workspace, workspace_bytes);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(hidden >= 1 && hidden <= SM_MAX_H && out_dim >= 1 && out_dim <= SM_MAX_H,
               "scene_mean_head: hidden=%d / out_dim=%d unsupported (each in [1, %d])", hidden, out_dim, SM_MAX_H);
  PTV3_REQUIRE(w1t && b1 && s1 && t1 && w2t && b2 && w3t && b3, "scene_mean_head: a head parameter is NULL");
  PTV3_REQUIRE(b == 0 || out, "scene_mean_head: out is NULL");
  if (b == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  scene_mean_partial(feat, offset, n, c, b, dtype, (float*)workspace, s);
  hipLaunchKernelGGL(scene_mean_finish_kernel<true>, dim3((unsigned)b), dim3(SF_THREADS), 0, s, (const float*)workspace,
                     offset, n, c, scene_rows_per_chunk(n), nullptr, w1t, b1, s1, t1, hidden, w2t, b2, w3t, b3, out_dim,
                     out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_scene_mean_bwd(const float* dg, const int64_t* offset, int64_t n, int c, int b, void* dfeat,
                                   int dtype, void* stream) {
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "scene_mean_bwd: dtype %d (0 = fp32, 1 = bf16)", dtype);
  PTV3_REQUIRE(n >= 0 && b >= 0, "scene_mean_bwd: bad shape n=%lld b=%d", (long long)n, b);
  PTV3_REQUIRE(c >= 8 && c <= SM_MAX_C && c % 8 == 0, "scene_mean_bwd: c=%d unsupported (multiple of 8 in [8, %d])", c,
               SM_MAX_C);
  PTV3_REQUIRE(n == 0 || (dfeat && aligned16(dfeat)), "scene_mean_bwd: dfeat must be 16-byte aligned");
  PTV3_REQUIRE(n == 0 || b == 0 || (dg && offset), "scene_mean_bwd: dg / offset is NULL");
  if (n == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t items = n * (c / dtype_granule(dtype));
  int64_t blocks = cdiv(items, SM_THREADS);
  if (blocks > 2048) blocks = 2048;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(scene_mean_bwd_kernel<T>, dim3((unsigned)blocks), dim3(SM_THREADS), 0, s, dg, offset, b, n, c,
                       (T*)dfeat);
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
