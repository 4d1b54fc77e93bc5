// Grid pooling of Point Transformer V2 (GridPool.forward, point_transformer_v2m2_base.py:251-276): the cell key of every
// point from its float coordinate, and the per-cluster coordinate mean.  ptv3_argsort_i64 + ptv3_pool_segments turn the
// key into order / segments / cluster ids / pooled offsets, ptv3_pool_reduce's feature half takes the per-cluster max.
// Beside ptv3_cluster_keys (oacnns.hip), which keys integer voxel indices; here the cell comes from fp32 arithmetic:
//   start[b] = per-axis minimum of scene b (segment_csr(coord, ptr, "min"))
//   cell     = (int64)((coord - start[b]) / size)   one fp32 subtraction, one correctly rounded fp32 division
//   key      = b << 51 | cz << 34 | cy << 17 | cx   sorts by (b, cz, cy, cx): the rank torch.unique gives voxel_grid's ids
#include <float.h>

#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int GK_THREADS = 256;
constexpr int GK_CELL_BITS = 17;
constexpr int GK_MAX_SCENES = 4096;

// one workgroup per scene; a minimum does not depend on the order it is taken in
__global__ void __launch_bounds__(GK_THREADS) grid_scene_min_kernel(const float* __restrict__ coord,
                                                                    const int64_t* __restrict__ offset, int64_t n,
                                                                    float* __restrict__ start) {
  __shared__ float sm[3][GK_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t s0 = max((int64_t)0, b ? offset[b - 1] : 0), s1 = min(offset[b], n);   // never past the coordinates
  float mx = FLT_MAX, my = FLT_MAX, mz = FLT_MAX;
  for (int64_t i = s0 + tid; i < s1; i += GK_THREADS) {
    mx = fminf(mx, coord[3 * i]);
    my = fminf(my, coord[3 * i + 1]);
    mz = fminf(mz, coord[3 * i + 2]);
  }
  sm[0][tid] = mx; sm[1][tid] = my; sm[2][tid] = mz;
  __syncthreads();
  for (int w = GK_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w)
      for (int a = 0; a < 3; ++a) sm[a][tid] = fminf(sm[a][tid], sm[a][tid + w]);
    __syncthreads();
  }
  if (tid < 3) start[3 * b + tid] = sm[tid][0];
}

__global__ void __launch_bounds__(GK_THREADS) grid_keys_kernel(const float* __restrict__ coord, int64_t n,
                                                               const int64_t* __restrict__ offset, int nb, float size,
                                                               const float* __restrict__ start,
                                                               int64_t* __restrict__ key, int64_t* __restrict__ batch,
                                                               int64_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * GK_THREADS + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = nb - 1;   // first scene whose end lies past i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offset[mid] > i) hi = mid; else lo = mid + 1;
  }
  int64_t k = lo;
  bool out = false;
#pragma unroll
  for (int a = 2; a >= 0; --a) {
    const float d = coord[3 * i + a] - start[3 * lo + a];
    int64_t cell = (int64_t)__fdiv_rn(d, size);
    if (!(cell >= 0 && cell < (1ll << GK_CELL_BITS))) { out = true; cell = 0; }
    k = (k << GK_CELL_BITS) | cell;
  }
  key[i] = k;
  batch[i] = lo;
  if (out) *bad = 1;   // every writer stores the same value
}

__global__ void __launch_bounds__(GK_THREADS) segment_mean3_kernel(const float* __restrict__ coord,
                                                                   const int64_t* __restrict__ order,
                                                                   const int32_t* __restrict__ seg_start, int64_t n_out,
                                                                   float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * GK_THREADS + threadIdx.x;
  if (j >= n_out) return;
  const int s0 = seg_start[j], s1 = seg_start[j + 1];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int p = s0; p < s1; ++p) {   // members in sorted order, as segment_csr sums them
    const int64_t r = order[p];
    sx += coord[3 * r]; sy += coord[3 * r + 1]; sz += coord[3 * r + 2];
  }
  const float cnt = (float)(s1 - s0);
  out[3 * j] = sx / cnt; out[3 * j + 1] = sy / cnt; out[3 * j + 2] = sz / cnt;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_grid_keys(const float* coord, int64_t n, const int64_t* offset, int num_scenes, float size,
                              float* start, int64_t* key, int64_t* batch, int64_t* bad, void* stream) {
  PTV3_REQUIRE(size > 0.f && size <= FLT_MAX, "grid_keys: size=%g must be positive and finite", (double)size);
  PTV3_REQUIRE(num_scenes >= 1 && num_scenes <= GK_MAX_SCENES, "grid_keys: %d scenes outside [1, %d]", num_scenes,
               GK_MAX_SCENES);
  PTV3_REQUIRE(n >= 0 && n <= 0x7fffffff, "grid_keys: n=%lld outside [0, 2^31)", (long long)n);
  if (n == 0) return PTV3_OK;
  PTV3_REQUIRE(coord && offset && start && key && batch && bad, "grid_keys: a NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grid_scene_min_kernel, dim3(num_scenes), dim3(GK_THREADS), 0, s, coord, offset, n, start);
  hipLaunchKernelGGL(grid_keys_kernel, dim3((unsigned)cdiv(n, GK_THREADS)), dim3(GK_THREADS), 0, s, coord, n, offset,
                     num_scenes, size, start, key, batch, bad);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_segment_mean3(const float* coord, const int64_t* order, const int32_t* seg_start, int64_t n_out,
                                  float* out, void* stream) {
  PTV3_REQUIRE(n_out >= 0 && n_out <= 0x7fffffff, "segment_mean3: n_out=%lld outside [0, 2^31)", (long long)n_out);
  if (n_out == 0) return PTV3_OK;
  PTV3_REQUIRE(coord && order && seg_start && out, "segment_mean3: a NULL tensor");
  hipLaunchKernelGGL(segment_mean3_kernel, dim3((unsigned)cdiv(n_out, GK_THREADS)), dim3(GK_THREADS), 0,
                     (hipStream_t)stream, coord, order, seg_start, n_out, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
