// Row chunks that never straddle a scene: shared by the per-scene reductions (global_head.hip, vote_head.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptv3 {

// Rows of scene b, clamped into [0, n]: a malformed offset vector yields wrong numbers, never an access outside feat.
__device__ __forceinline__ void scene_bounds(const int64_t* __restrict__ offset, int b, int64_t n, int64_t* s,
                                             int64_t* e) {
  int64_t lo = b ? offset[b - 1] : 0, hi = offset[b];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  *s = lo;
  *e = hi;
}

// Chunk ids: the rows are cut at multiples of rb AND at scene boundaries.  Scene b owns the ids
// [s_b / rb + b, s_b / rb + b + nblk_b) with nblk_b = number of rb-blocks its rows touch; the ids of successive scenes
// are increasing and disjoint (an empty scene or a scene ending on a multiple of rb leaves one unused id), and every
// id is < cdiv(n, rb) + B.  So the host sizes the grid from n and B alone; nothing is read back.
__device__ __forceinline__ int64_t scene_nblk(int64_t s, int64_t e, int64_t rb) { return e > s ? (e - 1) / rb - s / rb + 1 : 0; }

// Scene of chunk id j = #{b >= 1 : first id of b <= j} (the first ids increase with b).  Called by every thread of a
// THREADS-wide workgroup (it synchronises).
template <int THREADS>
__device__ __forceinline__ int scene_of_chunk(const int64_t* __restrict__ offset, int nb, int64_t n, int64_t rb,
                                              int64_t j) {
  int b = 0;
  for (int b0 = 0; b0 < nb; b0 += THREADS) {
    const int q = b0 + (int)threadIdx.x;
    int hit = 0;
    if (q >= 1 && q < nb) {
      int64_t s, e;
      scene_bounds(offset, q, n, &s, &e);
      hit = s / rb + q <= j;
    }
    b += __syncthreads_count(hit);
  }
  return b;
}

// The rows [r0, r1) of chunk j of scene b (empty for an unused id).
__device__ __forceinline__ void chunk_rows(int64_t j, int b, int64_t s, int64_t e, int64_t rb, int64_t* r0,
                                           int64_t* r1) {
  int64_t lo = (j - b) * rb, hi = lo + rb;
  *r0 = lo < s ? s : lo;
  *r1 = hi > e ? e : hi;
}

// The pooling partials (global_head.hip), shared with the classifier head (cls_head.hip): rows per chunk for n rows,
// and the launch of scene_mean_partial_kernel - one fp32 slab row (c floats) per chunk id into `slab`, which holds
// ptv3_scene_mean_workspace_bytes(n, c, b).  The caller has checked the arguments (scene_mean_check's conditions).
int64_t scene_rows_per_chunk(int64_t n);
void scene_mean_partial(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype, float* slab,
                        hipStream_t s);

}  // namespace ptv3
