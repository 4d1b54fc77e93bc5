// libs/pointops farthest point sampling (sampling/sampling_cuda_kernel.cu:15-129) for gfx950.
// One workgroup per scene; the scene's selections are a dependent chain, so the cost is the latency of ONE selection:
//   * every thread owns the points k = tid, tid + T, ... of its scene.  The first T * P of them (coordinates and running
//     distance) live in registers for the whole kernel, the next `lds_cap` in LDS, whatever is left stays in global
//     memory (coordinates read through the caches, `tmp` read and written in place);
//   * a thread's best (distance, index) is reduced over its wave with DPP row shifts / broadcasts on the distance bits
//     alone (distances are >= 0, so their bits order as unsigned integers), a ballot then names the lane that holds it;
//   * that lane posts (distance, index, x, y, z) to one of two LDS exchange buffers, ONE barrier, and every wave
//     reduces the <= 16 posted entries the same way and reads the winner's coordinates out of the entry - no second
//     barrier and no global load sits between two selections.
// Two deliberate differences from the reference:
//   * ties go to the LOWEST index at every level (strict `>` in ascending index order inside a thread, lowest index
//     among equal lanes / waves), where the reference's tie order depends on its block size; the result therefore does
//     not depend on T or P, is bitwise reproducible, and a scene of identical points returns its first index repeated;
//   * a scene asked for zero samples writes nothing (the reference writes idx[start_m] regardless, which lands in the
//     next scene's slot or past the end).
// No workgroup waits for another one.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int FPS_REG_POINTS = 16;      // points per thread kept in registers by the large variant
constexpr int FPS_LDS_POINTS = 8192;    // points of one scene kept in LDS behind the registers (16 B each)
constexpr int FPS_XCH_FLOATS = 2 * 16 * 8;

// (x2 - x1)^2 + (y2 - y1)^2 + (z2 - z1)^2 as one product and two fused multiply-adds (the reference's nvcc contracts
// its expression the same way); three instructions instead of five in a loop that is bound by the vector ALU.
// Two register slots per v_pk_fma_f32 were measured slower (12.8 against 11.4 ms for 8 x 20 000 -> 5000 points).
__device__ __forceinline__ float fps_dist2(float x1, float y1, float z1, float x2, float y2, float z2) {
  const float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_umax_step(unsigned v) {
  // lanes without a source (row edge, masked row) keep `old` = v, and max(v, v) = v
  const unsigned t = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
  return v > t ? v : t;
}
// after this lane 15 of every 16-lane row holds the row's maximum
__device__ __forceinline__ unsigned row_umax(unsigned v) {
  v = dpp_umax_step<0x111, 0xf>(v);   // row_shr:1
  v = dpp_umax_step<0x112, 0xf>(v);   // row_shr:2
  v = dpp_umax_step<0x114, 0xf>(v);   // row_shr:4
  v = dpp_umax_step<0x118, 0xf>(v);   // row_shr:8
  return v;
}
// maximum over the 64 lanes, as a wave-uniform value
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
  v = row_umax(v);
  v = dpp_umax_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_umax_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// the lane, among those in `mask`, whose index is lowest (mask != 0; wave-uniform)
__device__ __forceinline__ int lowest_index_lane(unsigned long long mask, int index) {
  int lane = __ffsll((long long)mask) - 1;
  mask &= mask - 1;
  if (mask == 0) return lane;   // the common case: one holder of the maximum
  int best = __builtin_amdgcn_readlane(index, lane);
  while (mask) {
    const int l = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int i = __builtin_amdgcn_readlane(index, l);
    if (i < best) { best = i; lane = l; }
  }
  return lane;
}

// key of a candidate: distance bits + 1, so that 0 stays below every real candidate (a zero distance included)
#define FPS_OFFER(kk, xx, yy, zz, dd)                                        \
  do {                                                                       \
    const unsigned key__ = __float_as_uint(dd) + 1u;                         \
    if (key__ > bkey) { bkey = key__; bidx = (kk); bx = (xx); by = (yy); bz = (zz); } \
  } while (0)

template <int T, int P>
__global__ void __launch_bounds__(T)
fps_kernel(const float* __restrict__ xyz, const int* __restrict__ offset, const int* __restrict__ new_offset,
           float* __restrict__ tmp, int* __restrict__ idx, int lds_cap) {
  extern __shared__ __attribute__((aligned(16))) float fps_smem[];
  constexpr int W = T / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = blockIdx.x;
  const int start_n = bid ? offset[bid - 1] : 0, end_n = offset[bid];
  const int start_m = bid ? new_offset[bid - 1] : 0, end_m = new_offset[bid];
  const int n = end_n - start_n, m = end_m - start_m;
  if (m <= 0 || n <= 0) return;   // block-uniform; a scene asked for nothing writes nothing

  float* xch = fps_smem;                       // [2][16][8]: key, index, x, y, z
  float* lx = fps_smem + FPS_XCH_FLOATS;       // [lds_cap] each
  float* ly = lx + lds_cap;
  float* lz = ly + lds_cap;
  float* ld = lz + lds_cap;
  const float* __restrict__ p = xyz + 3 * (int64_t)start_n;
  float* __restrict__ t = tmp + start_n;
  const int nl = min(max(n - T * P, 0), lds_cap);   // points held in LDS
  const int g0 = T * P + nl;                        // first point left in global memory

  float rx[P], ry[P], rz[P], rd[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const int k = tid + q * T;
    const bool v = k < n;
    rx[q] = v ? p[3 * k] : 0.f; ry[q] = v ? p[3 * k + 1] : 0.f; rz[q] = v ? p[3 * k + 2] : 0.f;
    rd[q] = v ? t[k] : 0.f;
  }
  // an LDS slot is only ever touched by the thread that owns it: no barrier
  for (int k = tid; k < nl; k += T) {
    const int g = T * P + k;
    lx[k] = p[3 * g]; ly[k] = p[3 * g + 1]; lz[k] = p[3 * g + 2]; ld[k] = t[g];
  }
  if (tid == 0) idx[start_m] = start_n;
  float ox = p[0], oy = p[1], oz = p[2];

  for (int j = 1; j < m; ++j) {
    unsigned bkey = 0u;
    int bidx = 0x7fffffff;
    float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int k = tid + q * T;
      if (k < n) {
        const float d = fminf(fps_dist2(ox, oy, oz, rx[q], ry[q], rz[q]), rd[q]);
        rd[q] = d;
        FPS_OFFER(k, rx[q], ry[q], rz[q], d);
      }
    }
    for (int k = tid; k < nl; k += T) {
      const float x = lx[k], y = ly[k], z = lz[k];
      const float d = fminf(fps_dist2(ox, oy, oz, x, y, z), ld[k]);
      ld[k] = d;
      FPS_OFFER(T * P + k, x, y, z, d);
    }
    // global tier: three points' loads in flight at a time - the store to tmp would otherwise order every load behind
    // it, and a fourth point spills registers; tmp is written only where it shrinks, which after the first selections
    // is a small part of the scene
    int k = g0 + tid;
    for (; k + 2 * T < n; k += 3 * T) {
      float x[3], y[3], z[3], d[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int kk = k + u * T;
        x[u] = p[3 * kk]; y[u] = p[3 * kk + 1]; z[u] = p[3 * kk + 2]; d[u] = t[kk];
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const float dn = fps_dist2(ox, oy, oz, x[u], y[u], z[u]);
        if (dn < d[u]) { d[u] = dn; t[k + u * T] = dn; }
        FPS_OFFER(k + u * T, x[u], y[u], z[u], d[u]);
      }
    }
    for (; k < n; k += T) {
      const float x = p[3 * k], y = p[3 * k + 1], z = p[3 * k + 2];
      const float d = fminf(fps_dist2(ox, oy, oz, x, y, z), t[k]);
      t[k] = d;
      FPS_OFFER(k, x, y, z, d);
    }
    // the wave's best candidate -> its slot of this selection's exchange buffer
    const unsigned wkey = wave_umax(bkey);
    int wl = 0;
    if (wkey != 0u) wl = lowest_index_lane(__ballot(bkey == wkey), bidx);
    float* slot = xch + ((j & 1) * 16 + wave) * 8;
    if (lane == wl) {
      ((unsigned*)slot)[0] = bkey; ((int*)slot)[1] = bidx;
      slot[2] = bx; slot[3] = by; slot[4] = bz;
    }
    __syncthreads();
    // every wave reduces the W posted entries (lane e < W holds entry e)
    const float* ent = xch + ((j & 1) * 16 + (lane & (W - 1))) * 8;
    const bool have = lane < W;
    const unsigned ekey = have ? ((const unsigned*)ent)[0] : 0u;
    const int eidx = have ? ((const int*)ent)[1] : 0x7fffffff;
    const float ex = ent[2], ey = ent[3], ez = ent[4];
    const unsigned top = (unsigned)__builtin_amdgcn_readlane((int)row_umax(ekey), 15);
    const int el = lowest_index_lane(__ballot(have && ekey == top), eidx);   // top != 0: n >= 1
    const int old = __builtin_amdgcn_readlane(eidx, el);
    ox = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex), el));
    oy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ey), el));
    oz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ez), el));
    if (tid == 0) idx[start_m + j] = start_n + old;
  }

#pragma unroll
  for (int q = 0; q < P; ++q) {
    const int k = tid + q * T;
    if (k < n) t[k] = rd[q];
  }
  for (int k = tid; k < nl; k += T) t[T * P + k] = ld[k];
}
#undef FPS_OFFER

template <int T, int P>
static int fps_launch(int b, int lds_points, const float* xyz, const int* offset, const int* new_offset, float* tmp,
                      int* idx, hipStream_t s) {
  const int bytes = (FPS_XCH_FLOATS + 4 * lds_points) * (int)sizeof(float);
  ensure_dynamic_lds((const void*)fps_kernel<T, P>, bytes);
  hipLaunchKernelGGL((fps_kernel<T, P>), dim3((unsigned)b), dim3(T), bytes, s, xyz, offset, new_offset, tmp, idx,
                     lds_points);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_farthest_point_sampling(int b, int n_max, const float* xyz, const int* offset,
                                            const int* new_offset, float* tmp, int* idx, void* stream) {
  PTV3_REQUIRE(b >= 1, "farthest_point_sampling: b=%d scenes (at least 1)", b);
  PTV3_REQUIRE(n_max >= 0, "farthest_point_sampling: n_max=%d is negative", n_max);
  PTV3_REQUIRE(xyz && offset && new_offset && tmp && idx, "farthest_point_sampling: a NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  // n_max picks where a scene's state lives; a scene larger than n_max says is still sampled correctly (its tail
  // runs out of global memory)
  if (n_max <= 256) return fps_launch<256, 1>(b, 0, xyz, offset, new_offset, tmp, idx, s);
  if (n_max <= 1024) return fps_launch<1024, 1>(b, 0, xyz, offset, new_offset, tmp, idx, s);
  if (n_max <= 4096) return fps_launch<1024, 4>(b, 0, xyz, offset, new_offset, tmp, idx, s);
  const int over = n_max - 1024 * FPS_REG_POINTS;
  const int lds_points = over <= 0 ? 0 : (over < FPS_LDS_POINTS ? over : FPS_LDS_POINTS);
  return fps_launch<1024, FPS_REG_POINTS>(b, lds_points, xyz, offset, new_offset, tmp, idx, s);
}
