// Voting keypoint head (KeypointSwin3DVote): per-scene column median of the per-point votes, and the masked
// smooth-L1 vote loss with its backward.
//   median_pass_kernel<P>    pass P of an exact radix select on an order-preserving 32-bit key, 8 bits per pass: one
//                            256-bin histogram per (scene, column) of the rows whose higher digits equal the median's,
//                            built in LDS per row chunk and merged with global INTEGER atomics (order-independent)
//   median_finish_kernel     one workgroup per scene: the four digits of each column's median -> the value itself
//   vote_loss_partial_kernel fixed row chunks -> one slab row (loss, distance, count per keypoint) per chunk
//   vote_loss_finish_kernel  the slabs summed in a fixed order (float64, integer counts) -> loss and curves
//   vote_loss_bwd_kernel     dvotes = dloss * mask * clamp(diff, -1, 1) / (3 * max(count, 1)), the mask recomputed
// Pass P + 1 re-derives (prefix, remaining rank) of every column from the histograms of passes 0..P, so every hand-off
// between workgroups is a kernel boundary: no tickets, no flags, no float atomics; two runs are bitwise equal.
// Row chunks never straddle a scene (scene_chunks.h); grids are sized from n and B alone, nothing is read back.
#include "common.h"
#include "scene_chunks.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int VH_THREADS = 256;
constexpr int VH_WAVES = VH_THREADS / 64;
constexpr int VH_MAX_C = 32;          // columns of a median call (the fork: 3K = 18)
constexpr int VH_MAX_K = 32;          // keypoints of a loss call
constexpr int VH_BINS = 256;          // 8-bit digits, four passes
constexpr int VH_LDS_STRIDE = VH_BINS + 1;   // column histograms on different banks

// Ascending float order as ascending unsigned order: non-negatives get the sign bit set, negatives are inverted
// (-0 < +0, which torch.median cannot tell apart either).  NaN sorts last (torch.median: NaN wins) and is counted.
__device__ __forceinline__ uint32_t median_key(float v, bool* is_nan) {
  const uint32_t u = __float_as_uint(v);
  *is_nan = (u & 0x7fffffffu) > 0x7f800000u;
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return *is_nan ? 0xffffffffu : k;
}
__device__ __forceinline__ float median_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Global histograms: hist[((p * B + b) * C + col) * 256 + digit], then nan[b * C + col].
__device__ __forceinline__ size_t hist_at(int p, int nb, int b, int c, int col) {
  return (((size_t)p * nb + b) * c + col) * VH_BINS;
}

// (prefix, remaining rank) of every column of scene b after passes [0, P): one wave per column, four bins per lane,
// a wave scan per pass.  All 4 * P loads of a column are issued before the first scan (they do not depend on it).
template <int P>
__device__ __forceinline__ void median_derive(const uint32_t* hist, int nb, int b, int c, uint32_t rank0,
                                              uint32_t* s_prefix, uint32_t* s_rank) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int col = wave; col < c; col += VH_WAVES) {
    uint4 h[P];
#pragma unroll
    for (int q = 0; q < P; ++q) h[q] = *reinterpret_cast<const uint4*>(hist + hist_at(q, nb, b, c, col) + 4 * lane);
    uint32_t prefix = 0, rank = rank0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const uint32_t s0 = h[q].x, s1 = s0 + h[q].y, s2 = s1 + h[q].z, s3 = s2 + h[q].w;
      uint32_t incl = s3;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      const uint32_t excl = incl - s3;
      const unsigned long long owner = __ballot(excl <= rank && rank < incl);
      const int src = owner ? __ffsll((long long)owner) - 1 : 63;   // a rank past the total cannot happen; stay defined
      const uint32_t r = rank - excl;
      const int sub = r < s0 ? 0 : (r < s1 ? 1 : (r < s2 ? 2 : 3));
      const uint32_t below = sub == 0 ? 0 : (sub == 1 ? s0 : (sub == 2 ? s1 : s2));
      const uint32_t digit = __shfl((uint32_t)(4 * lane + sub), src);
      rank = __shfl(r - below, src);
      prefix = (prefix << 8) | digit;
    }
    if (lane == 0) { s_prefix[col] = prefix; s_rank[col] = rank; }
  }
}

template <int P>
__global__ void __launch_bounds__(VH_THREADS) median_pass_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ coord,
                                                                  const int64_t* __restrict__ offset, int nb, int64_t n,
                                                                  int c, int64_t rb, uint32_t* hist) {
  __shared__ uint32_t lh[VH_MAX_C * VH_LDS_STRIDE];
  __shared__ uint32_t s_prefix[VH_MAX_C], s_rank[VH_MAX_C], s_nan[VH_MAX_C];
  const int t = (int)threadIdx.x;
  const int64_t j = blockIdx.x;
  const int b = scene_of_chunk<VH_THREADS>(offset, nb, n, rb, j);
  int64_t s, e, r0, r1;
  scene_bounds(offset, b, n, &s, &e);
  chunk_rows(j, b, s, e, rb, &r0, &r1);
  if (r0 >= r1) return;   // an unused id (uniform over the workgroup)
  for (int i = t; i < c * VH_LDS_STRIDE; i += VH_THREADS) lh[i] = 0;
  if (t < VH_MAX_C) s_nan[t] = 0;
  if (P > 0) median_derive<(P > 0 ? P : 1)>(hist, nb, b, c, (uint32_t)((e - s - 1) / 2), s_prefix, s_rank);
  __syncthreads();
  // Thread t keeps column t % c for the whole chunk (the first (256 / c) * c threads work; the accesses stay
  // contiguous), and counts RUNS of equal digits in registers: votes for one keypoint cluster, so the sign / exponent
  // digits are the same for almost every row, and one LDS atomic per element would serialise on one address.
  const int rows_it = VH_THREADS / c;
  if (t < rows_it * c) {
    const int col = t % c, cc = col % 3;
    const uint32_t prefix = P > 0 ? s_prefix[col] : 0;
    uint32_t* mine = lh + col * VH_LDS_STRIDE;
    uint32_t run_digit = 0, run_cnt = 0, nan_cnt = 0;
    auto take = [&](float v) {
      bool is_nan;
      const uint32_t key = median_key(v, &is_nan);
      if (P == 0) nan_cnt += is_nan;
      if (P == 0 || (key >> (32 - 8 * (P > 0 ? P : 1))) == prefix) {
        const uint32_t d = (key >> (24 - 8 * P)) & 255u;
        if (d == run_digit) {
          ++run_cnt;
        } else {
          if (run_cnt) atomicAdd(mine + run_digit, run_cnt);
          run_digit = d;
          run_cnt = 1;
        }
      }
    };
    int64_t r = r0 + t / c;
    for (; r + 3 * rows_it < r1; r += 4 * rows_it) {   // four loads in flight per lane
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = x[(r + (int64_t)u * rows_it) * c + col];
      if (coord) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] += coord[(r + (int64_t)u * rows_it) * 3 + cc];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) take(v[u]);
    }
    for (; r < r1; r += rows_it) {
      float v = x[r * c + col];
      if (coord) v += coord[r * 3 + cc];
      take(v);
    }
    if (run_cnt) atomicAdd(mine + run_digit, run_cnt);
    if (P == 0 && nan_cnt) atomicAdd(s_nan + col, nan_cnt);
  }
  __syncthreads();
  uint32_t* gh = hist + hist_at(P, nb, b, c, 0);
  for (int i = t; i < c * VH_BINS; i += VH_THREADS) {
    const uint32_t v = lh[(i >> 8) * VH_LDS_STRIDE + (i & 255)];
    if (v) atomicAdd(gh + i, v);
  }
  if (P == 0 && t < c && s_nan[t]) atomicAdd(hist + hist_at(4, nb, 0, c, 0) + (size_t)b * c + t, s_nan[t]);
}

__global__ void __launch_bounds__(VH_THREADS) median_finish_kernel(const uint32_t* __restrict__ hist,
                                                                    const int64_t* __restrict__ offset, int nb,
                                                                    int64_t n, int c, float* __restrict__ out) {
  __shared__ uint32_t s_prefix[VH_MAX_C], s_rank[VH_MAX_C];
  const int b = blockIdx.x, t = (int)threadIdx.x;
  int64_t s, e;
  scene_bounds(offset, b, n, &s, &e);
  if (e <= s) {   // an empty scene: zeros
    if (t < c) out[(int64_t)b * c + t] = 0.f;
    return;
  }
  median_derive<4>(hist, nb, b, c, (uint32_t)((e - s - 1) / 2), s_prefix, s_rank);
  __syncthreads();
  if (t < c) {
    const uint32_t nans = hist[hist_at(4, nb, 0, c, 0) + (size_t)b * c + t];
    out[(int64_t)b * c + t] = nans ? __uint_as_float(0x7fc00000u) : median_unkey(s_prefix[t]);
  }
}

// ---- vote loss --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float smooth_l1(float d) {
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

// Slab row of a chunk: loss[K], scaled distance[K], count[K] (integer bits).  Thread t keeps keypoint t % K.
__global__ void __launch_bounds__(VH_THREADS) vote_loss_partial_kernel(
    const float* __restrict__ votes, const float* __restrict__ coord, const float* __restrict__ target,
    int target_per_point, const int64_t* __restrict__ offset, int nb, const float* __restrict__ scale,
    int scale_per_point, int64_t n, int K, int64_t rb, float radius, float* __restrict__ slab) {
  __shared__ float red_l[VH_THREADS], red_d[VH_THREADS];
  __shared__ int red_c[VH_THREADS];
  const int t = (int)threadIdx.x;
  const int64_t j = blockIdx.x;
  const int b = scene_of_chunk<VH_THREADS>(offset, nb, n, rb, j);
  int64_t s, e, r0, r1;
  scene_bounds(offset, b, n, &s, &e);
  chunk_rows(j, b, s, e, rb, &r0, &r1);
  float* row = slab + j * 3 * K;
  if (r0 >= r1) {   // an unused id: a zero row, so the finishing kernel can add every row
    if (t < 3 * K) row[t] = 0.f;
    return;
  }
  const int lanes = VH_THREADS / K, kk = t % K, rl = t / K;
  float ls = 0.f, ds = 0.f;
  int cnt = 0;
  if (rl < lanes) {
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (!target_per_point) {
      const float* tp = target + ((int64_t)b * K + kk) * 3;
      tx = tp[0]; ty = tp[1]; tz = tp[2];
    }
    const float sc = (scale && !scale_per_point) ? scale[b] : 1.f;
    for (int64_t r = r0 + rl; r < r1; r += lanes) {
      const float cx = coord[r * 3], cy = coord[r * 3 + 1], cz = coord[r * 3 + 2];
      if (target_per_point) {
        const float* tp = target + (r * K + kk) * 3;
        tx = tp[0]; ty = tp[1]; tz = tp[2];
      }
      const float dx = cx - tx, dy = cy - ty, dz = cz - tz;
      const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
      if (dist < radius) {
        const float* vp = votes + (r * K + kk) * 3;
        const float ex = (cx + vp[0]) - tx, ey = (cy + vp[1]) - ty, ez = (cz + vp[2]) - tz;
        ls += (smooth_l1(ex) + smooth_l1(ey) + smooth_l1(ez)) / 3.f;
        ds += dist * (scale_per_point ? scale[r] : sc);
        ++cnt;
      }
    }
    red_l[t] = ls; red_d[t] = ds; red_c[t] = cnt;
  }
  // fixed tree over the row lanes of one keypoint
  int p2 = 1;
  while (p2 < lanes) p2 <<= 1;
  for (int d = p2 >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if (rl < d && rl + d < lanes) {
      ls += red_l[t + d * K]; ds += red_d[t + d * K]; cnt += red_c[t + d * K];
      red_l[t] = ls; red_d[t] = ds; red_c[t] = cnt;
    }
  }
  if (rl == 0) {
    row[kk] = ls;
    row[K + kk] = ds;
    row[2 * K + kk] = __int_as_float(cnt);
  }
}

// out[0] = loss, out[1] = train/masked_dist_err, out[2 + k] = train/kp{k}_dist_err; count[0] = mask total, count[1 + k].
__global__ void __launch_bounds__(VH_THREADS) vote_loss_finish_kernel(const float* __restrict__ slab, int64_t chunks,
                                                                       int K, float* __restrict__ out,
                                                                       int32_t* __restrict__ count) {
  __shared__ double red[VH_THREADS];
  __shared__ long long redc[VH_THREADS];
  const int t = (int)threadIdx.x, w = 3 * K, lanes = VH_THREADS / w, col = t % w, z = t / w;
  const bool is_count = col >= 2 * K;
  double acc = 0.0;
  long long acc_c = 0;
  if (z < lanes) {
    for (int64_t k = z; k < chunks; k += lanes) {
      const float v = slab[k * w + col];
      if (is_count) acc_c += __float_as_int(v); else acc += (double)v;
    }
    red[t] = acc; redc[t] = acc_c;
  }
  __syncthreads();
  if (t == 0) {
    double loss = 0.0, dist = 0.0;
    long long total = 0;
    for (int k = 0; k < K; ++k) {
      double lk = 0.0, dk = 0.0;
      long long ck = 0;
      for (int q = 0; q < lanes; ++q) { lk += red[q * w + k]; dk += red[q * w + K + k]; ck += redc[q * w + 2 * K + k]; }
      loss += lk; dist += dk; total += ck;
      out[2 + k] = ck > 0 ? (float)(dk / (double)ck) : 0.f;
      count[1 + k] = (int32_t)ck;
    }
    out[0] = (float)(loss / (double)(total > 0 ? total : 1));
    out[1] = total > 0 ? (float)(dist / (double)total) : 0.f;
    count[0] = (int32_t)total;
  }
}

__global__ void __launch_bounds__(VH_THREADS) vote_loss_bwd_kernel(
    const float* __restrict__ dloss, const float* __restrict__ votes, const float* __restrict__ coord,
    const float* __restrict__ target, int target_per_point, const int64_t* __restrict__ offset, int nb,
    const int32_t* __restrict__ count, int64_t n, int K, float radius, float* __restrict__ dvotes) {
  const int32_t total = count[0];
  const float g = dloss[0] / (3.f * (float)(total > 0 ? total : 1));
  const int64_t pairs = n * K;
  for (int64_t p = (int64_t)blockIdx.x * VH_THREADS + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * VH_THREADS) {
    const int64_t r = p / K;
    const int kk = (int)(p - r * K);
    int lo = 0, hi = nb;   // scene = first b with offset[b] > r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (offset[mid] > r) hi = mid; else lo = mid + 1;
    }
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (lo < nb) {   // rows past offset[B-1] belong to no scene: zero gradient
      const float* tp = target + (target_per_point ? (r * K + kk) : ((int64_t)lo * K + kk)) * 3;
      const float tx = tp[0], ty = tp[1], tz = tp[2];
      const float cx = coord[r * 3], cy = coord[r * 3 + 1], cz = coord[r * 3 + 2];
      const float dx = cx - tx, dy = cy - ty, dz = cz - tz;
      if (sqrtf(dx * dx + dy * dy + dz * dz) < radius) {
        const float* vp = votes + p * 3;
        gx = g * fminf(fmaxf((cx + vp[0]) - tx, -1.f), 1.f);
        gy = g * fminf(fmaxf((cy + vp[1]) - ty, -1.f), 1.f);
        gz = g * fminf(fmaxf((cz + vp[2]) - tz, -1.f), 1.f);
      }
    }
    dvotes[p * 3] = gx; dvotes[p * 3 + 1] = gy; dvotes[p * 3 + 2] = gz;
  }
}

// ~512 chunks at any size (two workgroups per CU); at least 256 rows, so the per-chunk preamble (the scene lookup and
// the re-derivation of the prefixes) stays small against the chunk's own rows
static int64_t vote_rows_per_chunk(int64_t n) {
  int64_t r = cdiv(cdiv(n, 512), 16) * 16;
  return r < 256 ? 256 : r;
}
static int64_t vote_chunks(int64_t n, int b) { return cdiv(n, vote_rows_per_chunk(n)) + b; }
static size_t median_words(int c, int b) { return (size_t)b * c * (4 * VH_BINS + 1); }
static bool vh_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace ptv3

using namespace ptv3;

extern "C" size_t ptv3_scene_median_workspace_bytes(int c, int b) {
  return median_words(c < 0 ? 0 : c, b < 0 ? 0 : b) * sizeof(uint32_t);
}

extern "C" int ptv3_scene_median(const float* x, const float* coord, const int64_t* offset, int64_t n, int c, int b,
                                 float* out, void* workspace, size_t workspace_bytes, void* stream) {
  PTV3_REQUIRE(n >= 0 && n <= 0x7fffffff && b >= 0, "scene_median: bad shape n=%lld b=%d", (long long)n, b);
  PTV3_REQUIRE(c >= 1 && c <= VH_MAX_C, "scene_median: c=%d unsupported (1 to %d columns)", c, VH_MAX_C);
  PTV3_REQUIRE(!coord || c % 3 == 0, "scene_median: c=%d is not a multiple of 3 (coord is added per xyz triple)", c);
  PTV3_REQUIRE(b == 0 || (offset && out), "scene_median: offset / out is NULL");
  PTV3_REQUIRE(n == 0 || x, "scene_median: x is NULL");
  PTV3_REQUIRE(b == 0 || (workspace && vh_aligned16(workspace)), "scene_median: workspace must be 16-byte aligned");
  PTV3_REQUIRE(workspace_bytes >= ptv3_scene_median_workspace_bytes(c, b), "scene_median: workspace too small");
  if (b == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* hist = (uint32_t*)workspace;
  if (hipMemsetAsync(hist, 0, median_words(c, b) * sizeof(uint32_t), s) != hipSuccess) {
    ptv3::set_error("scene_median: clearing the histograms failed");
    return PTV3_ERR_LAUNCH;
  }
  const int64_t rb = vote_rows_per_chunk(n);
  const dim3 grid((unsigned)vote_chunks(n, b)), block(VH_THREADS);
  if (n > 0) {
    hipLaunchKernelGGL(median_pass_kernel<0>, grid, block, 0, s, x, coord, offset, b, n, c, rb, hist);
    hipLaunchKernelGGL(median_pass_kernel<1>, grid, block, 0, s, x, coord, offset, b, n, c, rb, hist);
    hipLaunchKernelGGL(median_pass_kernel<2>, grid, block, 0, s, x, coord, offset, b, n, c, rb, hist);
    hipLaunchKernelGGL(median_pass_kernel<3>, grid, block, 0, s, x, coord, offset, b, n, c, rb, hist);
  }
  hipLaunchKernelGGL(median_finish_kernel, dim3((unsigned)b), block, 0, s, hist, offset, b, n, c, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" size_t ptv3_vote_loss_workspace_bytes(int64_t n, int k, int b) {
  return (size_t)vote_chunks(n < 0 ? 0 : n, b < 0 ? 0 : b) * 3 * (k < 0 ? 0 : k) * sizeof(float);
}

static int vote_loss_check(const char* who, const float* votes, const float* coord, const float* target,
                           const int64_t* offset, int64_t n, int k, int b, float radius) {
  PTV3_REQUIRE(n >= 0 && n <= 0x7fffffff && b >= 0, "%s: bad shape n=%lld b=%d", who, (long long)n, b);
  PTV3_REQUIRE(k >= 1 && k <= VH_MAX_K, "%s: k=%d unsupported (1 to %d keypoints)", who, k, VH_MAX_K);
  PTV3_REQUIRE(radius == radius, "%s: vote_radius is NaN", who);
  PTV3_REQUIRE(n == 0 || b == 0 || (votes && coord && target && offset), "%s: votes / coord / target / offset is NULL",
               who);
  return PTV3_OK;
}

extern "C" int ptv3_vote_loss(const float* votes, const float* coord, const float* target, int target_per_point,
                              const int64_t* offset, const float* scale, int scale_per_point, int64_t n, int k, int b,
                              float radius, float* out, int32_t* count, void* workspace, size_t workspace_bytes,
                              void* stream) {
  const int rc = vote_loss_check("vote_loss", votes, coord, target, offset, n, k, b, radius);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(out && count, "vote_loss: out / count is NULL");
  PTV3_REQUIRE(workspace && vh_aligned16(workspace), "vote_loss: workspace must be 16-byte aligned");
  PTV3_REQUIRE(workspace_bytes >= ptv3_vote_loss_workspace_bytes(n, k, b), "vote_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = (n > 0 && b > 0) ? vote_chunks(n, b) : 0;
  if (chunks)
    hipLaunchKernelGGL(vote_loss_partial_kernel, dim3((unsigned)chunks), dim3(VH_THREADS), 0, s, votes, coord, target,
                       target_per_point, offset, b, scale, scale && scale_per_point, n, k, vote_rows_per_chunk(n),
                       radius, (float*)workspace);
  hipLaunchKernelGGL(vote_loss_finish_kernel, dim3(1), dim3(VH_THREADS), 0, s, (const float*)workspace, chunks, k, out,
                     count);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_vote_loss_bwd(const float* dloss, const float* votes, const float* coord, const float* target,
                                  int target_per_point, const int64_t* offset, const int32_t* count, int64_t n, int k,
                                  int b, float radius, float* dvotes, void* stream) {
  const int rc = vote_loss_check("vote_loss_bwd", votes, coord, target, offset, n, k, b, radius);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(n == 0 || (dloss && count && dvotes), "vote_loss_bwd: dloss / count / dvotes is NULL");
  if (n == 0) return PTV3_OK;
  int64_t blocks = cdiv(n * k, VH_THREADS);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(vote_loss_bwd_kernel, dim3((unsigned)blocks), dim3(VH_THREADS), 0, (hipStream_t)stream, dloss, votes,
                     coord, target, target_per_point, offset, b, count, n, k, radius, dvotes);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
