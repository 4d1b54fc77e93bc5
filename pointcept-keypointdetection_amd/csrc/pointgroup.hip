// PointGroup's evaluation tail (pointcept/models/point_group/point_group_v1m1_base.py:101-178 and
// libs/pointgroup_ops/src/bfs_cluster_kernel.cu) on the device: the ball query over a cell grid, connected components by
// a lock-free union over the same walk, and the proposal filter with its scores and dense masks.  DESIGN.md section 22.
//
// Geometry shared by the ball query and the clustering.  A point's cell is floor(x * (1 / edge)) per axis with
// edge = 1.01 * radius: the 1 % guard covers the fp32 rounding of the cell position (at most 2^-24 * 2^15 * 2 cells
// inside the key's range), so two rows whose fp32 d2 is below fl(radius^2) never lie two cells apart.  Cells are clamped
// to 16 bits per axis; clamping is monotone and never widens a gap, so far-out points cost time, not correctness.
// key = scene << 48 | cx << 32 | cy << 16 | cz.  ptv3_argsort_i64 is stable: inside a cell rows stay in ascending index.
// With z in the lowest bits the three cells (cx + dx, cy + dy, cz - 1 .. cz + 1) are one contiguous run of the sorted
// keys, so a point visits 9 runs, each found by one binary search.
#include <limits.h>
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace {

constexpr int PG_CAP = 1000;          // int idx_temp[1000] of bfs_cluster_kernel.cu:21
constexpr int PG_T = 256;
constexpr int SCAN_T = 256, SCAN_E = 4, SCAN_CHUNK = SCAN_T * SCAN_E;
constexpr int CELL_MAX = 65535;

struct S3 { unsigned a, b, c; };
__host__ __device__ __forceinline__ S3 add3(S3 x, S3 y) { return S3{x.a + y.a, x.b + y.b, x.c + y.c}; }

// d2 as bfs_cluster_kernel.cu:37 writes it, one rounding per operation (no contraction into fma)
__device__ __forceinline__ float pg_d2(float ox, float oy, float oz, float x, float y, float z) {
#pragma clang fp contract(off)
  const float dx = ox - x, dy = oy - y, dz = oz - z;
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ int pg_cell(float v, float inv_edge) {
  const float c = fminf(fmaxf(floorf(v * inv_edge), -32768.f), 32767.f);  // NaN ends in cell 0
  return (int)c + 32768;
}

__device__ __forceinline__ int64_t pg_key(int scene, int cx, int cy, int cz) {
  return ((int64_t)scene << 48) | ((int64_t)cx << 32) | ((int64_t)cy << 16) | (int64_t)cz;
}

__device__ __forceinline__ int64_t lower_bound64(const int64_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int scene_of(const int32_t* __restrict__ offsets, int num_scenes, int64_t i) {
  int lo = 0, hi = num_scenes - 1;  // largest s with offsets[s] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void pg_keys_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ batch_idxs,
                               const int32_t* __restrict__ offsets, int num_scenes, int64_t n, float inv_edge,
                               int64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (i >= n) return;
  int s = batch_idxs ? batch_idxs[i] : scene_of(offsets, num_scenes, i);
  s = min(max(s, 0), num_scenes - 1);
  key[i] = pg_key(s, pg_cell(xyz[3 * i], inv_edge), pg_cell(xyz[3 * i + 1], inv_edge), pg_cell(xyz[3 * i + 2], inv_edge));
}

// rows in key order: position, index (bits in .w), key and label side by side, so the walk reads runs, not gathers
__global__ void pg_gather_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ key,
                                 const int32_t* __restrict__ label, const int64_t* __restrict__ order, int64_t n,
                                 float4* __restrict__ sp, int64_t* __restrict__ skey, int32_t* __restrict__ slabel) {
  const int64_t t = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (t >= n) return;
  const int64_t i = order[t];
  sp[t] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
  skey[t] = key[i];
  if (label) slabel[t] = label[i];
}

// the 9 runs around a key: calls f(first, last_key) for each run that can exist
template <typename F>
__device__ __forceinline__ void pg_runs(int64_t k, const int64_t* __restrict__ skey, int64_t n, F f) {
  const int s = (int)(k >> 48), cx = (int)(k >> 32) & 0xffff, cy = (int)(k >> 16) & 0xffff, cz = (int)k & 0xffff;
  const int zlo = max(cz - 1, 0), zhi = min(cz + 1, CELL_MAX);
  for (int dx = -1; dx <= 1; ++dx) {
    const int x2 = cx + dx;
    if (x2 < 0 || x2 > CELL_MAX) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int y2 = cy + dy;
      if (y2 < 0 || y2 > CELL_MAX) continue;
      f(lower_bound64(skey, n, pg_key(s, x2, y2, zlo)), pg_key(s, x2, y2, zhi));
    }
  }
}

// ---- union: the larger root goes under the smaller, so a component's final root is its smallest member ------------
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
  while (p != x) {
    const int g = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (g != p) __atomic_store_n(&parent[x], g, __ATOMIC_RELAXED);  // halving: an ancestor, always a valid parent
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(&parent[a], a, b);  // a is still a root -> hook it under the smaller root
    if (old == a) return;
    a = old;
  }
}

__global__ void pg_iota_kernel(int* __restrict__ parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (i < n) parent[i] = (int)i;
}

// one thread per row in key order.  UNION = false: the ball query's count pass.  UNION = true: the count of all
// neighbours (any label) for the cap flag plus a union with every same-label neighbour of smaller index.
template <bool UNION>
__global__ void pg_walk_kernel(const float4* __restrict__ sp, const int64_t* __restrict__ skey,
                               const int32_t* __restrict__ slabel, int64_t n, float radius2, int32_t* __restrict__ cnt,
                               int* parent, int32_t* __restrict__ record) {
  const int64_t t = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (t >= n) return;
  const float4 o = sp[t];
  const int i = __float_as_int(o.w);
  const int li = UNION ? slabel[t] : 0;
  int c = 0;
  pg_runs(skey[t], skey, n, [&](int64_t p, int64_t last) {
    for (; p < n && skey[p] <= last; ++p) {
      const float4 q = sp[p];
      if (pg_d2(o.x, o.y, o.z, q.x, q.y, q.z) < radius2) {
        ++c;
        if (UNION) {
          const int j = __float_as_int(q.w);
          if (j < i && slabel[p] == li) uf_union(parent, i, j);
        }
      }
    }
  });
  if (UNION) {
    if (c > PG_CAP) record[2] = 1;  // same value from every writer
  } else {
    cnt[i] = c;
  }
}

// ---- exclusive scan of S3 triples: chunk totals, one workgroup over the totals, chunks again ---------------------
__device__ __forceinline__ S3 chunk_scan(const S3* in, S3* out, int64_t base, int64_t n, S3 carry, S3* sh) {
  const int t = threadIdx.x;
  S3 v[SCAN_E], s = S3{0, 0, 0};
#pragma unroll
  for (int e = 0; e < SCAN_E; ++e) {
    const int64_t k = base + (int64_t)t * SCAN_E + e;
    v[e] = k < n ? in[k] : S3{0, 0, 0};
    s = add3(s, v[e]);
  }
  sh[t] = s;
  __syncthreads();
  for (int o = 1; o < SCAN_T; o <<= 1) {
    const S3 x = t >= o ? sh[t - o] : S3{0, 0, 0};
    __syncthreads();
    sh[t] = add3(sh[t], x);
    __syncthreads();
  }
  const S3 incl = sh[t], total = sh[SCAN_T - 1];
  __syncthreads();
  if (out) {
    S3 run = add3(carry, S3{incl.a - s.a, incl.b - s.b, incl.c - s.c});
#pragma unroll
    for (int e = 0; e < SCAN_E; ++e) {
      const int64_t k = base + (int64_t)t * SCAN_E + e;
      if (k < n) out[k] = run;
      run = add3(run, v[e]);
    }
  }
  return total;
}

__global__ void __launch_bounds__(SCAN_T) scan_totals_kernel(const S3* __restrict__ in, int64_t n, S3* __restrict__ bs) {
  __shared__ S3 sh[SCAN_T];
  const S3 total = chunk_scan(in, nullptr, (int64_t)blockIdx.x * SCAN_CHUNK, n, S3{0, 0, 0}, sh);
  if (threadIdx.x == 0) bs[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_T) scan_carries_kernel(S3* bs, int64_t nb) {  // bs[nb] <- grand total
  __shared__ S3 sh[SCAN_T];
  S3 carry = S3{0, 0, 0};
  for (int64_t base = 0; base < nb; base += SCAN_CHUNK) carry = add3(carry, chunk_scan(bs, bs, base, nb, carry, sh));
  if (threadIdx.x == 0) bs[nb] = carry;
}

__global__ void __launch_bounds__(SCAN_T) scan_apply_kernel(const S3* __restrict__ in, int64_t n, const S3* __restrict__ bs,
                                                            S3* __restrict__ out) {
  __shared__ S3 sh[SCAN_T];
  chunk_scan(in, out, (int64_t)blockIdx.x * SCAN_CHUNK, n, bs[blockIdx.x], sh);
}

int scan3(const S3* in, S3* out, S3* bs, int64_t n, hipStream_t st) {
  const int64_t nb = ptv3::cdiv(n, SCAN_CHUNK);
  scan_totals_kernel<<<dim3((unsigned)nb), SCAN_T, 0, st>>>(in, n, bs);
  scan_carries_kernel<<<1, SCAN_T, 0, st>>>(bs, nb);
  scan_apply_kernel<<<dim3((unsigned)nb), SCAN_T, 0, st>>>(in, n, bs, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

// ---- ball query ------------------------------------------------------------------------------------------------------
__global__ void pg_bq_vals_kernel(const int32_t* __restrict__ cnt, int64_t n, S3* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (i < n) vals[i] = S3{(unsigned)min(cnt[i], PG_CAP), 0u, 0u};
}

__global__ void pg_bq_start_len_kernel(const int32_t* __restrict__ cnt, const S3* __restrict__ excl, int64_t n,
                                       int32_t* __restrict__ start_len) {
  const int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (i >= n) return;
  start_len[2 * i] = (int)excl[i].a;
  start_len[2 * i + 1] = min(cnt[i], PG_CAP);
}

// one wave per point.  Up to the cap: the hits of the 9 runs go to LDS and a bitonic network puts them in ascending
// index.  Above it: the reference's own scan of the scene in index order, 64 rows a step, until 1000 are written - the
// 1000 lowest indices without looking at the rest.
__global__ void __launch_bounds__(64) pg_bq_fill_kernel(const float* __restrict__ xyz, const float4* __restrict__ sp,
                                                        const int64_t* __restrict__ skey,
                                                        const int64_t* __restrict__ inverse,
                                                        const int32_t* __restrict__ offsets, int num_scenes, int64_t n,
                                                        float radius2, const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ start_len, int64_t n_active,
                                                        int32_t* __restrict__ idx) {
  __shared__ int hits[1024];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t start = start_len[2 * i];
  const int total = cnt[i];
  const int64_t t = inverse[i];
  const float4 o = sp[t];
  const unsigned long long below = (1ull << lane) - 1ull;
  if (total > PG_CAP) {
    const int s = (int)(skey[t] >> 48);
    const int64_t k0 = max((int64_t)offsets[s], (int64_t)0), k1 = min((int64_t)offsets[s + 1], n);
    int written = 0;
    for (int64_t base = k0; base < k1 && written < PG_CAP; base += 64) {
      const int64_t k = base + lane;
      bool hit = false;
      if (k < k1) hit = pg_d2(o.x, o.y, o.z, xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]) < radius2;
      const unsigned long long m = __ballot(hit);
      const int at = written + __popcll(m & below);
      if (hit && at < PG_CAP && start + at < n_active) idx[start + at] = (int)k;
      written += __popcll(m);
    }
    return;
  }
  int m = 0;
  pg_runs(skey[t], skey, n, [&](int64_t p0, int64_t last) {
    for (int64_t base = p0;; base += 64) {
      const int64_t p = base + lane;
      const bool in = p < n && skey[p] <= last;
      bool hit = false;
      float4 q = o;
      if (in) {
        q = sp[p];
        hit = pg_d2(o.x, o.y, o.z, q.x, q.y, q.z) < radius2;
      }
      const unsigned long long hm = __ballot(hit);
      const int at = m + __popcll(hm & below);
      if (hit && at < 1024) hits[at] = __float_as_int(q.w);
      m += __popcll(hm);
      if (__ballot(in) != ~0ull) break;
    }
  });
  m = min(m, min(total, 1024));
  int p2 = 1;
  while (p2 < m) p2 <<= 1;
  __syncthreads();
  for (int e = m + lane; e < p2; e += 64) hits[e] = INT_MAX;
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = lane; e < p2; e += 64) {
        const int partner = e ^ j;
        if (partner > e) {
          const int a = hits[e], b = hits[partner];
          const bool up = (e & k) == 0;
          if ((a > b) == up) { hits[e] = b; hits[partner] = a; }
        }
      }
      __syncthreads();
    }
  for (int e = lane; e < m; e += 64)
    if (start + e < n_active) idx[start + e] = hits[e];
}

// ---- clustering: components -> lists --------------------------------------------------------------------------------
__global__ void pg_roots_kernel(int* parent, int64_t n, int64_t* __restrict__ root_key) {
  const int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (i >= n) return;
  int x = (int)i, p = parent[x];   // the unions are done: a read-only walk to the root
  while (p != x) { x = p; p = parent[x]; }
  root_key[i] = x;
}

__global__ void pg_sorted_roots_kernel(const int64_t* __restrict__ root_key, const int64_t* __restrict__ order, int64_t n,
                                       int64_t* __restrict__ sroot) {
  const int64_t p = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (p < n) sroot[p] = root_key[order[p]];
}

// rows sorted by root (stable: members ascending).  A row finds its component's run by two binary searches, so sizes
// need no counters: vals = (kept row, kept head, head of a component above propose_points)
__global__ void pg_comp_vals_kernel(const int64_t* __restrict__ sroot, int64_t n, int min_points, int propose_points,
                                    S3* __restrict__ vals) {
  const int64_t p = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (p >= n) return;
  const int64_t r = sroot[p];
  const int64_t b = lower_bound64(sroot, n, r), e = lower_bound64(sroot, n, r + 1);
  const int64_t size = e - b;
  const bool kept = size >= (int64_t)min_points, head = p == b;
  vals[p] = S3{kept ? 1u : 0u, kept && head ? 1u : 0u, kept && head && size > (int64_t)propose_points ? 1u : 0u};
}

__global__ void pg_emit_kernel(const int64_t* __restrict__ order, const S3* __restrict__ vals, const S3* __restrict__ excl,
                               int64_t n, int32_t* __restrict__ cluster_idxs, int32_t* __restrict__ cluster_offsets,
                               int32_t* __restrict__ record) {
  const int64_t p = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (p >= n) return;
  const S3 v = vals[p], x = excl[p];
  if (v.a) {
    const int cid = (int)(v.b ? x.b : x.b - 1);
    cluster_idxs[2 * (int64_t)x.a] = cid;
    cluster_idxs[2 * (int64_t)x.a + 1] = (int)order[p];
    if (v.b) cluster_offsets[cid] = (int)x.a;
  }
  if (p == n - 1) {
    const S3 tot = add3(x, v);
    cluster_offsets[tot.b] = (int)tot.a;
    record[0] = (int)tot.b;
    record[1] = (int)tot.a;
    record[3] = (int)tot.c;
  }
}

// ---- proposals ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PG_T) pg_prop_slots_kernel(const int32_t* __restrict__ cluster_idxs,
                                                             const int32_t* __restrict__ cluster_offsets, int nc,
                                                             int64_t sum, const int64_t* __restrict__ segment_pred,
                                                             const int64_t* __restrict__ row_map, int64_t n_rows,
                                                             int64_t n_map, int propose_points, int P,
                                                             int32_t* __restrict__ slot,
                                                             int64_t* __restrict__ pred_classes) {
  __shared__ int sh[PG_T];
  const int t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < nc; base += PG_T) {
    const int c = base + t;
    int keep = 0;
    if (c < nc) keep = cluster_offsets[c + 1] - cluster_offsets[c] > propose_points ? 1 : 0;
    sh[t] = keep;
    __syncthreads();
    for (int o = 1; o < PG_T; o <<= 1) {
      const int x = t >= o ? sh[t - o] : 0;
      __syncthreads();
      sh[t] += x;
      __syncthreads();
    }
    const int at = carry + sh[t] - keep;
    carry += sh[PG_T - 1];
    __syncthreads();
    if (c < nc) {
      const bool ok = keep && at < P;
      slot[c] = ok ? at : -1;
      if (ok) {
        const int64_t first = cluster_offsets[c];
        int64_t row = first >= 0 && first < sum ? cluster_idxs[2 * first + 1] : -1;
        if (row_map) row = row >= 0 && row < n_map ? row_map[row] : -1;
        pred_classes[at] = row >= 0 && row < n_rows ? segment_pred[row] : -1;
      }
    }
  }
}

__global__ void pg_prop_masks_kernel(const int32_t* __restrict__ cluster_idxs, int64_t sum, int nc,
                                     const int32_t* __restrict__ slot, const int64_t* __restrict__ row_map, int64_t n_rows,
                                     int64_t n_map, int32_t* __restrict__ pred_masks) {
  const int64_t e = (int64_t)blockIdx.x * PG_T + threadIdx.x;
  if (e >= sum) return;
  const int c = cluster_idxs[2 * e];
  if (c < 0 || c >= nc) return;
  const int s = slot[c];
  if (s < 0) return;
  int64_t row = cluster_idxs[2 * e + 1];
  if (row_map) row = row >= 0 && row < n_map ? row_map[row] : -1;
  if (row >= 0 && row < n_rows) pred_masks[(int64_t)s * n_rows + row] = 1;
}

// one workgroup per cluster: thread t adds members t, t + 256, ... in that order, then a fixed tree over the 256 sums
__global__ void __launch_bounds__(PG_T) pg_prop_scores_kernel(const int32_t* __restrict__ cluster_idxs,
                                                              const int32_t* __restrict__ cluster_offsets, int64_t sum,
                                                              const int32_t* __restrict__ slot,
                                                              const float* __restrict__ prob, int C,
                                                              const int64_t* __restrict__ pred_classes,
                                                              const int64_t* __restrict__ row_map, int64_t n_rows,
                                                              int64_t n_map, float* __restrict__ pred_scores) {
  __shared__ float sh[PG_T];
  const int c = blockIdx.x, t = threadIdx.x;
  const int s = slot[c];
  if (s < 0) return;
  const int64_t cls = pred_classes[s];
  const int64_t b = max((int64_t)cluster_offsets[c], (int64_t)0), e = min((int64_t)cluster_offsets[c + 1], sum);
  float acc = 0.f;
  if (cls >= 0 && cls < C)
    for (int64_t m = b + t; m < e; m += PG_T) {
      int64_t row = cluster_idxs[2 * m + 1];
      if (row_map) row = row >= 0 && row < n_map ? row_map[row] : -1;
      if (row >= 0 && row < n_rows) acc += prob[row * C + cls];
    }
  sh[t] = acc;
  __syncthreads();
  for (int o = PG_T / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) pred_scores[s] = sh[0] / (float)(e - b);
}

// ---- workspace layout ------------------------------------------------------------------------------------------------
struct Ws {
  int64_t *key, *order, *inverse, *skey;
  float4* sp;
  int32_t *slabel, *cnt, *parent, *record;
  S3 *vals, *excl, *bs;
  void* sort;
  size_t sort_bytes, total;
};

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

Ws carve(void* base, int64_t n) {
  Ws w;
  char* p = (char*)base;
  const size_t m = (size_t)(n > 0 ? n : 1);
  auto take = [&](size_t bytes) { char* r = p; p += up16(bytes); return r; };
  w.sp = (float4*)take(m * sizeof(float4));
  w.key = (int64_t*)take(m * 8);
  w.order = (int64_t*)take(m * 8);
  w.inverse = (int64_t*)take(m * 8);
  w.skey = (int64_t*)take(m * 8);
  w.slabel = (int32_t*)take(m * 4);
  w.cnt = (int32_t*)take(m * 4);
  w.parent = (int32_t*)take(m * 4);
  w.record = (int32_t*)take(16);
  w.vals = (S3*)take(m * sizeof(S3));
  w.excl = (S3*)take(m * sizeof(S3));
  w.bs = (S3*)take((size_t)(ptv3::cdiv((int64_t)m, SCAN_CHUNK) + 1) * sizeof(S3));
  w.sort_bytes = ptv3_argsort_workspace_bytes(1, (int64_t)m);
  w.sort = take(w.sort_bytes);
  w.total = (size_t)(p - (char*)base);
  return w;
}

unsigned blocks(int64_t n) { return (unsigned)ptv3::cdiv(n, PG_T); }

// keys -> stable sort -> rows in key order
int build_grid(const float* xyz, const int32_t* batch_idxs, const int32_t* offsets, int num_scenes, const int32_t* label,
               int64_t n, float radius, const Ws& w, hipStream_t st) {
  const float inv_edge = 1.0f / (radius * 1.01f);
  pg_keys_kernel<<<blocks(n), PG_T, 0, st>>>(xyz, batch_idxs, offsets, num_scenes, n, inv_edge, w.key);
  PTV3_LAUNCH_CHECK();
  const int rc = ptv3_argsort_i64(w.key, 1, n, 63, w.order, w.inverse, w.sort, w.sort_bytes, st);
  if (rc != PTV3_OK) return rc;
  pg_gather_kernel<<<blocks(n), PG_T, 0, st>>>(xyz, w.key, label, w.order, n, w.sp, w.skey, w.slabel);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

int check_common(const char* who, const void* xyz, const int32_t* offsets, int num_scenes, int64_t n, float radius,
                 void* workspace, size_t workspace_bytes) {
  PTV3_REQUIRE(n >= 0 && n <= (int64_t)2000000, "%s: n = %lld outside [0, 2000000]", who, (long long)n);
  PTV3_REQUIRE(num_scenes >= 1 && num_scenes < 32768, "%s: %d scenes outside [1, 32767]", who, num_scenes);
  PTV3_REQUIRE(radius > 0.f && radius < 1e30f, "%s: radius must be positive and finite", who);
  PTV3_REQUIRE(offsets && (n == 0 || xyz), "%s: null pointer", who);
  PTV3_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= ptv3_pg_workspace_bytes(n),
               "%s: workspace of %zu bytes, 16-byte aligned, needed", who, ptv3_pg_workspace_bytes(n));
  return PTV3_OK;
}

}  // namespace

extern "C" size_t ptv3_pg_workspace_bytes(int64_t n) { return carve(nullptr, n).total; }

extern "C" int ptv3_pg_ballquery_batch_p(const float* xyz, const int32_t* batch_idxs, const int32_t* batch_offsets,
                                         int num_scenes, int64_t n, float radius, int32_t* start_len, int32_t* idx,
                                         int64_t* n_active, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int rc0 = check_common("ptv3_pg_ballquery_batch_p", xyz, batch_offsets, num_scenes, n, radius, workspace,
                               workspace_bytes);
  if (rc0 != PTV3_OK) return rc0;
  PTV3_REQUIRE(n_active && (n == 0 || start_len), "ptv3_pg_ballquery_batch_p: null pointer");
  if (n == 0) { *n_active = 0; return PTV3_OK; }
  const Ws w = carve(workspace, n);
  const float radius2 = radius * radius;
  if (!idx) {  // phase 1: count, scan, start_len; the total goes to the host, which sizes idx with it
    const int rc = build_grid(xyz, batch_idxs, batch_offsets, num_scenes, nullptr, n, radius, w, st);
    if (rc != PTV3_OK) return rc;
    pg_walk_kernel<false><<<blocks(n), PG_T, 0, st>>>(w.sp, w.skey, nullptr, n, radius2, w.cnt, nullptr, nullptr);
    pg_bq_vals_kernel<<<blocks(n), PG_T, 0, st>>>(w.cnt, n, w.vals);
    PTV3_LAUNCH_CHECK();
    const int rs = scan3(w.vals, w.excl, w.bs, n, st);
    if (rs != PTV3_OK) return rs;
    pg_bq_start_len_kernel<<<blocks(n), PG_T, 0, st>>>(w.cnt, w.excl, n, start_len);
    PTV3_LAUNCH_CHECK();
    S3 total;
    if (hipMemcpyAsync(&total, w.bs + ptv3::cdiv(n, SCAN_CHUNK), sizeof(S3), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      ptv3::set_error("ptv3_pg_ballquery_batch_p: reading the total failed: %s", hipGetErrorString(hipGetLastError()));
      return PTV3_ERR_LAUNCH;
    }
    *n_active = (int64_t)total.a;
    return PTV3_OK;
  }
  // phase 2: the workspace still holds phase 1's grid, counts and start_len's source
  PTV3_REQUIRE(*n_active >= 0 && *n_active <= n * PG_CAP, "ptv3_pg_ballquery_batch_p: n_active out of range");
  pg_bq_fill_kernel<<<dim3((unsigned)n), 64, 0, st>>>(xyz, w.sp, w.skey, w.inverse, batch_offsets, num_scenes, n, radius2,
                                                      w.cnt, start_len, *n_active, idx);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_pg_cluster(const float* xyz, const int32_t* label, const int32_t* offsets, int num_scenes, int64_t n,
                               float radius, int min_points, int propose_points, int32_t* cluster_idxs,
                               int32_t* cluster_offsets, int32_t* record_host, void* workspace, size_t workspace_bytes,
                               void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int rc0 = check_common("ptv3_pg_cluster", xyz, offsets, num_scenes, n, radius, workspace, workspace_bytes);
  if (rc0 != PTV3_OK) return rc0;
  PTV3_REQUIRE(record_host && cluster_offsets && (n == 0 || (label && cluster_idxs)), "ptv3_pg_cluster: null pointer");
  record_host[0] = record_host[1] = record_host[2] = record_host[3] = 0;
  if (n == 0) {
    if (hipMemsetAsync(cluster_offsets, 0, sizeof(int32_t), st) != hipSuccess) return PTV3_ERR_LAUNCH;
    return PTV3_OK;
  }
  const Ws w = carve(workspace, n);
  if (hipMemsetAsync(w.record, 0, 16, st) != hipSuccess) return PTV3_ERR_LAUNCH;
  const int rc = build_grid(xyz, nullptr, offsets, num_scenes, label, n, radius, w, st);
  if (rc != PTV3_OK) return rc;
  pg_iota_kernel<<<blocks(n), PG_T, 0, st>>>(w.parent, n);
  pg_walk_kernel<true><<<blocks(n), PG_T, 0, st>>>(w.sp, w.skey, w.slabel, n, radius * radius, nullptr, w.parent, w.record);
  pg_roots_kernel<<<blocks(n), PG_T, 0, st>>>(w.parent, n, w.key);
  PTV3_LAUNCH_CHECK();
  const int rs = ptv3_argsort_i64(w.key, 1, n, 32, w.order, w.inverse, w.sort, w.sort_bytes, st);
  if (rs != PTV3_OK) return rs;
  pg_sorted_roots_kernel<<<blocks(n), PG_T, 0, st>>>(w.key, w.order, n, w.skey);
  pg_comp_vals_kernel<<<blocks(n), PG_T, 0, st>>>(w.skey, n, min_points, propose_points, w.vals);
  PTV3_LAUNCH_CHECK();
  const int rq = scan3(w.vals, w.excl, w.bs, n, st);
  if (rq != PTV3_OK) return rq;
  pg_emit_kernel<<<blocks(n), PG_T, 0, st>>>(w.order, w.vals, w.excl, n, cluster_idxs, cluster_offsets, w.record);
  PTV3_LAUNCH_CHECK();
  if (hipMemcpyAsync(record_host, w.record, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    ptv3::set_error("ptv3_pg_cluster: reading the record failed: %s", hipGetErrorString(hipGetLastError()));
    return PTV3_ERR_LAUNCH;
  }
  if (record_host[2]) {
    ptv3::set_error("ptv3_pg_cluster: a point has more than %d neighbours; take the list path", PG_CAP);
    return PTV3_PG_TRUNCATED;
  }
  return PTV3_OK;
}

extern "C" int ptv3_pg_proposals(const int32_t* cluster_idxs, const int32_t* cluster_offsets, int num_clusters,
                                 int64_t sum, const float* prob, int num_classes, const int64_t* segment_pred,
                                 const int64_t* row_map, int64_t n_map, int64_t n_rows, int propose_points,
                                 int num_proposals, int64_t* pred_classes, float* pred_scores, int32_t* pred_masks,
                                 int32_t* slot, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  PTV3_REQUIRE(num_clusters >= 0 && sum >= 0 && n_rows >= 0 && num_proposals >= 0 && num_proposals <= num_clusters,
               "ptv3_pg_proposals: negative size or more proposals than clusters");
  PTV3_REQUIRE(num_classes >= 1 && propose_points >= 0, "ptv3_pg_proposals: num_classes >= 1 and propose_points >= 0");
  if (num_clusters == 0) return PTV3_OK;
  PTV3_REQUIRE(cluster_idxs && cluster_offsets && prob && segment_pred && slot, "ptv3_pg_proposals: null pointer");
  PTV3_REQUIRE(num_proposals == 0 || (pred_classes && pred_scores && pred_masks), "ptv3_pg_proposals: null output");
  if (num_proposals > 0 &&
      hipMemsetAsync(pred_masks, 0, (size_t)num_proposals * (size_t)n_rows * sizeof(int32_t), st) != hipSuccess)
    return PTV3_ERR_LAUNCH;
  pg_prop_slots_kernel<<<1, PG_T, 0, st>>>(cluster_idxs, cluster_offsets, num_clusters, sum, segment_pred, row_map,
                                           n_rows, n_map, propose_points, num_proposals, slot, pred_classes);
  PTV3_LAUNCH_CHECK();
  if (num_proposals == 0 || sum == 0) return PTV3_OK;
  pg_prop_masks_kernel<<<blocks(sum), PG_T, 0, st>>>(cluster_idxs, sum, num_clusters, slot, row_map, n_rows, n_map,
                                                    pred_masks);
  pg_prop_scores_kernel<<<dim3((unsigned)num_clusters), PG_T, 0, st>>>(cluster_idxs, cluster_offsets, sum, slot, prob,
                                                                     num_classes, pred_classes, row_map, n_rows, n_map,
                                                                     pred_scores);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
