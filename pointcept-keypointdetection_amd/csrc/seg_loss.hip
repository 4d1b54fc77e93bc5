// Segmentation losses of the pigseg / *-lovasz configs: multiclass Lovasz-Softmax and the multi-class sigmoid focal loss,
// forward and backward, with nothing read back by the host.
//   lovasz_prep_kernel<G>     a G-lane group per row: fp32 softmax, err = |fg - p_c|, one 64-bit sort key per (class, row)
//   (ptv3_argsort_i64)        the library's stable LSD radix sort, k = C rows of keys, end_bit 33
//   lovasz_tile_count_kernel  foreground count of every SL_TILE positions of a class's sorted order
//   lovasz_tile_scan_kernel   one workgroup per class: exclusive scan of the tile counts; the total is G_c = count[c]
//   lovasz_apply_kernel       in-tile scan + tile base -> F; closed-form weight in fp64 -> weight[point, c]; err * g per
//                             tile -> slab
//   lovasz_finish_kernel      one workgroup: per-class slab sums in a fixed order (float64), mean over present classes
//   lovasz_bwd_kernel<G>      softmax recomputed by the same G-lane code (bitwise the forward's p), softmax backward
//   focal_partial_kernel      fixed chunks of FL_CHUNK elements -> (sum, valid rows) slab
//   focal_finish_kernel       one workgroup: the slabs in a fixed order (float64, integer counts)
//   focal_bwd_kernel          elementwise
// Every hand-off between workgroups is a kernel boundary: no look-back, no flags, no atomics at all; two runs are bitwise
// equal.  A row is VALID when its label differs from ignore_index and lies in [0, C); any other row is treated as ignored
// (the reference faults on an out-of-range label), so no index leaves the buffers.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int SL_THREADS = 256;
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr int SL_ITEMS = 4;                       // consecutive sorted positions per thread
constexpr int SL_TILE = SL_THREADS * SL_ITEMS;    // scan tile (ptv3_lovasz_scan_tile)
constexpr int SL_MAX_C = 1024;
constexpr int FL_ITEMS = 16;
constexpr int FL_CHUNK = SL_THREADS * FL_ITEMS;   // elements of (n, C) per focal slab entry

__device__ __forceinline__ bool sl_valid(int64_t label, int64_t ignore_index, int C) {
  return label != ignore_index && label >= 0 && label < (int64_t)C;
}

// all-lanes reductions inside an aligned group of G lanes (xor butterfly: every lane ends with the same bits)
template <int G> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int m = G >> 1; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = G >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Softmax statistics of one row held by a G-lane group (lane l takes classes l, l + G, ...): p_c = expf(x_c - mx) * inv.
// Shared by the forward and the backward, so both see the same p bit for bit.
template <int G>
__device__ __forceinline__ void row_softmax_stats(const float* __restrict__ x, int C, int l, bool active, float* mx,
                                                  float* inv) {
  float m = -3.0e38f;
  if (active)
    for (int c = l; c < C; c += G) m = fmaxf(m, x[c]);
  m = group_max<G>(m);
  float s = 0.f;
  if (active)
    for (int c = l; c < C; c += G) s += expf(x[c] - m);
  s = group_sum<G>(s);
  *mx = m;
  *inv = 1.f / s;
}

// key: ascending unsigned order = descending err (err >= 0, so its inverted bits are monotonic); bit 32 set for a row
// that is not valid, which then sorts after every valid row.  The stable sort breaks ties by point index.
template <int G>
__global__ void __launch_bounds__(SL_THREADS) lovasz_prep_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ labels, int64_t n, int C,
                                                                  int64_t ignore_index, uint64_t* __restrict__ keys) {
  constexpr int RPB = SL_THREADS / G;
  const int l = threadIdx.x % G, rl = threadIdx.x / G;
  for (int64_t rb = (int64_t)blockIdx.x * RPB; rb < n; rb += (int64_t)gridDim.x * RPB) {
    const int64_t r = rb + rl;
    const bool active = r < n;
    const float* x = logits + (active ? r : 0) * C;
    float mx, inv;
    row_softmax_stats<G>(x, C, l, active, &mx, &inv);
    if (!active) continue;
    const int64_t lab = labels[r];
    const bool valid = sl_valid(lab, ignore_index, C);
    for (int c = l; c < C; c += G) {
      const float p = expf(x[c] - mx) * inv;
      const float err = fabsf(((valid && lab == c) ? 1.f : 0.f) - p);
      const uint64_t k = (uint64_t)(~__float_as_uint(err)) | (valid ? 0ull : (1ull << 32));
      keys[(int64_t)c * n + r] = k;
    }
  }
}

__device__ __forceinline__ float key_err(uint64_t k) { return __uint_as_float(~(uint32_t)k); }

// block-wide exclusive scan of one int per thread (fixed order); returns the exclusive prefix, *total = block sum
__device__ __forceinline__ int block_exclusive_scan(int v, int* total, int* wsum /* SL_WAVES */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(x, d, 64);
    if (lane >= d) x += t;
  }
  __syncthreads();   // wsum may still be read from a previous call
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SL_WAVES; ++w) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  *total = tot;
  return base + x - v;
}

// tile_count[c][tile] = number of foreground rows among the tile's sorted positions
__global__ void __launch_bounds__(SL_THREADS) lovasz_tile_count_kernel(const int64_t* __restrict__ order,
                                                                        const int64_t* __restrict__ labels, int64_t n,
                                                                        int C, int64_t ignore_index, int nt,
                                                                        int32_t* __restrict__ tile_count) {
  __shared__ int wsum[SL_WAVES];
  const int c = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * SL_TILE + (int64_t)threadIdx.x * SL_ITEMS;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < SL_ITEMS; ++j) {
    const int64_t pos = p0 + j;
    if (pos < n) {
      const int64_t lab = labels[order[(int64_t)c * n + pos]];
      cnt += (sl_valid(lab, ignore_index, C) && lab == c) ? 1 : 0;
    }
  }
  int total;
  block_exclusive_scan(cnt, &total, wsum);
  if (threadIdx.x == 0) tile_count[(int64_t)c * nt + blockIdx.x] = total;
}

// one workgroup per class: tile_count[c][.] becomes its exclusive prefix; count[c] = G_c.  SL_THREADS tiles per pass,
// the carry handed from pass to pass inside the workgroup.
__global__ void __launch_bounds__(SL_THREADS) lovasz_tile_scan_kernel(int32_t* __restrict__ tile_count, int nt,
                                                                       int32_t* __restrict__ count) {
  __shared__ int wsum[SL_WAVES];
  int32_t* row = tile_count + (int64_t)blockIdx.x * nt;
  int carry = 0;
  for (int t0 = 0; t0 < nt; t0 += SL_THREADS) {
    const int t = t0 + (int)threadIdx.x;
    const int v = t < nt ? row[t] : 0;
    int total;
    const int ex = block_exclusive_scan(v, &total, wsum);
    if (t < nt) row[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

// Lovasz weight of sorted position i (1-based) with F foreground rows among positions 1..i, in closed form:
//   I = G - F, U = G + i - F;  fg: 1/U;  bg: I / (U (U - 1)), and 1 - I/U at i = 1
// = jaccard_i - jaccard_{i-1} of lovasz.py:22-33 without the subtraction of near-equal numbers.
__device__ __forceinline__ double lovasz_weight(bool fg, int64_t i, int64_t F, int64_t G) {
  const int64_t I = G - F, U = G + i - F;
  if (fg) return 1.0 / (double)U;
  if (i == 1) return 1.0 - (double)I / (double)U;
  return (double)I / ((double)U * (double)(U - 1));
}

__global__ void __launch_bounds__(SL_THREADS) lovasz_apply_kernel(
    const int64_t* __restrict__ order, const int64_t* __restrict__ labels, const uint64_t* __restrict__ keys,
    const int32_t* __restrict__ tile_base, const int32_t* __restrict__ count, int64_t n, int C, int64_t ignore_index,
    int nt, float* __restrict__ weight, double* __restrict__ slab) {
  __shared__ int wsum[SL_WAVES];
  __shared__ double red[SL_THREADS];
  const int c = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * SL_TILE + (int64_t)threadIdx.x * SL_ITEMS;
  int64_t idx[SL_ITEMS];
  bool valid[SL_ITEMS], fg[SL_ITEMS];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < SL_ITEMS; ++j) {
    const int64_t pos = p0 + j;
    idx[j] = -1; valid[j] = false; fg[j] = false;
    if (pos < n) {
      idx[j] = order[(int64_t)c * n + pos];
      const int64_t lab = labels[idx[j]];
      valid[j] = sl_valid(lab, ignore_index, C);
      fg[j] = valid[j] && lab == c;
      cnt += fg[j] ? 1 : 0;
    }
  }
  int total;
  int64_t F = (int64_t)tile_base[(int64_t)c * nt + blockIdx.x] + block_exclusive_scan(cnt, &total, wsum);
  const int64_t G = count[c];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < SL_ITEMS; ++j) {
    if (idx[j] < 0) continue;
    F += fg[j] ? 1 : 0;
    float w = 0.f;
    if (valid[j]) {   // valid rows sort first, so position p0 + j + 1 counts valid rows only
      const double g = lovasz_weight(fg[j], p0 + j + 1, F, G);
      acc += (double)key_err(keys[(int64_t)c * n + idx[j]]) * g;
      w = (float)g;
    }
    weight[idx[j] * C + c] = w;
  }
  red[threadIdx.x] = acc;
  for (int d = SL_THREADS >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
  }
  if (threadIdx.x == 0) slab[(int64_t)c * nt + blockIdx.x] = red[0];
}

// out[0] = loss_weight * (sum over present classes of their slab sums) / n_present, 0 without a present class;
// count[C] = n_present
__global__ void __launch_bounds__(SL_THREADS) lovasz_finish_kernel(const double* __restrict__ slab, int nt, int C,
                                                                    float loss_weight, float* __restrict__ out,
                                                                    int32_t* __restrict__ count) {
  __shared__ double red[SL_THREADS];
  double loss = 0.0;
  int present = 0;
  for (int c = 0; c < C; ++c) {
    if (count[c] <= 0) continue;   // uniform across the workgroup
    ++present;
    double acc = 0.0;
    for (int t = threadIdx.x; t < nt; t += SL_THREADS) acc += slab[(int64_t)c * nt + t];
    __syncthreads();
    red[threadIdx.x] = acc;
    for (int d = SL_THREADS >> 1; d >= 1; d >>= 1) {
      __syncthreads();
      if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    }
    __syncthreads();
    loss += red[0];
  }
  if (threadIdx.x == 0) {
    out[0] = present ? (float)((double)loss_weight * loss / (double)present) : 0.f;
    count[C] = present;
  }
}

// dP_c = dloss * loss_weight / n_present * weight[i, c] * (fg ? -1 : +1) for a present class, else 0;
// dlogit_j = p_j (dP_j - sum_k p_k dP_k); zeros for a row that is not valid
template <int G>
__global__ void __launch_bounds__(SL_THREADS) lovasz_bwd_kernel(
    const float* __restrict__ dloss, const float* __restrict__ logits, const int64_t* __restrict__ labels,
    const float* __restrict__ weight, const int32_t* __restrict__ count, int64_t n, int C, int64_t ignore_index,
    float loss_weight, float* __restrict__ dlogits) {
  constexpr int RPB = SL_THREADS / G;
  const int l = threadIdx.x % G, rl = threadIdx.x / G;
  const int present = count[C];
  const float scale = present > 0 ? dloss[0] * loss_weight / (float)present : 0.f;
  for (int64_t rb = (int64_t)blockIdx.x * RPB; rb < n; rb += (int64_t)gridDim.x * RPB) {
    const int64_t r = rb + rl;
    const bool active = r < n;
    const float* x = logits + (active ? r : 0) * C;
    float mx, inv;
    row_softmax_stats<G>(x, C, l, active, &mx, &inv);
    const int64_t lab = active ? labels[r] : -1;
    const bool valid = active && sl_valid(lab, ignore_index, C);
    float dot = 0.f;
    if (valid)
      for (int c = l; c < C; c += G) {
        const float p = expf(x[c] - mx) * inv;
        const float dp = count[c] > 0 ? scale * weight[r * C + c] * (lab == c ? -1.f : 1.f) : 0.f;
        dot += p * dp;
      }
    dot = group_sum<G>(dot);
    if (!active) continue;
    for (int c = l; c < C; c += G) {
      float d = 0.f;
      if (valid) {
        const float p = expf(x[c] - mx) * inv;
        const float dp = count[c] > 0 ? scale * weight[r * C + c] * (lab == c ? -1.f : 1.f) : 0.f;
        d = p * (dp - dot);
      }
      dlogits[r * C + c] = d;
    }
  }
}

// ---- focal loss -------------------------------------------------------------------------------------------------
// One element of misc.py:157-167 in a form without cancellation: e = exp(-|x|), s = sigmoid(x) and 1 - s from e,
// q = t ? 1 - s : s, bce = max(x, 0) - x t + log1p(e).  *dq_factor = (1 - q)(1 - 2t) (dq/dx = q * that), *s_minus_t.
__device__ __forceinline__ float pow_gamma(float q, float gamma) {
  return gamma == 2.f ? q * q : (gamma == 0.f ? 1.f : powf(q, gamma));
}
__device__ __forceinline__ void focal_terms(float x, bool t, float* q, float* bce, float* s_minus_t) {
  const float e = expf(-fabsf(x));
  const float big = 1.f / (1.f + e), small = e * big;     // sigmoid(|x|), sigmoid(-|x|)
  const float s = x >= 0.f ? big : small, om = x >= 0.f ? small : big;
  *q = t ? om : s;
  *bce = fmaxf(x, 0.f) - (t ? x : 0.f) + log1pf(e);
  *s_minus_t = t ? -om : s;
}

__global__ void __launch_bounds__(SL_THREADS) focal_partial_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ labels,
                                                                    const float* __restrict__ alpha, int64_t total,
                                                                    int C, int64_t ignore_index, float gamma,
                                                                    double* __restrict__ slab_sum,
                                                                    int32_t* __restrict__ slab_rows) {
  __shared__ double red[SL_THREADS];
  __shared__ int redc[SL_THREADS];
  const int64_t base = (int64_t)blockIdx.x * FL_CHUNK;
  float acc = 0.f;
  int rows = 0;
#pragma unroll 4
  for (int j = 0; j < FL_ITEMS; ++j) {
    const int64_t e = base + (int64_t)j * SL_THREADS + threadIdx.x;
    if (e >= total) break;
    const int64_t r = (int64_t)((uint32_t)e / (uint32_t)C);   // total < 2^31
    const int c = (int)(e - r * C);
    const int64_t lab = labels[r];
    if (!sl_valid(lab, ignore_index, C)) continue;
    rows += c == 0 ? 1 : 0;
    const bool t = lab == c;
    float q, bce, smt;
    focal_terms(logits[e], t, &q, &bce, &smt);
    const float a = t ? alpha[c] : 1.f - alpha[c];
    acc += a * pow_gamma(q, gamma) * bce;
  }
  red[threadIdx.x] = (double)acc;
  redc[threadIdx.x] = rows;
  for (int d = SL_THREADS >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < d) {
      red[threadIdx.x] += red[threadIdx.x + d];
      redc[threadIdx.x] += redc[threadIdx.x + d];
    }
  }
  if (threadIdx.x == 0) {
    slab_sum[blockIdx.x] = red[0];
    slab_rows[blockIdx.x] = redc[0];
  }
}

// out[0] = loss_weight * sum (/ (n_valid * C) for "mean"), 0 without a valid row; nvalid[0] = n_valid
__global__ void __launch_bounds__(SL_THREADS) focal_finish_kernel(const double* __restrict__ slab_sum,
                                                                   const int32_t* __restrict__ slab_rows, int64_t chunks,
                                                                   int C, float loss_weight, int mean,
                                                                   float* __restrict__ out, int32_t* __restrict__ nvalid) {
  __shared__ double red[SL_THREADS];
  __shared__ long long redc[SL_THREADS];
  double acc = 0.0;
  long long rows = 0;
  for (int64_t k = threadIdx.x; k < chunks; k += SL_THREADS) {
    acc += slab_sum[k];
    rows += slab_rows[k];
  }
  red[threadIdx.x] = acc;
  redc[threadIdx.x] = rows;
  for (int d = SL_THREADS >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < d) {
      red[threadIdx.x] += red[threadIdx.x + d];
      redc[threadIdx.x] += redc[threadIdx.x + d];
    }
  }
  if (threadIdx.x == 0) {
    const long long nv = redc[0];
    double loss = 0.0;
    if (nv > 0) loss = (double)loss_weight * (mean ? red[0] / ((double)nv * (double)C) : red[0]);
    out[0] = (float)loss;
    nvalid[0] = (int32_t)nv;
  }
}

// dx = scale * a * q^gamma * (gamma (1 - q)(1 - 2t) bce + (s - t)): gamma q^(gamma-1) s(1-s) written as
// gamma q^gamma (1 - q), since s(1 - s) = q(1 - q) - no q^(gamma-1), which overflows at q = 0 for gamma < 1
__global__ void __launch_bounds__(SL_THREADS) focal_bwd_kernel(const float* __restrict__ dloss,
                                                                const float* __restrict__ logits,
                                                                const int64_t* __restrict__ labels,
                                                                const float* __restrict__ alpha,
                                                                const int32_t* __restrict__ nvalid, int64_t total, int C,
                                                                int64_t ignore_index, float gamma, float loss_weight,
                                                                int mean, float* __restrict__ dlogits) {
  const int nv = nvalid[0];
  float scale = dloss[0] * loss_weight;
  if (mean) scale = nv > 0 ? (float)((double)scale / ((double)nv * (double)C)) : 0.f;
  for (int64_t e = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * SL_THREADS) {
    const int64_t r = (int64_t)((uint32_t)e / (uint32_t)C);   // total < 2^31
    const int c = (int)(e - r * C);
    const int64_t lab = labels[r];
    float d = 0.f;
    if (sl_valid(lab, ignore_index, C)) {
      const bool t = lab == c;
      float q, bce, smt;
      focal_terms(logits[e], t, &q, &bce, &smt);
      const float a = t ? alpha[c] : 1.f - alpha[c];
      d = scale * a * pow_gamma(q, gamma) * (gamma * (1.f - q) * (t ? -1.f : 1.f) * bce + smt);
    }
    dlogits[e] = d;
  }
}

static inline size_t sl_align256(size_t x) { return (x + 255) / 256 * 256; }
static bool sl_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int sl_group(int C) {
  int g = 2;
  while (g < C && g < 64) g <<= 1;
  return g;
}
static unsigned sl_row_blocks(int64_t n, int g) {
  const int64_t b = cdiv(n, SL_THREADS / g);
  return (unsigned)(b > 8192 ? 8192 : b);
}

static int seg_loss_check(const char* who, const void* logits, const void* labels, int64_t n, int C) {
  PTV3_REQUIRE(C >= 2 && C <= SL_MAX_C, "%s: C=%d unsupported (2 to %d classes)", who, C, SL_MAX_C);
  PTV3_REQUIRE(n >= 0 && n * (int64_t)C < (1ll << 31), "%s: n=%lld, C=%d: n * C must stay below 2^31", who,
               (long long)n, C);
  PTV3_REQUIRE(n == 0 || (logits && labels), "%s: logits / labels is NULL", who);
  PTV3_REQUIRE(sl_aligned16(logits) && sl_aligned16(labels), "%s: logits / labels must be 16-byte aligned", who);
  return PTV3_OK;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_lovasz_scan_tile(void) { return SL_TILE; }

// keys (C, n) u64 | inverse (C, n) i64 | tile counts (C, nt) i32 | slab (C, nt) f64 | the sort's own workspace
extern "C" size_t ptv3_lovasz_workspace_bytes(int64_t n, int C) {
  if (n < 0) n = 0;
  if (C < 0) C = 0;
  const int64_t nt = cdiv(n, SL_TILE);
  return 2 * sl_align256((size_t)C * n * 8) + sl_align256((size_t)C * nt * 4) + sl_align256((size_t)C * nt * 8) +
         ptv3_argsort_workspace_bytes(C, n);
}

extern "C" int ptv3_lovasz_fwd(const float* logits, const int64_t* labels, int64_t n, int C, int64_t ignore_index,
                               float loss_weight, float* out, float* weight, int64_t* order, int32_t* count,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = seg_loss_check("lovasz_fwd", logits, labels, n, C);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(out && count && (n == 0 || (weight && order)), "lovasz_fwd: out / count / weight / order is NULL");
  PTV3_REQUIRE(sl_aligned16(weight) && sl_aligned16(order), "lovasz_fwd: weight / order must be 16-byte aligned");
  PTV3_REQUIRE(workspace && sl_aligned16(workspace), "lovasz_fwd: workspace must be 16-byte aligned");
  PTV3_REQUIRE(workspace_bytes >= ptv3_lovasz_workspace_bytes(n, C), "lovasz_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nt = (int)cdiv(n, SL_TILE);
  char* ws = (char*)workspace;
  const size_t kb = sl_align256((size_t)C * n * 8);
  uint64_t* keys = (uint64_t*)ws;
  int64_t* inverse = (int64_t*)(ws + kb);
  int32_t* tiles = (int32_t*)(ws + 2 * kb);
  double* slab = (double*)(ws + 2 * kb + sl_align256((size_t)C * nt * 4));
  char* sort_ws = ws + 2 * kb + sl_align256((size_t)C * nt * 4) + sl_align256((size_t)C * nt * 8);
  if (n > 0) {
    const int g = sl_group(C);
    by_value<2, 4, 8, 16, 32, 64>(g, [&](auto G) {
      hipLaunchKernelGGL(lovasz_prep_kernel<G()>, dim3(sl_row_blocks(n, G())), dim3(SL_THREADS), 0, s, logits, labels, n,
                         C, ignore_index, keys);
    });
    const int src = ptv3_argsort_i64((const int64_t*)keys, C, n, 33, order, inverse, sort_ws,
                                     ptv3_argsort_workspace_bytes(C, n), stream);
    if (src != PTV3_OK) return src;
    const dim3 grid((unsigned)nt, (unsigned)C), block(SL_THREADS);
    hipLaunchKernelGGL(lovasz_tile_count_kernel, grid, block, 0, s, order, labels, n, C, ignore_index, nt, tiles);
  }
  // with n = 0 there is no tile: the scan writes count[c] = 0 and the finish a zero loss
  hipLaunchKernelGGL(lovasz_tile_scan_kernel, dim3((unsigned)C), dim3(SL_THREADS), 0, s, tiles, nt, count);
  if (n > 0)
    hipLaunchKernelGGL(lovasz_apply_kernel, dim3((unsigned)nt, (unsigned)C), dim3(SL_THREADS), 0, s, order, labels, keys,
                       tiles, count, n, C, ignore_index, nt, weight, slab);
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(SL_THREADS), 0, s, slab, nt, C, loss_weight, out, count);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_lovasz_bwd(const float* dloss, const float* logits, const int64_t* labels, const float* weight,
                               const int32_t* count, int64_t n, int C, int64_t ignore_index, float loss_weight,
                               float* dlogits, void* stream) {
  const int rc = seg_loss_check("lovasz_bwd", logits, labels, n, C);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(n == 0 || (dloss && weight && count && dlogits), "lovasz_bwd: dloss / weight / count / dlogits is NULL");
  PTV3_REQUIRE(sl_aligned16(weight) && sl_aligned16(dlogits), "lovasz_bwd: weight / dlogits must be 16-byte aligned");
  if (n == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  const int g = sl_group(C);
  by_value<2, 4, 8, 16, 32, 64>(g, [&](auto G) {
    hipLaunchKernelGGL(lovasz_bwd_kernel<G()>, dim3(sl_row_blocks(n, G())), dim3(SL_THREADS), 0, s, dloss, logits, labels,
                       weight, count, n, C, ignore_index, loss_weight, dlogits);
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" size_t ptv3_focal_workspace_bytes(int64_t n, int C) {
  if (n < 0) n = 0;
  if (C < 0) C = 0;
  const int64_t chunks = cdiv(n * C, FL_CHUNK);
  return sl_align256((size_t)chunks * 8) + sl_align256((size_t)chunks * 4);
}

extern "C" int ptv3_focal_fwd(const float* logits, const int64_t* labels, const float* alpha, int64_t n, int C,
                              int64_t ignore_index, float gamma, float loss_weight, int mean, float* out,
                              int32_t* nvalid, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = seg_loss_check("focal_fwd", logits, labels, n, C);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(alpha && out && nvalid, "focal_fwd: alpha / out / nvalid is NULL");
  PTV3_REQUIRE(gamma == gamma && gamma >= 0.f, "focal_fwd: gamma must be a non-negative number");
  PTV3_REQUIRE(workspace && sl_aligned16(workspace), "focal_fwd: workspace must be 16-byte aligned");
  PTV3_REQUIRE(workspace_bytes >= ptv3_focal_workspace_bytes(n, C), "focal_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = n * C, chunks = cdiv(total, FL_CHUNK);
  double* slab_sum = (double*)workspace;
  int32_t* slab_rows = (int32_t*)((char*)workspace + sl_align256((size_t)chunks * 8));
  if (chunks)
    hipLaunchKernelGGL(focal_partial_kernel, dim3((unsigned)chunks), dim3(SL_THREADS), 0, s, logits, labels, alpha, total,
                       C, ignore_index, gamma, slab_sum, slab_rows);
  hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(SL_THREADS), 0, s, slab_sum, slab_rows, chunks, C, loss_weight,
                     mean, out, nvalid);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_focal_bwd(const float* dloss, const float* logits, const int64_t* labels, const float* alpha,
                              const int32_t* nvalid, int64_t n, int C, int64_t ignore_index, float gamma,
                              float loss_weight, int mean, float* dlogits, void* stream) {
  const int rc = seg_loss_check("focal_bwd", logits, labels, n, C);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(n == 0 || (dloss && alpha && nvalid && dlogits), "focal_bwd: dloss / alpha / nvalid / dlogits is NULL");
  PTV3_REQUIRE(gamma == gamma && gamma >= 0.f, "focal_bwd: gamma must be a non-negative number");
  if (n == 0) return PTV3_OK;
  const int64_t total = n * C;
  int64_t blocks = cdiv(total, SL_THREADS);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(focal_bwd_kernel, dim3((unsigned)blocks), dim3(SL_THREADS), 0, (hipStream_t)stream, dloss, logits,
                     labels, alpha, nvalid, total, C, ignore_index, gamma, loss_weight, mean, dlogits);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
