// Head of the context-aware classifier ("CAC-v1m1", context_aware_classifier_v1m1_base.py): the three loops of
// full-size tensor operations of the reference as one pass over the points each, nothing read back by the host.
//   cac_proto_partial_kernel<LABEL>  a workgroup per chunk of CAC_CHUNK points that never straddles a scene: tiles of
//                                    CAC_P points in LDS (x with a column of ones appended, the K weights of each
//                                    point - masked softmax or one-hot label - computed by an 8-lane group in
//                                    registers), a (K, C + 1) accumulator in LDS, every entry owned by one thread
//   cac_proto_reduce_kernel          the chunks of a scene in increasing order (float64), the division, den / count
//   cac_proto_bwd_kernel             dx = w . (dproto / (den + eps)); the weights recomputed by the forward's code
//   cac_cos_logits_kernel            prototypes of the scene normalised into LDS (transposed), rows normalised into LDS,
//                                    (N, K) written once
//   cac_distill_partial_kernel       per point softmax(soft), log_softmax(pred), loss and entropy; per class sums of a
//                                    chunk of CAC_DCHUNK points in point order
//   cac_distill_finish_kernel        one workgroup: per class the chunks in order (float64), the ratios, the loss, and
//                                    the per-class factor of the backward
//   cac_distill_bwd_kernel           dpred in one launch
// Every hand-off between workgroups is a kernel boundary; no atomics at all, so two runs are bitwise equal.
#include "common.h"
#include "scene_chunks.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int CAC_THREADS = 256;
constexpr int CAC_G = 8;                        // lanes that share one point in the row phases
constexpr int CAC_P = CAC_THREADS / CAC_G;      // points per LDS tile
constexpr int CAC_CHUNK = 2048;                 // points per workgroup (prototypes, cosine logits)
constexpr int CAC_DCHUNK = 1024;                // points per workgroup (distillation partials)
constexpr int CAC_MAX_K = 256, CAC_MAX_C = 128;
constexpr size_t CAC_MAX_LDS = 144 * 1024;

__device__ __forceinline__ float cac_gmax(float v) {
#pragma unroll
  for (int m = CAC_G >> 1; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float cac_gsum(float v) {
#pragma unroll
  for (int m = CAC_G >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// softmax statistics of one row held by a CAC_G-lane group (lane l takes k = l, l + G, ...): p_k = expf(x_k - mx) * inv
__device__ __forceinline__ void cac_row_stats(const float* __restrict__ x, int K, int l, bool active, float* mx,
                                              float* sum) {
  float m = -3.0e38f;
  if (active)
    for (int k = l; k < K; k += CAC_G) m = fmaxf(m, x[k]);
  m = cac_gmax(m);
  float s = 0.f;
  if (active)
    for (int k = l; k < K; k += CAC_G) s += expf(x[k] - m);
  s = cac_gsum(s);
  *mx = m;
  *sum = active ? s : 1.f;
}

// the K weights of row `row` into w[k * ks] for k = l, l + G, ... < Kp (zeros from K on and for an inactive row).
// Softmax: p_k, all of them zero when conf > 0 and the largest p (= 1 / sum) is below conf.  Label: 1 at the label.
template <bool LABEL>
__device__ __forceinline__ void cac_weights(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                            int64_t row, bool active, int K, int Kp, float conf, int l,
                                            float* __restrict__ w, int ks) {
  if (LABEL) {
    const int64_t lab = active ? labels[row] : -1;
    for (int k = l; k < Kp; k += CAC_G) w[k * ks] = (lab == (int64_t)k && k < K) ? 1.f : 0.f;
  } else {
    const float* x = logits + (active ? row : 0) * K;
    float mx, sum;
    cac_row_stats(x, K, l, active, &mx, &sum);
    const float inv = 1.f / sum;
    const bool keep = active && !(conf > 0.f && inv < conf);
    for (int k = l; k < Kp; k += CAC_G) w[k * ks] = (keep && k < K) ? expf(x[k] - mx) * inv : 0.f;
  }
}

// the scene and the rows of chunk id j (scene_chunks.h); offset == NULL: one scene of n rows.  Synchronises.
__device__ __forceinline__ int cac_chunk(const int64_t* __restrict__ offset, int nb, int64_t n, int64_t j, int64_t* r0,
                                         int64_t* r1) {
  int b = 0;
  int64_t s = 0, e = n;
  if (offset) {
    b = scene_of_chunk<CAC_THREADS>(offset, nb, n, CAC_CHUNK, j);
    scene_bounds(offset, b, n, &s, &e);
  }
  chunk_rows(j, b, s, e, CAC_CHUNK, r0, r1);
  return b;
}

// slab[j][Kp][C + 1]: column C holds the sum of the weights
template <bool LABEL>
__global__ void __launch_bounds__(CAC_THREADS) cac_proto_partial_kernel(
    const float* __restrict__ x, const float* __restrict__ logits, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ offset, int nb, int64_t n, int K, int C, float conf, float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) float cac_lds[];
  const int Kp = (K + 3) & ~3, C1 = C + 1;
  float* acc = cac_lds;              // [Kp][C1]
  float* xs = acc + Kp * C1;         // [P][C1]
  float* ps = xs + CAC_P * C1;       // [P][Kp], 16-byte aligned rows
  int64_t r0, r1;
  cac_chunk(offset, nb, n, blockIdx.x, &r0, &r1);
  if (r1 <= r0) return;              // an unused id: the reduction never reads its slab
  const int tid = threadIdx.x, g = tid / CAC_G, l = tid % CAC_G;
  for (int i = tid; i < Kp * C1; i += CAC_THREADS) acc[i] = 0.f;
  const int nt = (Kp >> 2) * C1;
  for (int64_t t0 = r0; t0 < r1; t0 += CAC_P) {
    for (int i = tid; i < CAC_P * C1; i += CAC_THREADS) {
      const int p = i / C1, c = i - p * C1;
      const int64_t row = t0 + p;
      xs[i] = row < r1 ? (c < C ? x[row * C + c] : 1.f) : 0.f;
    }
    cac_weights<LABEL>(logits, labels, t0 + g, t0 + g < r1, K, Kp, conf, l, ps + g * Kp, 1);
    __syncthreads();
    for (int e = tid; e < nt; e += CAC_THREADS) {
      const int k4 = e / C1, c = e - k4 * C1;
      float* a = acc + (k4 * 4) * C1 + c;
      // a tile's sum starts at zero and joins the chunk's once: blocked summation, 32 + 64 terms deep, not 2048
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
      for (int p = 0; p < CAC_P; ++p) {
        const float xv = xs[p * C1 + c];
        const f32x4 w = *reinterpret_cast<const f32x4*>(ps + p * Kp + k4 * 4);
        a0 = fmaf(w[0], xv, a0); a1 = fmaf(w[1], xv, a1); a2 = fmaf(w[2], xv, a2); a3 = fmaf(w[3], xv, a3);
      }
      a[0] += a0; a[C1] += a1; a[2 * C1] += a2; a[3 * C1] += a3;
    }
    __syncthreads();
  }
  float* out = slab + (int64_t)blockIdx.x * Kp * C1;
  for (int i = tid; i < Kp * C1; i += CAC_THREADS) out[i] = acc[i];
}

// proto[b][k][c] = num / (den + eps); den[b][k]; count[k] = (int) den (label mode, exact: float64 sums of integers)
__global__ void __launch_bounds__(CAC_THREADS) cac_proto_reduce_kernel(
    const float* __restrict__ slab, const int64_t* __restrict__ offset, int64_t n, int K, int C, float eps,
    float* __restrict__ proto, float* __restrict__ den, int32_t* __restrict__ count) {
  const int Kp = (K + 3) & ~3, C1 = C + 1, b = blockIdx.y;
  const int i = blockIdx.x * CAC_THREADS + threadIdx.x;
  if (i >= K * C) return;
  const int k = i / C, c = i - k * C;
  int64_t s = 0, e = n;
  if (offset) scene_bounds(offset, b, n, &s, &e);
  const int64_t j0 = s / CAC_CHUNK + b, nblk = scene_nblk(s, e, CAC_CHUNK);
  double num = 0.0, d = 0.0;
  for (int64_t j = j0; j < j0 + nblk; ++j) {
    const float* row = slab + (j * Kp + k) * C1;
    num += (double)row[c];
    d += (double)row[C];
  }
  proto[((int64_t)b * K + k) * C + c] = (float)num / ((float)d + eps);
  if (c == 0) {
    den[(int64_t)b * K + k] = (float)d;
    if (count) count[k] = (int32_t)d;
  }
}

// dx[i][c] = sum_k w[i][k] * dproto[b][k][c] / (den[b][k] + eps)
template <bool LABEL>
__global__ void __launch_bounds__(CAC_THREADS) cac_proto_bwd_kernel(
    const float* __restrict__ dproto, const float* __restrict__ den, const float* __restrict__ logits,
    const int64_t* __restrict__ labels, const int64_t* __restrict__ offset, int nb, int64_t n, int K, int C, float conf,
    float eps, float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float cac_lds[];
  const int Kp = (K + 3) & ~3;
  float* gs = cac_lds;               // [Kp][C]
  float* wt = gs + Kp * C;           // [Kp][P]: 16-byte aligned rows (Kp * C is a multiple of 4)
  int64_t r0, r1;
  const int b = cac_chunk(offset, nb, n, blockIdx.x, &r0, &r1);
  if (r1 <= r0) return;
  const int tid = threadIdx.x, g = tid / CAC_G, l = tid % CAC_G;
  for (int i = tid; i < Kp * C; i += CAC_THREADS) {
    const int k = i / C;
    gs[i] = k < K ? dproto[(int64_t)b * K * C + i] / (den[(int64_t)b * K + k] + eps) : 0.f;
  }
  const int nt = (CAC_P >> 2) * C;
  for (int64_t t0 = r0; t0 < r1; t0 += CAC_P) {
    __syncthreads();                 // gs is complete; the previous tile's reads of wt are over
    cac_weights<LABEL>(logits, labels, t0 + g, t0 + g < r1, K, Kp, conf, l, wt + g, CAC_P);
    __syncthreads();
    for (int e = tid; e < nt; e += CAC_THREADS) {
      const int pg = e / C, c = e - pg * C;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
      for (int k = 0; k < Kp; ++k) {
        const float gv = gs[k * C + c];
        const f32x4 w = *reinterpret_cast<const f32x4*>(wt + k * CAC_P + pg * 4);
        a0 = fmaf(w[0], gv, a0); a1 = fmaf(w[1], gv, a1); a2 = fmaf(w[2], gv, a2); a3 = fmaf(w[3], gv, a3);
      }
      const int64_t row = t0 + pg * 4;
      if (row < r1) dx[row * C + c] = a0;
      if (row + 1 < r1) dx[(row + 1) * C + c] = a1;
      if (row + 2 < r1) dx[(row + 2) * C + c] = a2;
      if (row + 3 < r1) dx[(row + 3) * C + c] = a3;
    }
  }
}

// out[i][k] = temp * <y_i / max(|y_i|, 1e-12), q_bk / max(|q_bk|, 1e-12)>; shared != 0: q is (1, K, C) for every scene
__global__ void __launch_bounds__(CAC_THREADS) cac_cos_logits_kernel(
    const float* __restrict__ y, const float* __restrict__ q, const int64_t* __restrict__ offset, int nb, int64_t n,
    int K, int C, int shared, float temp, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float cac_lds[];
  const int Kp = (K + 3) & ~3;
  float* qt = cac_lds;               // [C][Kp], 16-byte aligned rows
  float* ys = qt + C * Kp;           // [P][C]
  int64_t r0, r1;
  const int b = cac_chunk(offset, nb, n, blockIdx.x, &r0, &r1);
  if (r1 <= r0) return;
  const int tid = threadIdx.x, g = tid / CAC_G, l = tid % CAC_G;
  const float* qb = q + (shared ? 0 : (int64_t)b * K * C);
  for (int k0 = 0; k0 < Kp; k0 += CAC_P) {
    const int k = k0 + g;
    const bool real = k < K;
    float ss = 0.f;
    if (real)
      for (int c = l; c < C; c += CAC_G) ss = fmaf(qb[k * C + c], qb[k * C + c], ss);
    ss = cac_gsum(ss);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    if (k < Kp)
      for (int c = l; c < C; c += CAC_G) qt[c * Kp + k] = real ? qb[k * C + c] * inv : 0.f;
  }
  const int K4 = Kp >> 2, nt = CAC_P * K4;
  for (int64_t t0 = r0; t0 < r1; t0 += CAC_P) {
    __syncthreads();                 // qt is complete; the previous tile's reads of ys are over
    {
      const int64_t row = t0 + g;
      const bool active = row < r1;
      const float* yr = y + (active ? row : 0) * C;
      float ss = 0.f;
      if (active)
        for (int c = l; c < C; c += CAC_G) ss = fmaf(yr[c], yr[c], ss);
      ss = cac_gsum(ss);
      const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
      for (int c = l; c < C; c += CAC_G) ys[g * C + c] = active ? yr[c] * inv : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < nt; e += CAC_THREADS) {
      const int p = e / K4, k4 = e - p * K4;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
      for (int c = 0; c < C; ++c) {
        const float yv = ys[p * C + c];
        const f32x4 w = *reinterpret_cast<const f32x4*>(qt + c * Kp + k4 * 4);
        a0 = fmaf(yv, w[0], a0); a1 = fmaf(yv, w[1], a1); a2 = fmaf(yv, w[2], a2); a3 = fmaf(yv, w[3], a3);
      }
      const int64_t row = t0 + p;
      if (row < r1) {
        float* o = out + row * K + k4 * 4;
        const int k = k4 * 4;
        if (k < K) o[0] = a0 * temp;
        if (k + 1 < K) o[1] = a1 * temp;
        if (k + 2 < K) o[2] = a2 * temp;
        if (k + 3 < K) o[3] = a3 * temp;
      }
    }
  }
}

// ---- distillation loss (get_distill_loss, smoothness 0.5, eps 0) -------------------------------------------------
// One row by a CAC_G-lane group: *loss = -sum_k log_softmax(pred)_k s_k with s = 0.5 softmax(soft) + 0.5 onehot(cls),
// *ent = -sum_k p_k log(p_k + 1e-4), p = softmax(soft); the statistics come back for the backward.
__device__ __forceinline__ void cac_distill_row(const float* __restrict__ pred, const float* __restrict__ soft, int K,
                                                int cls, int l, bool active, float* loss, float* ent, float* ms,
                                                float* invs, float* mp, float* sp) {
  float sums;
  cac_row_stats(soft, K, l, active, ms, &sums);
  cac_row_stats(pred, K, l, active, mp, sp);
  *invs = 1.f / sums;
  const float lse = *mp + logf(*sp);
  float lo = 0.f, en = 0.f;
  if (active)
    for (int k = l; k < K; k += CAC_G) {
      const float p = expf(soft[k] - *ms) * *invs;
      const float s = 0.5f * p + (k == cls ? 0.5f : 0.f);
      lo -= (pred[k] - lse) * s;
      en -= p * logf(p + 1e-4f);
    }
  *loss = cac_gsum(lo);
  *ent = cac_gsum(en);
}

__device__ __forceinline__ bool cac_label_valid(int64_t lab, int K) { return lab >= 0 && lab < (int64_t)K; }

// part_le / part_e [chunk][K] fp32, part_n [chunk][K] int32
__global__ void __launch_bounds__(CAC_THREADS) cac_distill_partial_kernel(
    const float* __restrict__ pred, const float* __restrict__ soft, const int64_t* __restrict__ labels, int64_t n, int K,
    float* __restrict__ part_le, float* __restrict__ part_e, int32_t* __restrict__ part_n) {
  __shared__ float ple[CAC_DCHUNK], pe[CAC_DCHUNK];
  __shared__ int plab[CAC_DCHUNK];
  const int tid = threadIdx.x, g = tid / CAC_G, l = tid % CAC_G;
  const int64_t r0 = (int64_t)blockIdx.x * CAC_DCHUNK;
  const int cnt = (int)(n - r0 < CAC_DCHUNK ? n - r0 : CAC_DCHUNK);
  for (int t = 0; t < CAC_DCHUNK; t += CAC_P) {
    const int i = t + g;
    const bool active = i < cnt;
    const int64_t row = r0 + (active ? i : 0);
    const int64_t lab = active ? labels[row] : -1;
    const bool valid = active && cac_label_valid(lab, K);
    float loss, ent, ms, invs, mp, sp;
    cac_distill_row(pred + row * K, soft + row * K, K, valid ? (int)lab : 0, l, active, &loss, &ent, &ms, &invs, &mp,
                    &sp);
    if (l == 0) {
      ple[i] = valid ? loss * ent : 0.f;
      pe[i] = valid ? ent : 0.f;
      plab[i] = valid ? (int)lab : -1;
    }
  }
  __syncthreads();
  for (int k = tid; k < K; k += CAC_THREADS) {
    float a = 0.f, e = 0.f;
    int c = 0;
    for (int i = 0; i < cnt; ++i)
      if (plab[i] == k) { a += ple[i]; e += pe[i]; ++c; }
    const int64_t o = (int64_t)blockIdx.x * K + k;
    part_le[o] = a; part_e[o] = e; part_n[o] = c;
  }
}

// out[0] = sum over present classes of LE_k / (E_k + 1e-4), / (n_present + 1e-4); coef[k] = the backward's per-class
// factor 1 / ((n_present + 1e-4)(E_k + 1e-4)), 0 for an absent class; count[k], count[K] = n_present
__global__ void __launch_bounds__(CAC_THREADS) cac_distill_finish_kernel(
    const float* __restrict__ part_le, const float* __restrict__ part_e, const int32_t* __restrict__ part_n,
    int64_t chunks, int K, float* __restrict__ out, float* __restrict__ coef, int32_t* __restrict__ count) {
  __shared__ double red[CAC_THREADS];
  __shared__ int redc[CAC_THREADS];
  double ratios = 0.0;
  int present = 0;
  for (int k = threadIdx.x; k < K; k += CAC_THREADS) {
    double le = 0.0, e = 0.0;
    long long c = 0;
    for (int64_t j = 0; j < chunks; ++j) {
      le += (double)part_le[j * K + k];
      e += (double)part_e[j * K + k];
      c += part_n[j * K + k];
    }
    const float ef = (float)e + 1e-4f;
    if (c > 0) { ratios += (double)((float)le / ef); ++present; }
    coef[k] = c > 0 ? 1.f / ef : 0.f;
    count[k] = (int32_t)(c > 0x7fffffffLL ? 0x7fffffffLL : c);
  }
  red[threadIdx.x] = ratios;
  redc[threadIdx.x] = present;
  for (int d = CAC_THREADS >> 1; d >= 1; d >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < d) {
      red[threadIdx.x] += red[threadIdx.x + d];
      redc[threadIdx.x] += redc[threadIdx.x + d];
    }
  }
  __syncthreads();
  const int np = redc[0];
  const float scale = np > 0 ? 1.f / ((float)np + 1e-4f) : 0.f;
  for (int k = threadIdx.x; k < K; k += CAC_THREADS) coef[k] *= scale;   // each thread rewrites its own entries
  if (threadIdx.x == 0) {
    out[0] = np > 0 ? (float)red[0] * scale : 0.f;
    count[K] = np;
  }
}

// dpred[i][k] = dloss * coef[t_i] * ent_i * (softmax(pred)_k - s_k) for a valid row, else 0
__global__ void __launch_bounds__(CAC_THREADS) cac_distill_bwd_kernel(
    const float* __restrict__ dloss, const float* __restrict__ pred, const float* __restrict__ soft,
    const int64_t* __restrict__ labels, const float* __restrict__ coef, int64_t n, int K, float* __restrict__ dpred) {
  const int tid = threadIdx.x, g = tid / CAC_G, l = tid % CAC_G;
  const float dl = dloss[0];
  for (int64_t rb = (int64_t)blockIdx.x * CAC_P; rb < n; rb += (int64_t)gridDim.x * CAC_P) {
    const int64_t r = rb + g;
    const bool active = r < n;
    const int64_t row = active ? r : 0;
    const int64_t lab = active ? labels[row] : -1;
    const bool valid = active && cac_label_valid(lab, K);
    const float* pr = pred + row * K;
    const float* so = soft + row * K;
    float loss, ent, ms, invs, mp, sp;
    cac_distill_row(pr, so, K, valid ? (int)lab : 0, l, active, &loss, &ent, &ms, &invs, &mp, &sp);
    if (!active) continue;
    const float f = valid ? dl * coef[lab] * ent : 0.f;
    const float invp = 1.f / sp;
    for (int k = l; k < K; k += CAC_G) {
      float d = 0.f;
      if (valid) {
        const float p = expf(so[k] - ms) * invs;
        const float s = 0.5f * p + (k == (int)lab ? 0.5f : 0.f);
        d = f * (expf(pr[k] - mp) * invp - s);
      }
      dpred[row * K + k] = d;
    }
  }
}

static inline int cac_kp(int K) { return (K + 3) & ~3; }
static size_t cac_proto_lds(int K, int C) { return sizeof(float) * ((size_t)cac_kp(K) * (C + 1) + (size_t)CAC_P * (C + 1 + cac_kp(K))); }
static size_t cac_bwd_lds(int K, int C) { return sizeof(float) * ((size_t)cac_kp(K) * C + (size_t)cac_kp(K) * CAC_P); }
static size_t cac_cos_lds(int K, int C) { return sizeof(float) * ((size_t)cac_kp(K) * C + (size_t)CAC_P * C); }
static bool cac_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int cac_check(const char* who, int64_t n, int K, int C, int nb) {
  PTV3_REQUIRE(ptv3_cac_capable(K, C), "%s: K=%d, C=%d outside the limits (ptv3_cac_capable)", who, K, C);
  PTV3_REQUIRE(n >= 0 && n < (1ll << 31) && nb >= 1 && nb <= (1 << 20), "%s: n=%lld, scenes=%d unsupported", who,
               (long long)n, nb);
  return PTV3_OK;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_cac_capable(int K, int C) {
  if (K < 2 || K > CAC_MAX_K || C < 1 || C > CAC_MAX_C) return 0;
  return cac_proto_lds(K, C) <= CAC_MAX_LDS && cac_bwd_lds(K, C) <= CAC_MAX_LDS && cac_cos_lds(K, C) <= CAC_MAX_LDS;
}

extern "C" size_t ptv3_cac_proto_workspace_bytes(int64_t n, int K, int C, int nb) {
  if (n < 0) n = 0;
  if (K < 0 || C < 0 || nb < 0) return 0;
  return (size_t)(cdiv(n, CAC_CHUNK) + nb) * cac_kp(K) * (C + 1) * sizeof(float);
}

extern "C" int ptv3_cac_proto_fwd(const float* x, const float* logits, const int64_t* labels, const int64_t* offset,
                                  int nb, int64_t n, int K, int C, float conf_thresh, float* proto, float* den,
                                  int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  const bool label = labels != nullptr;
  if (label) nb = 1;
  const int rc = cac_check("cac_proto_fwd", n, K, C, nb);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE((logits != nullptr) != label, "cac_proto_fwd: give logits (softmax weights) or labels, not both");
  PTV3_REQUIRE(label || offset, "cac_proto_fwd: the softmax form needs the scene offsets");
  PTV3_REQUIRE(proto && den && (n == 0 || x), "cac_proto_fwd: x / proto / den is NULL");
  PTV3_REQUIRE(workspace && cac_aligned16(workspace) && workspace_bytes >= ptv3_cac_proto_workspace_bytes(n, K, C, nb),
               "cac_proto_fwd: workspace missing, unaligned or too small");
  hipStream_t s = (hipStream_t)stream;
  const unsigned chunks = (unsigned)(cdiv(n, CAC_CHUNK) + nb);
  const size_t lds = cac_proto_lds(K, C);
  float* slab = (float*)workspace;
  const int64_t* off = label ? nullptr : offset;
  if (n > 0) {
    if (label) {
      ensure_dynamic_lds((const void*)cac_proto_partial_kernel<true>, (int)lds);
      hipLaunchKernelGGL(cac_proto_partial_kernel<true>, dim3(chunks), dim3(CAC_THREADS), lds, s, x, logits, labels, off,
                         nb, n, K, C, 0.f, slab);
    } else {
      ensure_dynamic_lds((const void*)cac_proto_partial_kernel<false>, (int)lds);
      hipLaunchKernelGGL(cac_proto_partial_kernel<false>, dim3(chunks), dim3(CAC_THREADS), lds, s, x, logits, labels, off,
                         nb, n, K, C, conf_thresh, slab);
    }
  }
  hipLaunchKernelGGL(cac_proto_reduce_kernel, dim3((unsigned)cdiv((int64_t)K * C, CAC_THREADS), (unsigned)nb),
                     dim3(CAC_THREADS), 0, s, slab, off, n, K, C, label ? 1e-4f : 1e-7f, proto, den,
                     label ? count : nullptr);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cac_proto_bwd(const float* dproto, const float* den, const float* logits, const int64_t* labels,
                                  const int64_t* offset, int nb, int64_t n, int K, int C, float conf_thresh, float* dx,
                                  void* stream) {
  const bool label = labels != nullptr;
  if (label) nb = 1;
  const int rc = cac_check("cac_proto_bwd", n, K, C, nb);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE((logits != nullptr) != label, "cac_proto_bwd: give logits (softmax weights) or labels, not both");
  PTV3_REQUIRE(label || offset, "cac_proto_bwd: the softmax form needs the scene offsets");
  PTV3_REQUIRE(dproto && den && (n == 0 || dx), "cac_proto_bwd: dproto / den / dx is NULL");
  if (n == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned chunks = (unsigned)(cdiv(n, CAC_CHUNK) + nb);
  const size_t lds = cac_bwd_lds(K, C);
  if (label) {
    ensure_dynamic_lds((const void*)cac_proto_bwd_kernel<true>, (int)lds);
    hipLaunchKernelGGL(cac_proto_bwd_kernel<true>, dim3(chunks), dim3(CAC_THREADS), lds, s, dproto, den, logits, labels,
                       (const int64_t*)nullptr, nb, n, K, C, 0.f, 1e-4f, dx);
  } else {
    ensure_dynamic_lds((const void*)cac_proto_bwd_kernel<false>, (int)lds);
    hipLaunchKernelGGL(cac_proto_bwd_kernel<false>, dim3(chunks), dim3(CAC_THREADS), lds, s, dproto, den, logits, labels,
                       offset, nb, n, K, C, conf_thresh, 1e-7f, dx);
  }
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cac_cos_logits_fwd(const float* y, const float* q, const int64_t* offset, int nb, int64_t n, int K,
                                       int C, int shared, float temp, float* out, void* stream) {
  if (shared) nb = 1;
  const int rc = cac_check("cac_cos_logits_fwd", n, K, C, nb);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(q && (shared || offset) && (n == 0 || (y && out)), "cac_cos_logits_fwd: y / q / offset / out is NULL");
  if (n == 0) return PTV3_OK;
  const unsigned chunks = (unsigned)(cdiv(n, CAC_CHUNK) + nb);
  const size_t lds = cac_cos_lds(K, C);
  ensure_dynamic_lds((const void*)cac_cos_logits_kernel, (int)lds);
  hipLaunchKernelGGL(cac_cos_logits_kernel, dim3(chunks), dim3(CAC_THREADS), lds, (hipStream_t)stream, y, q,
                     shared ? (const int64_t*)nullptr : offset, nb, n, K, C, shared, temp, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

// part_le (chunks, K) f32 | part_e (chunks, K) f32 | part_n (chunks, K) i32
extern "C" size_t ptv3_cac_distill_workspace_bytes(int64_t n, int K) {
  if (n < 0) n = 0;
  if (K < 0) K = 0;
  return (size_t)cdiv(n, CAC_DCHUNK) * K * 12 + 16;
}

extern "C" int ptv3_cac_distill_fwd(const float* pred, const float* soft, const int64_t* labels, int64_t n, int K,
                                    float* out, float* coef, int32_t* count, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  PTV3_REQUIRE(K >= 2 && K <= CAC_MAX_K, "cac_distill_fwd: K=%d unsupported (2 to %d classes)", K, CAC_MAX_K);
  PTV3_REQUIRE(n >= 0 && n < (1ll << 31), "cac_distill_fwd: n=%lld unsupported", (long long)n);
  PTV3_REQUIRE(out && coef && count && (n == 0 || (pred && soft && labels)), "cac_distill_fwd: a pointer is NULL");
  PTV3_REQUIRE(workspace && cac_aligned16(workspace) && workspace_bytes >= ptv3_cac_distill_workspace_bytes(n, K),
               "cac_distill_fwd: workspace missing, unaligned or too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = cdiv(n, CAC_DCHUNK);
  float* part_le = (float*)workspace;
  float* part_e = part_le + chunks * K;
  int32_t* part_n = (int32_t*)(part_e + chunks * K);
  if (chunks)
    hipLaunchKernelGGL(cac_distill_partial_kernel, dim3((unsigned)chunks), dim3(CAC_THREADS), 0, s, pred, soft, labels, n,
                       K, part_le, part_e, part_n);
  hipLaunchKernelGGL(cac_distill_finish_kernel, dim3(1), dim3(CAC_THREADS), 0, s, part_le, part_e, part_n, chunks, K, out,
                     coef, count);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cac_distill_bwd(const float* dloss, const float* pred, const float* soft, const int64_t* labels,
                                    const float* coef, int64_t n, int K, float* dpred, void* stream) {
  PTV3_REQUIRE(K >= 2 && K <= CAC_MAX_K, "cac_distill_bwd: K=%d unsupported (2 to %d classes)", K, CAC_MAX_K);
  PTV3_REQUIRE(n >= 0 && n < (1ll << 31), "cac_distill_bwd: n=%lld unsupported", (long long)n);
  PTV3_REQUIRE(n == 0 || (dloss && pred && soft && labels && coef && dpred), "cac_distill_bwd: a pointer is NULL");
  if (n == 0) return PTV3_OK;
  int64_t blocks = cdiv(n, CAC_P);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cac_distill_bwd_kernel, dim3((unsigned)blocks), dim3(CAC_THREADS), 0, (hipStream_t)stream, dloss,
                     pred, soft, labels, coef, n, K, dpred);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
