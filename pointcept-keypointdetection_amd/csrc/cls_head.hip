// Classifier / regressor head of DefaultClassifier and PigBodyRegressor, written for the BATCH of pooled rows:
//   Linear(C, H1) -> BatchNorm1d -> ReLU -> Dropout -> Linear(H1, H2) -> BatchNorm1d -> ReLU -> Dropout -> Linear(H2, out)
// followed, on request, by the L1 loss and the per-column mean absolute errors.  B is 4 .. 32 rows, so every kernel
// here is ONE workgroup (or a grid of independent elements): each weight is read once for all rows, rows are walked
// in tiles of CH_RT with the tile in LDS and one output column per thread (the rows are register accumulators).
//   cls_head_eval_kernel        per-scene slab sums (the order of scene_mean_finish_kernel) -> folded-BatchNorm head
//                               -> logits, loss, column errors; weights TRANSPOSED (K, outs), loads coalesce over outs
//   cls_head_train_fwd_kernel   batch-statistic BatchNorm (two-pass variance, running statistics updated), keep-masks,
//                               nn.Linear's own (outs, K) weights read as 16-byte pieces along K
//   cls_head_train_bwd_kernel   the activation-gradient chain down to dg, bias and BatchNorm affine gradients
//   cls_head_wgrad_kernel       dW1, dW2, dW3: one thread per element, a sum over the rows in row order
// No atomics anywhere; every sum has a fixed order, so two runs are bitwise equal.
#include "common.h"
#include "scene_chunks.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int CH_RT = PTV3_CLS_HEAD_ROW_TILE;   // rows (scenes) per tile
constexpr int CH_MAX_C = 1024;                  // pooled width = the LDS row length of a tile
constexpr int CH_MAX_H = 512;                   // hidden widths and out
constexpr int CE_THREADS = 1024;                // eval: the lane count of scene_mean_finish_kernel (same slab order)
constexpr int CT_THREADS = 256;                 // training kernels

// acc[r] = sum_k xs[r][k] wt[k][o]: weights (K, outs), lanes along o.  U loads are issued before the first use.
template <int LDX, int U>
__device__ __forceinline__ void dot_wt(const float* xs, int K, const float* __restrict__ wt, int outs, int o,
                                       float (&acc)[CH_RT]) {
#pragma unroll
  for (int r = 0; r < CH_RT; ++r) acc[r] = 0.f;
  const float* wp = wt + o;
  int k = 0;
  for (; k + U <= K; k += U) {
    float w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = wp[(int64_t)(k + u) * outs];
    // blocked summation: a trip's U products are summed on their own, then added (the rounding error grows with
    // U + K / U instead of K, and the trips' chains are independent)
    float part[CH_RT];
#pragma unroll
    for (int r = 0; r < CH_RT; ++r) part[r] = xs[r * LDX + k] * w[0];
#pragma unroll
    for (int u = 1; u < U; ++u)
#pragma unroll
      for (int r = 0; r < CH_RT; ++r) part[r] = fmaf(xs[r * LDX + k + u], w[u], part[r]);
#pragma unroll
    for (int r = 0; r < CH_RT; ++r) acc[r] += part[r];
  }
  for (; k < K; ++k) {
    const float w = wp[(int64_t)k * outs];
#pragma unroll
    for (int r = 0; r < CH_RT; ++r) acc[r] = fmaf(xs[r * LDX + k], w, acc[r]);
  }
}

// acc[r] = sum_k xs[r][k] w[k]: one row of an (outs, K) weight per thread, 16 bytes per load when the row allows it.
template <int LDX>
__device__ __forceinline__ void dot_w(const float* xs, int K, const float* __restrict__ w, bool vec,
                                      float (&acc)[CH_RT]) {
#pragma unroll
  for (int r = 0; r < CH_RT; ++r) acc[r] = 0.f;
  int k = 0;
  if (vec) {
    for (; k + 16 <= K; k += 16) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(w + k + 4 * u);
      float part[CH_RT];   // blocked summation, as in dot_wt
#pragma unroll
      for (int r = 0; r < CH_RT; ++r) part[r] = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int r = 0; r < CH_RT; ++r) part[r] = fmaf(xs[r * LDX + k + 4 * u + q], v[u][q], part[r]);
#pragma unroll
      for (int r = 0; r < CH_RT; ++r) acc[r] += part[r];
    }
    for (; k + 4 <= K; k += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < CH_RT; ++r) acc[r] = fmaf(xs[r * LDX + k + q], v[q], acc[r]);
    }
  } else {
    for (; k + 4 <= K; k += 4) {
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = w[k + q];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < CH_RT; ++r) acc[r] = fmaf(xs[r * LDX + k + q], v[q], acc[r]);
    }
  }
  for (; k < K; ++k) {
    const float v = w[k];
#pragma unroll
    for (int r = 0; r < CH_RT; ++r) acc[r] = fmaf(xs[r * LDX + k], v, acc[r]);
  }
}

// rows [t0, t0 + rows) of x (nb, K) -> xs[r][k]; the rows of a short last tile are zero
template <int THREADS, int LDX>
__device__ __forceinline__ void stage_rows(const float* x, int K, int t0, int rows, float* xs) {
  for (int i = threadIdx.x; i < CH_RT * K; i += THREADS) {
    const int r = i / K, k = i - r * K;
    xs[r * LDX + k] = r < rows ? x[(int64_t)(t0 + r) * K + k] : 0.f;
  }
}

// loss and column errors from the per-column sums of |logit - target| (cs, in LDS): fixed order
__device__ __forceinline__ void write_stats(const float* cs, int nb, int out, float loss_weight, float metric_scale,
                                            float* __restrict__ stats) {
  const int t = threadIdx.x;
  if (t == 0) {
    float tot = 0.f;
    for (int o = 0; o < out; ++o) tot += cs[o];
    stats[0] = loss_weight * (tot / ((float)nb * (float)out));
  }
  for (int o = t; o < out; o += blockDim.x) stats[1 + o] = metric_scale * (cs[o] / (float)nb);
}

__global__ void __launch_bounds__(CE_THREADS) cls_head_eval_kernel(
    const float* __restrict__ slab, const int64_t* __restrict__ offset, int64_t n, int c, int64_t rb, int nb,
    const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ s1,
    const float* __restrict__ t1, int h1, const float* __restrict__ w2t, const float* __restrict__ b2,
    const float* __restrict__ s2, const float* __restrict__ t2, int h2, const float* __restrict__ w3t,
    const float* __restrict__ b3, int out, const float* __restrict__ target, float loss_weight, float metric_scale,
    float* __restrict__ logits, float* __restrict__ stats) {
  __shared__ float lds[CH_RT * CH_MAX_C + CH_RT * CH_MAX_H];
  float* bufA = lds;                       // pooled rows of the tile, later the second hidden activation
  float* bufB = lds + CH_RT * CH_MAX_C;    // first hidden activation; the slab-sum tree while the rows are pooled
  f32x4* red = reinterpret_cast<f32x4*>(bufB);
  static_assert(CH_RT * CH_MAX_H * sizeof(float) >= CE_THREADS * sizeof(f32x4), "tree scratch");
  const int t = threadIdx.x;
  const int cv4 = c / 4, lanes = CE_THREADS / cv4;
  const int cv = t % cv4, z = t / cv4;
  int p2 = 1;
  while (p2 < lanes) p2 <<= 1;
  float colsum = 0.f;   // thread o < out: sum over the rows, in row order, of |logit - target|
  for (int t0 = 0; t0 < nb; t0 += CH_RT) {
    const int rows = nb - t0 < CH_RT ? nb - t0 : CH_RT;
    for (int i = 0; i < CH_RT; ++i) {
      if (i >= rows) {   // uniform
        if (z == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) bufA[i * CH_MAX_C + 4 * cv + q] = 0.f;
        }
        continue;
      }
      // scene t0 + i: the sum of scene_mean_finish_kernel, lane for lane
      int64_t s, e;
      scene_bounds(offset, t0 + i, n, &s, &e);
      const int64_t first = s / rb + (t0 + i), nblk = scene_nblk(s, e, rb);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (z < lanes) {
        int64_t k = z;
        for (; k + 3 * lanes < nblk; k += 4 * lanes) {
          f32x4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            v[u] = *reinterpret_cast<const f32x4*>(slab + (first + k + u * lanes) * c + 4 * cv);
#pragma unroll
          for (int u = 0; u < 4; ++u) acc += v[u];
        }
        for (; k < nblk; k += lanes) acc += *reinterpret_cast<const f32x4*>(slab + (first + k) * c + 4 * cv);
        red[z * cv4 + cv] = acc;
      }
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
#pragma unroll
        for (int q = 0; q < 4; ++q) bufA[i * CH_MAX_C + 4 * cv + q] = m[q];
      }
      __syncthreads();   // the tree scratch is free for the next scene
    }
    __syncthreads();
    float acc[CH_RT];
    for (int o = t; o < h1; o += CE_THREADS) {
      dot_wt<CH_MAX_C, 4>(bufA, c, w1t, h1, o, acc);
      const float bb = b1[o], sc = s1[o], sh = t1[o];
#pragma unroll
      for (int r = 0; r < CH_RT; ++r) bufB[r * CH_MAX_H + o] = fmaxf((acc[r] + bb) * sc + sh, 0.f);
    }
    __syncthreads();
    for (int o = t; o < h2; o += CE_THREADS) {
      dot_wt<CH_MAX_H, 4>(bufB, h1, w2t, h2, o, acc);
      const float bb = b2[o], sc = s2[o], sh = t2[o];
#pragma unroll
      for (int r = 0; r < CH_RT; ++r) bufA[r * CH_MAX_C + o] = fmaxf((acc[r] + bb) * sc + sh, 0.f);
    }
    __syncthreads();
    if (t < out) {   // out <= CH_MAX_H < CE_THREADS: one column per thread, so colsum stays in its register
      dot_wt<CH_MAX_C, 4>(bufA, h2, w3t, out, t, acc);
      const float bb = b3[t];
#pragma unroll
      for (int r = 0; r < CH_RT; ++r) {
        if (r < rows) {
          const float v = acc[r] + bb;
          logits[(int64_t)(t0 + r) * out + t] = v;
          if (target) colsum += fabsf(v - target[(int64_t)(t0 + r) * out + t]);
        }
      }
    }
    __syncthreads();
  }
  if (target) {
    if (t < out) bufA[t] = colsum;
    __syncthreads();
    write_stats(bufA, nb, out, loss_weight, metric_scale, stats);
  }
}

// z (nb, outs) = x (nb, K) w^T + bias, rows in tiles of CH_RT; ends with a barrier (z is visible to the workgroup)
__device__ __forceinline__ void train_linear(const float* x, int nb, int K, const float* __restrict__ w,
                                             const float* __restrict__ bias, int outs, float* z, float* xs) {
  const bool vec = K % 4 == 0 && ((uintptr_t)w & 15) == 0;
  for (int t0 = 0; t0 < nb; t0 += CH_RT) {
    const int rows = nb - t0 < CH_RT ? nb - t0 : CH_RT;
    stage_rows<CT_THREADS, CH_MAX_C>(x, K, t0, rows, xs);
    __syncthreads();
    for (int o = threadIdx.x; o < outs; o += CT_THREADS) {
      float acc[CH_RT];
      dot_w<CH_MAX_C>(xs, K, w + (int64_t)o * K, vec, acc);
      const float bb = bias[o];
#pragma unroll
      for (int r = 0; r < CH_RT; ++r)
        if (r < rows) z[(int64_t)(t0 + r) * outs + o] = acc[r] + bb;
    }
    __syncthreads();
  }
}

// a = relu(BatchNorm(z; batch statistics)) * mask * inv_keep.  A thread owns whole columns: it reads back only what it
// wrote itself.  Two-pass variance; running statistics as torch updates them (momentum, unbiased variance).
__device__ __forceinline__ void train_bn_relu_mask(const float* z, int nb, int H, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float* run_mean, float* run_var,
                                                   float momentum, float eps, const float* __restrict__ mask,
                                                   float inv_keep, float* a, float* mean_out, float* rstd_out) {
  for (int o = threadIdx.x; o < H; o += CT_THREADS) {
    float sum = 0.f;
#pragma unroll 4
    for (int r = 0; r < nb; ++r) sum += z[(int64_t)r * H + o];
    const float mean = sum / (float)nb;
    float sq = 0.f;
#pragma unroll 4
    for (int r = 0; r < nb; ++r) {
      const float d = z[(int64_t)r * H + o] - mean;
      sq = fmaf(d, d, sq);
    }
    const float var = sq / (float)nb;
    const float rstd = 1.0f / sqrtf(var + eps);
    run_mean[o] = (1.f - momentum) * run_mean[o] + momentum * mean;
    run_var[o] = (1.f - momentum) * run_var[o] + momentum * (sq / (float)(nb - 1));
    mean_out[o] = mean;
    rstd_out[o] = rstd;
    const float ga = gamma[o], be = beta[o];
#pragma unroll 4
    for (int r = 0; r < nb; ++r) {
      const int64_t i = (int64_t)r * H + o;
      const float y = fmaf((z[i] - mean) * rstd, ga, be);
      a[i] = fmaxf(y, 0.f) * (mask[i] * inv_keep);
    }
  }
  __syncthreads();
}

struct ClsSave {   // the forward's tape inside one buffer (ptv3_cls_head_save_floats)
  float *z1, *a1, *z2, *a2, *mean1, *rstd1, *mean2, *rstd2, *sgn;
  __host__ __device__ ClsSave(float* p, int nb, int h1, int h2, int out) {
    z1 = p; p += (int64_t)nb * h1;
    a1 = p; p += (int64_t)nb * h1;
    z2 = p; p += (int64_t)nb * h2;
    a2 = p; p += (int64_t)nb * h2;
    mean1 = p; p += h1;
    rstd1 = p; p += h1;
    mean2 = p; p += h2;
    rstd2 = p; p += h2;
    sgn = p;
  }
};

__global__ void __launch_bounds__(CT_THREADS) cls_head_train_fwd_kernel(
    const float* g, int nb, int c, int h1, int h2, int out, ptv3_cls_head_params p, const float* __restrict__ mask1,
    const float* __restrict__ mask2, float inv_keep, const float* __restrict__ target, float loss_weight,
    float metric_scale, float* save, float* logits, float* __restrict__ stats) {
  __shared__ float xs[CH_RT * CH_MAX_C];
  const ClsSave sv(save, nb, h1, h2, out);
  train_linear(g, nb, c, p.w1, p.b1, h1, sv.z1, xs);
  train_bn_relu_mask(sv.z1, nb, h1, p.bn1_weight, p.bn1_bias, p.bn1_running_mean, p.bn1_running_var, p.bn1_momentum,
                     p.bn1_eps, mask1, inv_keep, sv.a1, sv.mean1, sv.rstd1);
  train_linear(sv.a1, nb, h1, p.w2, p.b2, h2, sv.z2, xs);
  train_bn_relu_mask(sv.z2, nb, h2, p.bn2_weight, p.bn2_bias, p.bn2_running_mean, p.bn2_running_var, p.bn2_momentum,
                     p.bn2_eps, mask2, inv_keep, sv.a2, sv.mean2, sv.rstd2);
  train_linear(sv.a2, nb, h2, p.w3, p.b3, out, logits, xs);
  if (!target) {   // no signs to tape: zeros, so that a backward asked to form dlogits from them reads no stale memory
    for (int i = threadIdx.x; i < nb * out; i += CT_THREADS) sv.sgn[i] = 0.f;
    return;
  }
  // a thread owns whole columns of the logits too
  for (int o = threadIdx.x; o < out; o += CT_THREADS) {
    float cs = 0.f;
    for (int r = 0; r < nb; ++r) {
      const int64_t i = (int64_t)r * out + o;
      const float d = logits[i] - target[i];
      cs += fabsf(d);
      sv.sgn[i] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // sign(0) = 0 (and NaN -> 0 gradient is not torch's; a NaN
                                                            // loss has no meaningful gradient either way)
    }
    xs[o] = cs;
  }
  __syncthreads();
  write_stats(xs, nb, out, loss_weight, metric_scale, stats);
}

// y (nb, K) = x (nb, O) w, w (O, K) as nn.Linear stores it (lanes along K: coalesced), rows in tiles; `a` given: the
// ReLU / keep-mask backward on the way out (a > 0 exactly where the unit was kept and positive).  Ends with a barrier.
__device__ __forceinline__ void back_linear(const float* x, int nb, int O, const float* __restrict__ w, int K,
                                            const float* a, float inv_keep, float* y, float* xs) {
  for (int t0 = 0; t0 < nb; t0 += CH_RT) {
    const int rows = nb - t0 < CH_RT ? nb - t0 : CH_RT;
    stage_rows<CT_THREADS, CH_MAX_C>(x, O, t0, rows, xs);
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += CT_THREADS) {
      float acc[CH_RT];
      dot_wt<CH_MAX_C, 8>(xs, O, w, K, k, acc);
#pragma unroll
      for (int r = 0; r < CH_RT; ++r)
        if (r < rows) {
          const int64_t i = (int64_t)(t0 + r) * K + k;
          y[i] = a ? (a[i] > 0.f ? acc[r] * inv_keep : 0.f) : acc[r];
        }
    }
    __syncthreads();
  }
}

// dy (in place) -> dz through the batch-statistic BatchNorm; dgamma, dbeta, and the bias gradient of the Linear in front
__device__ __forceinline__ void back_bn(float* dy, const float* __restrict__ z, int nb, int H,
                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                        const float* __restrict__ gamma, float* dgamma, float* dbeta, float* dbias) {
  for (int o = threadIdx.x; o < H; o += CT_THREADS) {
    const float mu = mean[o], rs = rstd[o];
    float sb = 0.f, sg = 0.f;
#pragma unroll 4
    for (int r = 0; r < nb; ++r) {
      const int64_t i = (int64_t)r * H + o;
      const float d = dy[i];
      sb += d;
      sg = fmaf(d, (z[i] - mu) * rs, sg);
    }
    dbeta[o] = sb;
    dgamma[o] = sg;
    const float ca = gamma[o] * rs, k1 = sb / (float)nb, k2 = sg / (float)nb;
    float db = 0.f;
#pragma unroll 4
    for (int r = 0; r < nb; ++r) {
      const int64_t i = (int64_t)r * H + o;
      const float v = ca * (dy[i] - k1 - (z[i] - mu) * rs * k2);
      dy[i] = v;
      db += v;
    }
    dbias[o] = db;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(CT_THREADS) cls_head_train_bwd_kernel(
    int nb, int c, int h1, int h2, int out, ptv3_cls_head_params p, const float* __restrict__ dlogits,
    const float* __restrict__ dloss, float loss_weight, float inv_keep, float* save, float* dz, float* dg,
    ptv3_cls_head_grads gr) {
  __shared__ float xs[CH_RT * CH_MAX_C];
  const ClsSave sv(save, nb, h1, h2, out);
  float* dz1 = dz;
  float* dz2 = dz1 + (int64_t)nb * h1;
  float* dz3 = dz2 + (int64_t)nb * h2;
  const float coef = dlogits ? 0.f : (dloss[0] * loss_weight) / ((float)nb * (float)out);
  for (int o = threadIdx.x; o < out; o += CT_THREADS) {
    float db = 0.f;
    for (int r = 0; r < nb; ++r) {
      const int64_t i = (int64_t)r * out + o;
      const float v = dlogits ? dlogits[i] : coef * sv.sgn[i];
      dz3[i] = v;
      db += v;
    }
    gr.db3[o] = db;
  }
  __syncthreads();
  back_linear(dz3, nb, out, p.w3, h2, sv.a2, inv_keep, dz2, xs);
  back_bn(dz2, sv.z2, nb, h2, sv.mean2, sv.rstd2, p.bn2_weight, gr.dbn2_weight, gr.dbn2_bias, gr.db2);
  back_linear(dz2, nb, h2, p.w2, h1, sv.a1, inv_keep, dz1, xs);
  back_bn(dz1, sv.z1, nb, h1, sv.mean1, sv.rstd1, p.bn1_weight, gr.dbn1_weight, gr.dbn1_bias, gr.db1);
  back_linear(dz1, nb, h1, p.w1, c, nullptr, 1.f, dg, xs);
}

// dW[o][k] = sum_r dz[r][o] x[r][k], r in row order; the three weights share one grid (blocks [0, n1) [n1, n2) [n2, ..))
__global__ void __launch_bounds__(CT_THREADS) cls_head_wgrad_kernel(int nb, int c, int h1, int h2, int out,
                                                                     const float* __restrict__ g,
                                                                     const float* __restrict__ save,
                                                                     const float* __restrict__ dz, int blk1, int blk2,
                                                                     float* __restrict__ dw1, float* __restrict__ dw2,
                                                                     float* __restrict__ dw3) {
  const ClsSave sv(const_cast<float*>(save), nb, h1, h2, out);
  int blk = blockIdx.x;
  const float *x, *d;
  float* dw;
  int O, K;
  if (blk < blk1) {
    x = g; d = dz; dw = dw1; O = h1; K = c;
  } else if (blk < blk1 + blk2) {
    blk -= blk1; x = sv.a1; d = dz + (int64_t)nb * h1; dw = dw2; O = h2; K = h1;
  } else {
    blk -= blk1 + blk2; x = sv.a2; d = dz + (int64_t)nb * (h1 + h2); dw = dw3; O = out; K = h2;
  }
  const int64_t e = (int64_t)blk * CT_THREADS + threadIdx.x;
  if (e >= (int64_t)O * K) return;
  const int o = (int)(e / K), k = (int)(e - (int64_t)o * K);
  float acc = 0.f;
  int r = 0;
  for (; r + 4 <= nb; r += 4) {
    float dv[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dv[u] = d[(int64_t)(r + u) * O + o];
      xv[u] = x[(int64_t)(r + u) * K + k];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = fmaf(dv[u], xv[u], acc);
  }
  for (; r < nb; ++r) acc = fmaf(d[(int64_t)r * O + o], x[(int64_t)r * K + k], acc);
  dw[e] = acc;
}

static bool ch_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int cls_head_dims_check(const char* who, int c, int h1, int h2, int out) {
  if (!(c >= 8 && c <= CH_MAX_C && c % 8 == 0)) {
    set_error("%s: c=%d unsupported (multiple of 8 in [8, %d])", who, c, CH_MAX_C);
    return PTV3_ERR_UNSUPPORTED;
  }
  if (!(h1 >= 1 && h1 <= CH_MAX_H && h2 >= 1 && h2 <= CH_MAX_H && out >= 1 && out <= CH_MAX_H)) {
    set_error("%s: widths %d / %d / %d unsupported (each in [1, %d])", who, h1, h2, out, CH_MAX_H);
    return PTV3_ERR_UNSUPPORTED;
  }
  return PTV3_OK;
}

static int cls_head_params_check(const char* who, const ptv3_cls_head_params* p, bool train) {
  PTV3_REQUIRE(p, "%s: params is NULL", who);
  PTV3_REQUIRE(p->w1 && p->b1 && p->bn1_weight && p->bn1_bias && p->w2 && p->b2 && p->bn2_weight && p->bn2_bias &&
                   p->w3 && p->b3, "%s: a head parameter is NULL", who);
  PTV3_REQUIRE(!train || (p->bn1_running_mean && p->bn1_running_var && p->bn2_running_mean && p->bn2_running_var),
               "%s: a running statistic is NULL", who);
  return PTV3_OK;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_cls_head_capable(int c, int h1, int h2, int out) {
  return c >= 8 && c <= CH_MAX_C && c % 8 == 0 && h1 >= 1 && h1 <= CH_MAX_H && h2 >= 1 && h2 <= CH_MAX_H && out >= 1 &&
         out <= CH_MAX_H;
}

extern "C" int ptv3_cls_head_eval(const void* feat, const int64_t* offset, int64_t n, int c, int b, int dtype,
                                  const float* w1t, const float* b1, const float* s1, const float* t1, int h1,
                                  const float* w2t, const float* b2, const float* s2, const float* t2, int h2,
                                  const float* w3t, const float* b3, int out, const float* target, float loss_weight,
                                  float metric_scale, float* logits, float* stats, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  int rc = cls_head_dims_check("cls_head_eval", c, h1, h2, out);
  if (rc != PTV3_OK) return rc;
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "cls_head_eval: dtype %d (0 = fp32, 1 = bf16)", dtype);
  PTV3_REQUIRE(n >= 0 && b >= 0, "cls_head_eval: bad shape n=%lld b=%d", (long long)n, b);
  PTV3_REQUIRE(b == 0 || offset, "cls_head_eval: offset is NULL");
  PTV3_REQUIRE(n == 0 || (feat && ch_aligned16(feat)), "cls_head_eval: feat must be 16-byte aligned");
  PTV3_REQUIRE(b == 0 || (workspace && ch_aligned16(workspace)), "cls_head_eval: workspace must be 16-byte aligned");
  PTV3_REQUIRE(workspace_bytes >= ptv3_scene_mean_workspace_bytes(n, c, b), "cls_head_eval: workspace too small");
  PTV3_REQUIRE(w1t && b1 && s1 && t1 && w2t && b2 && s2 && t2 && w3t && b3, "cls_head_eval: a head parameter is NULL");
  PTV3_REQUIRE(b == 0 || logits, "cls_head_eval: logits is NULL");
  PTV3_REQUIRE(!target || stats, "cls_head_eval: target without stats");
  if (b == 0) return PTV3_OK;
  hipStream_t s = (hipStream_t)stream;
  scene_mean_partial(feat, offset, n, c, b, dtype, (float*)workspace, s);
  hipLaunchKernelGGL(cls_head_eval_kernel, dim3(1), dim3(CE_THREADS), 0, s, (const float*)workspace, offset, n, c,
                     scene_rows_per_chunk(n), b, w1t, b1, s1, t1, h1, w2t, b2, s2, t2, h2, w3t, b3, out, target,
                     loss_weight, metric_scale, logits, stats);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" size_t ptv3_cls_head_save_floats(int b, int h1, int h2, int out) {
  if (b < 0 || h1 < 0 || h2 < 0 || out < 0) return 0;
  return (size_t)2 * b * ((size_t)h1 + h2) + 2 * ((size_t)h1 + h2) + (size_t)b * out;
}

extern "C" int ptv3_cls_head_train_fwd(const float* g, int b, int c, int h1, int h2, int out,
                                       const ptv3_cls_head_params* params, const float* mask1, const float* mask2,
                                       float inv_keep, const float* target, float loss_weight, float metric_scale,
                                       float* save, float* logits, float* stats, void* stream) {
  int rc = cls_head_dims_check("cls_head_train_fwd", c, h1, h2, out);
  if (rc != PTV3_OK) return rc;
  rc = cls_head_params_check("cls_head_train_fwd", params, true);
  if (rc != PTV3_OK) return rc;
  if (b < 2) {
    set_error("cls_head_train_fwd: b=%d unsupported (batch statistics need at least 2 rows)", b);
    return PTV3_ERR_UNSUPPORTED;
  }
  PTV3_REQUIRE(g && mask1 && mask2 && save && logits, "cls_head_train_fwd: a buffer is NULL");
  PTV3_REQUIRE(!target || stats, "cls_head_train_fwd: target without stats");
  hipLaunchKernelGGL(cls_head_train_fwd_kernel, dim3(1), dim3(CT_THREADS), 0, (hipStream_t)stream, g, b, c, h1, h2, out,
                     *params, mask1, mask2, inv_keep, target, loss_weight, metric_scale, save, logits, stats);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cls_head_train_bwd(const float* g, int b, int c, int h1, int h2, int out,
                                       const ptv3_cls_head_params* params, const float* dlogits, const float* dloss,
                                       float loss_weight, float inv_keep, float* save, float* dz, float* dg,
                                       const ptv3_cls_head_grads* grads, void* stream) {
  int rc = cls_head_dims_check("cls_head_train_bwd", c, h1, h2, out);
  if (rc != PTV3_OK) return rc;
  rc = cls_head_params_check("cls_head_train_bwd", params, false);
  if (rc != PTV3_OK) return rc;
  if (b < 2) {
    set_error("cls_head_train_bwd: b=%d unsupported (batch statistics need at least 2 rows)", b);
    return PTV3_ERR_UNSUPPORTED;
  }
  PTV3_REQUIRE(g && save && dz && dg && grads, "cls_head_train_bwd: a buffer is NULL");
  PTV3_REQUIRE((dlogits != nullptr) != (dloss != nullptr), "cls_head_train_bwd: give dlogits or dloss, not both");
  PTV3_REQUIRE(grads->dw1 && grads->db1 && grads->dbn1_weight && grads->dbn1_bias && grads->dw2 && grads->db2 &&
                   grads->dbn2_weight && grads->dbn2_bias && grads->dw3 && grads->db3,
               "cls_head_train_bwd: a gradient buffer is NULL");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cls_head_train_bwd_kernel, dim3(1), dim3(CT_THREADS), 0, s, b, c, h1, h2, out, *params, dlogits,
                     dloss, loss_weight, inv_keep, save, dz, dg, *grads);
  const int blk1 = (int)cdiv((int64_t)h1 * c, CT_THREADS), blk2 = (int)cdiv((int64_t)h2 * h1, CT_THREADS),
            blk3 = (int)cdiv((int64_t)out * h2, CT_THREADS);
  hipLaunchKernelGGL(cls_head_wgrad_kernel, dim3((unsigned)(blk1 + blk2 + blk3)), dim3(CT_THREADS), 0, s, b, c, h1, h2,
                     out, g, (const float*)save, (const float*)dz, blk1, blk2, grads->dw1, grads->dw2, grads->dw3);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
