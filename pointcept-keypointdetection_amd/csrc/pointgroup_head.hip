// PointGroup's two heads and its bias losses as single launches.
//   ptv3_pg_head_eval      point_group_v1m1_base.py:66-67 and :101-117 (eval): both heads, softmax, argmax, the shifted
//                          centre in voxel units and the keep flag of segment_ignore_index
//   ptv3_pg_bias_loss_fwd  :75-89, the masked L1 and negative-cosine losses of the predicted shift
//   ptv3_pg_bias_loss_bwd  autograd of the above with respect to bias_pred
// fp32, no atomics, bitwise repeatable.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace {

constexpr int HE_T = 256;   // threads of a head workgroup
constexpr int HE_R = 8;     // rows per tile: with C = 96 and 256 classes the weights and one tile fill 151 KB of LDS
constexpr int HE_MAX_CLASSES = 256;
constexpr int HE_MAX_IGNORE = 8;

struct IgnoreList { int n; int v[HE_MAX_IGNORE]; };

// LDS (floats): w1t (C x C, [k][j]) | wst (C x K, [k][o]) | w2t (C x 3) | bn scale, bn shift, b1, (C each) |
// bs (K) | feat tile (R x C) | hidden tile (R x C) | logit tile (R x K).  Transposed weights: neighbouring threads read
// neighbouring banks; a tile's rows are read as broadcasts.
__host__ __device__ inline size_t he_lds_floats(int c, int k) {
  return (size_t)c * c + (size_t)c * k + 3 * (size_t)c + 3 * (size_t)c + (size_t)k + 2 * (size_t)HE_R * c +
         (size_t)HE_R * k;
}

__global__ void __launch_bounds__(HE_T)
pg_head_eval_kernel(const float* __restrict__ feat, const float* __restrict__ coord, int64_t n, int c, int k,
                    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ bn_w,
                    const float* __restrict__ bn_b, const float* __restrict__ bn_mean, const float* __restrict__ bn_var,
                    float bn_eps, const float* __restrict__ w2, const float* __restrict__ b2,
                    const float* __restrict__ ws, const float* __restrict__ bs, float voxel_size, IgnoreList ignore,
                    float* __restrict__ bias_pred, float* __restrict__ logit, float* __restrict__ prob,
                    int64_t* __restrict__ segment_pred, float* __restrict__ center, uint8_t* __restrict__ keep) {
  extern __shared__ float lds[];
  float* w1t = lds;
  float* wst = w1t + c * c;
  float* w2t = wst + c * k;
  float* sc = w2t + 3 * c;
  float* sh = sc + c;
  float* sb1 = sh + c;
  float* sbs = sb1 + c;
  float* xf = sbs + k;
  float* xh = xf + HE_R * c;
  float* xl = xh + HE_R * c;
  const int t = threadIdx.x;
  // the weights, once per workgroup
  for (int e = t; e < c * c; e += HE_T) w1t[(e % c) * c + e / c] = w1[e];       // w1[j][kk] -> [kk][j]
  for (int e = t; e < k * c; e += HE_T) wst[(e % c) * k + e / c] = ws[e];       // ws[o][kk] -> [kk][o]
  for (int e = t; e < 3 * c; e += HE_T) w2t[(e % c) * 3 + e / c] = w2[e];       // w2[a][kk] -> [kk][a]
  for (int e = t; e < c; e += HE_T) {
    const float s = bn_w[e] / sqrtf(bn_var[e] + bn_eps);
    sc[e] = s;
    sh[e] = bn_b[e] - bn_mean[e] * s;
    sb1[e] = b1[e];
  }
  for (int e = t; e < k; e += HE_T) sbs[e] = bs[e];
  __syncthreads();
  const int64_t tiles = (n + HE_R - 1) / HE_R;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * HE_R;
    const int rows = (int)min((int64_t)HE_R, n - row0);
    for (int e = t; e < HE_R * c; e += HE_T) xf[e] = e < rows * c ? feat[row0 * c + e] : 0.f;
    __syncthreads();
    // hidden = relu(bn(feat W1^T + b1))
    for (int e = t; e < HE_R * c; e += HE_T) {
      const int r = e / c, j = e % c;
      float acc = sb1[j];
      for (int kk = 0; kk < c; ++kk) acc = fmaf(xf[r * c + kk], w1t[kk * c + j], acc);
      xh[e] = fmaxf(fmaf(acc, sc[j], sh[j]), 0.f);
    }
    __syncthreads();
    // logits (K per row) and the shift (3 per row)
    for (int e = t; e < HE_R * (k + 3); e += HE_T) {
      const int r = e / (k + 3), o = e % (k + 3);
      if (o < k) {
        float acc = sbs[o];
        for (int kk = 0; kk < c; ++kk) acc = fmaf(xf[r * c + kk], wst[kk * k + o], acc);
        xl[r * k + o] = acc;
        if (r < rows) logit[(row0 + r) * k + o] = acc;
      } else if (r < rows) {
        const int a = o - k;
        float acc = b2[a];
        for (int kk = 0; kk < c; ++kk) acc = fmaf(xh[r * c + kk], w2t[kk * 3 + a], acc);
        const int64_t at = (row0 + r) * 3 + a;
        bias_pred[at] = acc;
        center[at] = (coord[at] + acc) / voxel_size;    // one rounding per operation, as torch's add and div
      }
    }
    __syncthreads();
    // softmax and argmax: 32 lanes per row
    {
      const int r = t / 32, lane = t % 32;
      float best = -INFINITY;
      int arg = 0;
      for (int o = lane; o < k; o += 32) {
        const float v = xl[r * k + o];
        if (v > best) { best = v; arg = o; }
      }
      for (int d = 16; d > 0; d >>= 1) {
        const float ob = __shfl_xor(best, d, 32);
        const int oa = __shfl_xor(arg, d, 32);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
      }
      float sum = 0.f;
      for (int o = lane; o < k; o += 32) sum += expf(xl[r * k + o] - best);
      for (int d = 16; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 32);
      if (r < rows) {
        for (int o = lane; o < k; o += 32) prob[(row0 + r) * k + o] = expf(xl[r * k + o] - best) / sum;
        if (lane == 0) {
          bool kept = true;
          for (int q = 0; q < ignore.n; ++q) kept = kept && arg != ignore.v[q];
          segment_pred[row0 + r] = arg;
          keep[row0 + r] = kept ? 1 : 0;
        }
      }
    }
    __syncthreads();
  }
}

// ---- bias losses ---------------------------------------------------------------------------------------------------
constexpr int BL_T = 1024;
constexpr float BL_EPS = 1e-8f;

// one workgroup: thread t adds rows t, t + 1024, ... in that order (stage 1), then a fixed tree over the 1024 sums
__global__ void __launch_bounds__(BL_T)
pg_bias_loss_fwd_kernel(const float* __restrict__ bias_pred, const float* __restrict__ coord,
                        const float* __restrict__ centroid, const int64_t* __restrict__ instance, int64_t ignore_index,
                        int64_t n, float* __restrict__ out) {
  __shared__ double s_l1[BL_T], s_cos[BL_T], s_m[BL_T];
  const int t = threadIdx.x;
  double l1 = 0.0, cs = 0.0, m = 0.0;
  for (int64_t i = t; i < n; i += BL_T) {
    if (instance[i] == ignore_index) continue;
    float p[3], g[3];
    for (int a = 0; a < 3; ++a) { p[a] = bias_pred[3 * i + a]; g[a] = centroid[3 * i + a] - coord[3 * i + a]; }
    const float pn = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + BL_EPS;
    const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) + BL_EPS;
    l1 += (double)(fabsf(p[0] - g[0]) + fabsf(p[1] - g[1]) + fabsf(p[2] - g[2]));
    cs -= (double)((p[0] / pn) * (g[0] / gn) + (p[1] / pn) * (g[1] / gn) + (p[2] / pn) * (g[2] / gn));
    m += 1.0;
  }
  s_l1[t] = l1; s_cos[t] = cs; s_m[t] = m;
  __syncthreads();
  for (int o = BL_T / 2; o > 0; o >>= 1) {
    if (t < o) { s_l1[t] += s_l1[t + o]; s_cos[t] += s_cos[t + o]; s_m[t] += s_m[t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    const float denom = (float)s_m[0] + BL_EPS;     // torch.sum(mask) + 1e-8 in fp32
    out[0] = (float)s_l1[0] / denom;
    out[1] = (float)s_cos[0] / denom;
    out[2] = denom;
  }
}

// d bias_pred = mask / denom * (dl1 * sign(p - g) + dcos * d(-u . v) / dp), u = p / (|p| + eps), v = g / (|g| + eps):
// d(-u . v)/dp = -(v / (|p| + eps) - (p . v) p / (|p| (|p| + eps)^2)); at p == 0 the norm's gradient is 0 (torch.norm's
// subgradient), so the second term drops; sign(0) = 0 (torch.abs)
__global__ void pg_bias_loss_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ bias_pred,
                                        const float* __restrict__ coord, const float* __restrict__ centroid,
                                        const int64_t* __restrict__ instance, int64_t ignore_index, int64_t n,
                                        const float* __restrict__ fwd_out, float* __restrict__ dbias) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float d[3] = {0.f, 0.f, 0.f};
  if (instance[i] != ignore_index) {
    const float inv = 1.0f / fwd_out[2], dl1 = dloss[0] * inv, dcs = dloss[1] * inv;
    float p[3], g[3], v[3];
    for (int a = 0; a < 3; ++a) { p[a] = bias_pred[3 * i + a]; g[a] = centroid[3 * i + a] - coord[3 * i + a]; }
    const float pn0 = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), pn = pn0 + BL_EPS;
    const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) + BL_EPS;
    for (int a = 0; a < 3; ++a) v[a] = g[a] / gn;
    const float pv = p[0] * v[0] + p[1] * v[1] + p[2] * v[2];
    const float radial = pn0 > 0.f ? pv / (pn0 * pn * pn) : 0.f;
    for (int a = 0; a < 3; ++a) {
      const float diff = p[a] - g[a];
      const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
      d[a] = dl1 * sgn - dcs * (v[a] / pn - radial * p[a]);
    }
  }
  for (int a = 0; a < 3; ++a) dbias[3 * i + a] = d[a];
}

}  // namespace

extern "C" int ptv3_pg_head_eval_capable(int c, int num_classes) {
  return (c == 64 || c == 96) && num_classes >= 1 && num_classes <= HE_MAX_CLASSES ? 1 : 0;
}

extern "C" int ptv3_pg_head_eval(const float* feat, const float* coord, int64_t n, int c, int num_classes,
                                 const float* w1, const float* b1, const float* bn_weight, const float* bn_bias,
                                 const float* bn_mean, const float* bn_var, float bn_eps, const float* w2,
                                 const float* b2, const float* w_seg, const float* b_seg, float voxel_size,
                                 const int* ignore_host, int num_ignore, float* bias_pred, float* logit, float* prob,
                                 int64_t* segment_pred, float* center, uint8_t* keep, void* stream) {
  PTV3_REQUIRE(ptv3_pg_head_eval_capable(c, num_classes), "ptv3_pg_head_eval: C = %d (64 or 96), %d classes (1 .. %d)", c,
               num_classes, HE_MAX_CLASSES);
  PTV3_REQUIRE(n >= 0 && num_ignore >= 0 && num_ignore <= HE_MAX_IGNORE && (num_ignore == 0 || ignore_host),
               "ptv3_pg_head_eval: n >= 0 and at most %d ignored classes", HE_MAX_IGNORE);
  PTV3_REQUIRE(voxel_size > 0.f, "ptv3_pg_head_eval: voxel_size must be positive");
  if (n == 0) return PTV3_OK;
  PTV3_REQUIRE(feat && coord && w1 && b1 && bn_weight && bn_bias && bn_mean && bn_var && w2 && b2 && w_seg && b_seg &&
               bias_pred && logit && prob && segment_pred && center && keep, "ptv3_pg_head_eval: null pointer");
  IgnoreList ig;
  ig.n = num_ignore;
  for (int q = 0; q < HE_MAX_IGNORE; ++q) ig.v[q] = q < num_ignore ? ignore_host[q] : 0;
  const size_t lds = he_lds_floats(c, num_classes) * sizeof(float);
  ptv3::ensure_dynamic_lds((const void*)pg_head_eval_kernel, (int)lds);
  const int64_t tiles = ptv3::cdiv(n, HE_R);
  const unsigned grid = (unsigned)(tiles < 256 ? tiles : 256);
  pg_head_eval_kernel<<<grid, HE_T, lds, (hipStream_t)stream>>>(feat, coord, n, c, num_classes, w1, b1, bn_weight, bn_bias,
                                                                bn_mean, bn_var, bn_eps, w2, b2, w_seg, b_seg, voxel_size,
                                                                ig, bias_pred, logit, prob, segment_pred, center, keep);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_pg_bias_loss_fwd(const float* bias_pred, const float* coord, const float* centroid,
                                     const int64_t* instance, int64_t ignore_index, int64_t n, float* out, void* stream) {
  PTV3_REQUIRE(n >= 0 && out && (n == 0 || (bias_pred && coord && centroid && instance)),
               "ptv3_pg_bias_loss_fwd: null pointer or negative n");
  pg_bias_loss_fwd_kernel<<<1, BL_T, 0, (hipStream_t)stream>>>(bias_pred, coord, centroid, instance, ignore_index, n, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_pg_bias_loss_bwd(const float* dloss, const float* bias_pred, const float* coord,
                                     const float* centroid, const int64_t* instance, int64_t ignore_index, int64_t n,
                                     const float* fwd_out, float* dbias, void* stream) {
  PTV3_REQUIRE(n >= 0 && (n == 0 || (dloss && bias_pred && coord && centroid && instance && fwd_out && dbias)),
               "ptv3_pg_bias_loss_bwd: null pointer or negative n");
  if (n == 0) return PTV3_OK;
  pg_bias_loss_bwd_kernel<<<dim3((unsigned)ptv3::cdiv(n, 256)), 256, 0, (hipStream_t)stream>>>(
      dloss, bias_pred, coord, centroid, instance, ignore_index, n, fwd_out, dbias);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
