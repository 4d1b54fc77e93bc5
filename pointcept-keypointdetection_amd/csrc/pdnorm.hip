// Modulation of every PDBatchNorm of SpUNet-v1m3 in one launch (spconv_unet_v1m3_pdnorm.py:63-74).
// The context is one row and the same for all layers, so all (shift, scale) = Linear_l(SiLU(context)) are one
// matrix-vector product over the concatenated rows of the layers' weights (17.6 MB in the default model): two flops per
// four bytes read, so memory is its limit by arithmetic; the kernel time alone has not been measured (DESIGN.md section
// 28 times calls, which at this size are bound by their launches).
// The weights stay the separate parameters of the state_dict: the kernels reach them through a device table of
// PdnLayer rows (pointers, channel offset, width), a channel finds its layer by a binary search over the offsets.
//   pdnorm_fwd_kernel   a = SiLU(context) staged once per workgroup in LDS.  One wave per output channel: its shift row
//                       and its scale row are read with 16-byte loads along Cc (64 lanes x 4 floats per step; 4-byte
//                       loads where Cc % 4 != 0 or W is not 16-byte aligned), two dot products, a shuffle reduction, and
//                       lane 0 writes gamma (1 + scale), beta (1 + scale) + shift - or, in fold mode, that pair folded
//                       with the running statistics into the (scale, shift) of the conv epilogues.
//   pdnorm_bwd_kernel   the same mapping: a wave writes its channel's two rows of dW = [dshift; dscale] (x) a and keeps
//                       W^T [dshift; dscale] of the channels it walks in registers (16 floats per lane, Cc <= 1024);
//                       the four waves add through LDS in wave order and the workgroup writes one row of `partial`.
//   pdnorm_ctx_kernel   dcontext = SiLU'(context) . sum of the partial rows, in row order.
// No atomics anywhere: every sum has a fixed order, two runs are bitwise equal.  Plain C++.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int PDN_THREADS = 256, PDN_WAVES = 4;
constexpr int PDN_MAX_CC = 1024, PDN_MAX_C = 4096, PDN_MAX_L = 4096;
constexpr int PDN_FWD_GRID = 2048, PDN_BWD_GRID = 512;

// one row of the device table (PTV3_PDNORM_ROW int64 entries, include/ptv3_hip.h)
struct PdnLayer {
  const float *w, *b, *gamma, *beta, *mean, *var;
  int64_t off, c;
};
static_assert(sizeof(PdnLayer) == PTV3_PDNORM_ROW * sizeof(int64_t), "PdnLayer is one row of the table");

__device__ __forceinline__ float pdn_silu(float x) { return x / (1.f + expf(-x)); }

// the last layer whose first channel is not past ch
__device__ __forceinline__ int pdn_layer(const PdnLayer* __restrict__ t, int L, int64_t ch) {
  int lo = 0, hi = L - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].off <= ch) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float pdn_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(PDN_THREADS) void pdnorm_fwd_kernel(const PdnLayer* __restrict__ table, int L, int Cc,
                                                                 int64_t total, const float* __restrict__ context, int fold,
                                                                 float eps, float* __restrict__ out0,
                                                                 float* __restrict__ out1, float* __restrict__ one_plus) {
  __shared__ __attribute__((aligned(16))) float sa[PDN_MAX_CC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < Cc; k += PDN_THREADS) sa[k] = pdn_silu(context[k]);
  __syncthreads();
  for (int64_t ch = (int64_t)blockIdx.x * PDN_WAVES + wave; ch < total; ch += (int64_t)gridDim.x * PDN_WAVES) {
    const PdnLayer ly = table[pdn_layer(table, L, ch)];
    const int64_t c = ch - ly.off;
    const float* ws = ly.w + c * Cc;              // the shift row
    const float* wc = ly.w + (ly.c + c) * Cc;     // the scale row
    float s0 = 0.f, s1 = 0.f;
    if ((Cc & 3) == 0 && ((uintptr_t)ly.w & 15) == 0) {
      for (int k = lane * 4; k < Cc; k += 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(sa + k);
        const f32x4 u = *reinterpret_cast<const f32x4*>(ws + k);
        const f32x4 v = *reinterpret_cast<const f32x4*>(wc + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s0 = fmaf(u[i], a[i], s0);
          s1 = fmaf(v[i], a[i], s1);
        }
      }
    } else {
      for (int k = lane; k < Cc; k += 64) {
        s0 = fmaf(ws[k], sa[k], s0);
        s1 = fmaf(wc[k], sa[k], s1);
      }
    }
    s0 = pdn_wave_sum(s0);
    s1 = pdn_wave_sum(s1);
    if (lane == 0) {
      const float shift = s0 + ly.b[c], op = 1.f + (s1 + ly.b[ly.c + c]);
      const float g = ly.gamma ? ly.gamma[c] : 1.f, be = ly.beta ? ly.beta[c] : 0.f;
      float o0 = g * op, o1 = be * op + shift;
      if (fold) {
        o0 = o0 * (1.f / sqrtf(ly.var[c] + eps));
        o1 = o1 - ly.mean[c] * o0;
      }
      out0[ch] = o0;
      out1[ch] = o1;
      if (one_plus) one_plus[ch] = op;
    }
  }
}

// VEC (Cc % 4 == 0): lane owns k = 256 j + 4 lane + i; otherwise k = 64 j + lane.  Either way acc[e] is one k.
template <bool VEC>
__global__ __launch_bounds__(PDN_THREADS) void pdnorm_bwd_kernel(const PdnLayer* __restrict__ table, int L, int Cc,
                                                                 int64_t total, const float* __restrict__ context,
                                                                 const float* __restrict__ d0, const float* __restrict__ d1,
                                                                 const float* __restrict__ one_plus, float* __restrict__ dW,
                                                                 float* __restrict__ db, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float sa[PDN_MAX_CC];
  __shared__ __attribute__((aligned(16))) float slab[PDN_WAVES][PDN_MAX_CC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < Cc; k += PDN_THREADS) sa[k] = pdn_silu(context[k]);
  __syncthreads();
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int64_t ch = (int64_t)blockIdx.x * PDN_WAVES + wave; ch < total; ch += (int64_t)gridDim.x * PDN_WAVES) {
    const PdnLayer ly = table[pdn_layer(table, L, ch)];
    const int64_t c = ch - ly.off;
    const float g0 = d0[ch], g1 = d1[ch];
    const float dsh = g1;
    const float dsc = g0 * (ly.gamma ? ly.gamma[c] : 1.f) + g1 * (ly.beta ? ly.beta[c] : 0.f);
    if (lane == 0) {
      db[2 * ly.off + c] = dsh;
      db[2 * ly.off + ly.c + c] = dsc;
      const float op = one_plus[ch];
      if (dgamma) dgamma[ch] = g0 * op;
      if (dbeta) dbeta[ch] = g1 * op;
    }
    const float* ws = ly.w + c * Cc;
    const float* wc = ly.w + (ly.c + c) * Cc;
    float* dws = dW + (2 * ly.off + c) * Cc;
    float* dwc = dW + (2 * ly.off + ly.c + c) * Cc;
    if (VEC) {
      const bool aligned = ((uintptr_t)ly.w & 15) == 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = j * 256 + lane * 4;
        if (k < Cc) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(sa + k);
          f32x4 u, v;
          if (aligned) {
            u = *reinterpret_cast<const f32x4*>(ws + k);
            v = *reinterpret_cast<const f32x4*>(wc + k);
          } else {
            u = f32x4{ws[k], ws[k + 1], ws[k + 2], ws[k + 3]};
            v = f32x4{wc[k], wc[k + 1], wc[k + 2], wc[k + 3]};
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[4 * j + i] += fmaf(u[i], dsh, v[i] * dsc);
          *reinterpret_cast<f32x4*>(dws + k) = a * dsh;     // dW is 16-byte aligned (checked on the host)
          *reinterpret_cast<f32x4*>(dwc + k) = a * dsc;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = j * 64 + lane;
        if (k < Cc) {
          acc[j] += fmaf(ws[k], dsh, wc[k] * dsc);
          dws[k] = sa[k] * dsh;
          dwc[k] = sa[k] * dsc;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int k = VEC ? (e >> 2) * 256 + lane * 4 + (e & 3) : e * 64 + lane;
    if (k < Cc) slab[wave][k] = acc[e];
  }
  __syncthreads();
  for (int k = tid; k < Cc; k += PDN_THREADS)
    partial[(int64_t)blockIdx.x * Cc + k] = ((slab[0][k] + slab[1][k]) + slab[2][k]) + slab[3][k];
}

// 64 columns per workgroup; the four waves take rows r = wave, wave + 4, .. and are added in wave order
__global__ __launch_bounds__(PDN_THREADS) void pdnorm_ctx_kernel(const float* __restrict__ partial, int rows, int Cc,
                                                                 const float* __restrict__ context,
                                                                 float* __restrict__ dcontext) {
  __shared__ float red[PDN_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (col < Cc)
    for (int r = wave; r < rows; r += PDN_WAVES) s += partial[(int64_t)r * Cc + col];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && col < Cc) {
    const float sum = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    const float x = context[col];
    const float sig = 1.f / (1.f + expf(-x));
    dcontext[col] = sig * (1.f + x * (1.f - sig)) * sum;
  }
}

static inline int pdn_rows(int64_t total) {
  const int64_t g = cdiv(total, PDN_WAVES);
  return (int)(g < PDN_BWD_GRID ? (g < 1 ? 1 : g) : PDN_BWD_GRID);
}

// the checks shared by both entry points; `total` = sum of the widths
static int pdn_check(const char* who, const void* table, const int32_t* widths, int L, int Cc, const float* context,
                     int64_t* total) {
  PTV3_REQUIRE(L >= 1 && L <= PDN_MAX_L, "%s: L=%d outside [1, %d]", who, L, PDN_MAX_L);
  PTV3_REQUIRE(Cc >= 1 && Cc <= PDN_MAX_CC, "%s: Cc=%d outside [1, %d]", who, Cc, PDN_MAX_CC);
  PTV3_REQUIRE(table && widths && context, "%s: table, widths or context is NULL", who);
  int64_t sum = 0;
  for (int l = 0; l < L; ++l) {
    PTV3_REQUIRE(widths[l] >= 1 && widths[l] <= PDN_MAX_C, "%s: layer %d has width %d outside [1, %d]", who, l,
                 (int)widths[l], PDN_MAX_C);
    sum += widths[l];
  }
  *total = sum;
  return PTV3_OK;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_pdnorm_capable(int C, int Cc) { return C >= 1 && C <= PDN_MAX_C && Cc >= 1 && Cc <= PDN_MAX_CC; }

extern "C" int ptv3_pdnorm_partial_rows(int64_t total) { return pdn_rows(total); }

extern "C" int ptv3_pdnorm_fwd(const int64_t* table_rows, const int32_t* widths, int L, int Cc, const float* context,
                               int fold, int has_stats, float eps, float* out0, float* out1, float* one_plus,
                               void* stream) {
  int64_t total = 0;
  const PdnLayer* table = reinterpret_cast<const PdnLayer*>(table_rows);
  if (int rc = pdn_check("pdnorm_fwd", table, widths, L, Cc, context, &total)) return rc;
  PTV3_REQUIRE(out0 && out1, "pdnorm_fwd: an output is NULL");
  PTV3_REQUIRE(!fold || has_stats, "pdnorm_fwd: fold mode needs the running statistics (has_stats = 0)");
  PTV3_REQUIRE(!fold || (eps >= 0.f && eps == eps), "pdnorm_fwd: eps=%g", (double)eps);
  int64_t grid = cdiv(total, PDN_WAVES);
  if (grid > PDN_FWD_GRID) grid = PDN_FWD_GRID;
  hipLaunchKernelGGL(pdnorm_fwd_kernel, dim3((unsigned)grid), dim3(PDN_THREADS), 0, (hipStream_t)stream, table, L, Cc,
                     total, context, fold ? 1 : 0, eps, out0, out1, one_plus);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_pdnorm_bwd(const int64_t* table_rows, const int32_t* widths, int L, int Cc, const float* context,
                               const float* d_out0, const float* d_out1, const float* one_plus, float* dW, float* db,
                               float* dgamma, float* dbeta, float* partial, float* dcontext, void* stream) {
  int64_t total = 0;
  const PdnLayer* table = reinterpret_cast<const PdnLayer*>(table_rows);
  if (int rc = pdn_check("pdnorm_bwd", table, widths, L, Cc, context, &total)) return rc;
  PTV3_REQUIRE(d_out0 && d_out1 && one_plus, "pdnorm_bwd: an input gradient or one_plus is NULL");
  PTV3_REQUIRE(dW && db && partial && dcontext, "pdnorm_bwd: an output is NULL");
  PTV3_REQUIRE((Cc & 3) != 0 || ((uintptr_t)dW & 15) == 0, "pdnorm_bwd: dW must be 16-byte aligned");
  const int rows = pdn_rows(total);
  hipStream_t st = (hipStream_t)stream;
  if ((Cc & 3) == 0)
    hipLaunchKernelGGL(pdnorm_bwd_kernel<true>, dim3(rows), dim3(PDN_THREADS), 0, st, table, L, Cc, total, context, d_out0,
                       d_out1, one_plus, dW, db, dgamma, dbeta, partial);
  else
    hipLaunchKernelGGL(pdnorm_bwd_kernel<false>, dim3(rows), dim3(PDN_THREADS), 0, st, table, L, Cc, total, context,
                       d_out0, d_out1, one_plus, dW, db, dgamma, dbeta, partial);
  PTV3_LAUNCH_CHECK();
  hipLaunchKernelGGL(pdnorm_ctx_kernel, dim3((unsigned)cdiv(Cc, 64)), dim3(PDN_THREADS), 0, st, partial, rows, Cc, context,
                     dcontext);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
