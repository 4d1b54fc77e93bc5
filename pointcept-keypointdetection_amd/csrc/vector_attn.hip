// Eval forward of the Point Transformer V1 vector attention (pointcept/models/point_transformer/
// point_transformer_seg.py:87-120) as one kernel, fp32 on the vector ALU, no atomics.
// A workgroup of 256 threads owns a tile of `pt` points = R = pt * ns (point, neighbour) rows and walks them through LDS:
//   0  per row: neighbour index, h = relu(bn(W_p1 rel))                                  -> H (R, 4)
//   1  a = relu(bn_c(x_k[j] - x_q[i] + p_r)),  p_r = W_p2 h + b_p2                         -> A (R, c)
//   2  u = relu(bn(W_w1 a)): W_w1 (c/8, c) streams through LDS in 64-column tiles          -> U (R, c/8)
//   3  logits = W_w2 u + b_w2                                                              -> L (R, c/8)
//   4  softmax over the ns rows of a point, per channel of L (missing neighbours take part, as in the reference)
//   5  out[i, ch] = sum_s (x_v[j_s, ch] + p_r[s, ch]) * L[s, ch mod c/8]   (p_r recomputed from H: 3 MACs)
// The two matrix products give every thread a 4-row x 1-column register tile (two of them when R * c/8 > 1024) read as
// float4 along K from padded LDS rows; the four K phases accumulate separately and are summed at the end.
// The linear biases in front of a BatchNorm arrive folded into its shift.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int VA_THREADS = 256;
constexpr int VA_KC = 64;            // columns of W_w1 per LDS tile
constexpr int VA_LDW = VA_KC + 4;    // padded tile row: consecutive rows start one 16-byte slot apart
constexpr int VA_MAX_CS = 64;
constexpr int VA_ITEMS = 2;          // register tiles per thread
constexpr int VA_LDS_LIMIT = 150 * 1024;

struct VaArgs {
  const float *xq, *xk, *xv, *xyz;
  const int* idx;
  const float *wp1, *sp, *tp, *wp2, *bp2, *sc, *tc, *ww1, *sw, *tw, *ww2, *bw2;
  float* out;
  int64_t n;
  int c, cs, ns, pt;
};

struct VaLayout {
  int R, lda, ldu, a, u, l, wt, h, floats;
};
__host__ __device__ inline VaLayout va_layout(int c, int cs, int ns, int pt) {
  VaLayout y;
  y.R = pt * ns;
  y.lda = c + 4;
  y.ldu = ((cs + 3) & ~3) + 4;
  y.a = 0;
  y.u = y.a + y.R * y.lda;
  y.l = y.u + y.R * y.ldu;
  y.wt = y.l + y.R * y.ldu;
  y.h = y.wt + VA_MAX_CS * VA_LDW;
  y.floats = y.h + y.R * 4;
  return y;
}

// acc[u][rr] += X[row(u, rr)][k0 .. k0 + 4 * k4n) * WT[t(u)][0 .. 4 * k4n), four K phases kept apart
__device__ __forceinline__ void va_mac(f32x4 (&acc)[VA_ITEMS][4], const float* X, int ldx, int k0, const float* wt,
                                       int k4n, const bool (&live)[VA_ITEMS], const int (&tcol)[VA_ITEMS],
                                       const int (&row)[VA_ITEMS][4]) {
#pragma unroll
  for (int u = 0; u < VA_ITEMS; ++u) {
    if (!live[u]) continue;
    const f32x4* w4 = reinterpret_cast<const f32x4*>(wt + tcol[u] * VA_LDW);
    const f32x4* x0 = reinterpret_cast<const f32x4*>(X + row[u][0] * ldx + k0);
    const f32x4* x1 = reinterpret_cast<const f32x4*>(X + row[u][1] * ldx + k0);
    const f32x4* x2 = reinterpret_cast<const f32x4*>(X + row[u][2] * ldx + k0);
    const f32x4* x3 = reinterpret_cast<const f32x4*>(X + row[u][3] * ldx + k0);
    for (int k = 0; k < k4n; ++k) {
      const f32x4 w = w4[k];
      acc[u][0] += x0[k] * w;
      acc[u][1] += x1[k] * w;
      acc[u][2] += x2[k] * w;
      acc[u][3] += x3[k] * w;
    }
  }
}

__device__ __forceinline__ float va_sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

__global__ void __launch_bounds__(VA_THREADS) vector_attn_kernel(VaArgs g) {
  extern __shared__ __attribute__((aligned(16))) float va_smem[];
  const int tid = threadIdx.x;
  const int c = g.c, cs = g.cs, ns = g.ns, pt = g.pt;
  const VaLayout y = va_layout(c, cs, ns, pt);
  const int R = y.R, lda = y.lda, ldu = y.ldu;
  float* A = va_smem + y.a;
  float* U = va_smem + y.u;
  float* L = va_smem + y.l;
  float* WT = va_smem + y.wt;
  float* H = va_smem + y.h;
  const int64_t i0 = (int64_t)blockIdx.x * pt;
  const int64_t last = g.n - 1;

  // ---- 0: neighbour and positional hidden layer per row; U zeroed (its K padding must read as zero)
  for (int r = tid; r < R; r += VA_THREADS) {
    const int64_t i = min(i0 + r / ns, last);
    int j = g.idx[i * ns + r % ns];
    if (j < 0 || j >= g.n) j = -1;
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (j >= 0) {
      rx = g.xyz[3 * (int64_t)j] - g.xyz[3 * i];
      ry = g.xyz[3 * (int64_t)j + 1] - g.xyz[3 * i + 1];
      rz = g.xyz[3 * (int64_t)j + 2] - g.xyz[3 * i + 2];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float t = g.wp1[3 * a] * rx + g.wp1[3 * a + 1] * ry + g.wp1[3 * a + 2] * rz;
      H[4 * r + a] = fmaxf(t * g.sp[a] + g.tp[a], 0.f);
    }
    reinterpret_cast<int*>(H)[4 * r + 3] = j;
  }
  for (int q = tid; q < R * ldu; q += VA_THREADS) U[q] = 0.f;
  __syncthreads();

  // ---- 1: A = relu(bn_c(x_k[j] - x_q[i] + p_r))
  for (int q = tid; q < R * c; q += VA_THREADS) {
    const int r = q / c, ch = q - r * c;
    const int64_t i = min(i0 + r / ns, last);
    const int j = reinterpret_cast<const int*>(H)[4 * r + 3];
    const float pr = g.wp2[3 * ch] * H[4 * r] + g.wp2[3 * ch + 1] * H[4 * r + 1] + g.wp2[3 * ch + 2] * H[4 * r + 2]
                     + g.bp2[ch];
    const float kv = j >= 0 ? g.xk[(int64_t)j * c + ch] : 0.f;
    const float v = (kv - g.xq[i * c + ch]) + pr;
    A[r * lda + ch] = fmaxf(v * g.sc[ch] + g.tc[ch], 0.f);
  }

  // register tiles: item = (column t, group of 4 rows)
  const int groups = (R + 3) >> 2, items = groups * cs;
  bool live[VA_ITEMS];
  int tcol[VA_ITEMS], row[VA_ITEMS][4], row0[VA_ITEMS];
#pragma unroll
  for (int u = 0; u < VA_ITEMS; ++u) {
    const int q = tid + u * VA_THREADS;
    live[u] = q < items;
    const int grp = live[u] ? q / cs : 0;
    tcol[u] = live[u] ? q - grp * cs : 0;
    row0[u] = 4 * grp;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) row[u][rr] = min(4 * grp + rr, R - 1);
  }
  f32x4 acc[VA_ITEMS][4];

  // ---- 2: U = relu(bn(W_w1 A))
#pragma unroll
  for (int u = 0; u < VA_ITEMS; ++u)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[u][rr] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < c; k0 += VA_KC) {
    const int k4n = min(VA_KC, c - k0) >> 2;
    __syncthreads();   // A complete (first tile) / the previous tile consumed
    for (int v = tid; v < cs * k4n; v += VA_THREADS) {
      const int t = v / k4n, k4 = v - t * k4n;
      *reinterpret_cast<f32x4*>(WT + t * VA_LDW + 4 * k4) =
          *reinterpret_cast<const f32x4*>(g.ww1 + (int64_t)t * c + k0 + 4 * k4);
    }
    __syncthreads();
    va_mac(acc, A, lda, k0, WT, k4n, live, tcol, row);
  }
#pragma unroll
  for (int u = 0; u < VA_ITEMS; ++u) {
    if (!live[u]) continue;
    const float s = g.sw[tcol[u]], t = g.tw[tcol[u]];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      if (row0[u] + rr < R) U[(row0[u] + rr) * ldu + tcol[u]] = fmaxf(va_sum4(acc[u][rr]) * s + t, 0.f);
  }

  // ---- 3: L = W_w2 U + b_w2
  const int cs4 = (cs + 3) & ~3;
  __syncthreads();   // U complete, the last W_w1 tile consumed
  for (int v = tid; v < cs * cs4; v += VA_THREADS) {
    const int t = v / cs4, k = v - t * cs4;
    WT[t * VA_LDW + k] = k < cs ? g.ww2[t * cs + k] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < VA_ITEMS; ++u)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[u][rr] = f32x4{0.f, 0.f, 0.f, 0.f};
  va_mac(acc, U, ldu, 0, WT, cs4 >> 2, live, tcol, row);
#pragma unroll
  for (int u = 0; u < VA_ITEMS; ++u) {
    if (!live[u]) continue;
    const float b = g.bw2[tcol[u]];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      if (row0[u] + rr < R) L[(row0[u] + rr) * ldu + tcol[u]] = va_sum4(acc[u][rr]) + b;
  }
  __syncthreads();

  // ---- 4: softmax over the neighbours
  for (int q = tid; q < pt * cs; q += VA_THREADS) {
    const int p = q / cs, t = q - p * cs;
    float* col = L + p * ns * ldu + t;
    float mx = col[0];
    for (int s = 1; s < ns; ++s) mx = fmaxf(mx, col[s * ldu]);
    float sum = 0.f;
    for (int s = 0; s < ns; ++s) {
      const float e = expf(col[s * ldu] - mx);
      col[s * ldu] = e;
      sum += e;
    }
    const float inv = 1.0f / sum;
    for (int s = 0; s < ns; ++s) col[s * ldu] *= inv;
  }
  __syncthreads();

  // ---- 5: weighted sum of (x_v + p_r) per share group
  for (int q = tid; q < pt * c; q += VA_THREADS) {
    const int p = q / c, ch = q - p * c;
    const int64_t i = i0 + p;
    if (i > last) break;   // q ascends with p
    const int t = ch % cs;
    const float w0 = g.wp2[3 * ch], w1 = g.wp2[3 * ch + 1], w2 = g.wp2[3 * ch + 2], b = g.bp2[ch];
    float o = 0.f;
    for (int s = 0; s < ns; ++s) {
      const int r = p * ns + s;
      const int j = reinterpret_cast<const int*>(H)[4 * r + 3];
      const float pr = w0 * H[4 * r] + w1 * H[4 * r + 1] + w2 * H[4 * r + 2] + b;
      const float v = j >= 0 ? g.xv[(int64_t)j * c + ch] : 0.f;
      o += (v + pr) * L[r * ldu + t];
    }
    g.out[i * c + ch] = o;
  }
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_vector_attn_fwd(const float* x_q, const float* x_k, const float* x_v, const float* xyz,
                                    const int32_t* idx, int64_t n, int c, int ns, const float* w_p1,
                                    const float* s_p, const float* t_p, const float* w_p2, const float* b_p2,
                                    const float* s_c, const float* t_c, const float* w_w1, const float* s_w,
                                    const float* t_w, const float* w_w2, const float* b_w2, float* out, void* stream) {
  PTV3_REQUIRE(c >= 8 && c <= 8 * VA_MAX_CS && c % 8 == 0,
               "vector_attn_fwd: c=%d unsupported (a multiple of 8 in [8, %d]: 8 share groups)", c, 8 * VA_MAX_CS);
  PTV3_REQUIRE(ns >= 1 && ns <= 32, "vector_attn_fwd: ns=%d unsupported (1 to 32 neighbours)", ns);
  PTV3_REQUIRE(n >= 0 && n <= 0x7fffffff, "vector_attn_fwd: n=%lld outside [0, 2^31)", (long long)n);
  if (n == 0) return PTV3_OK;
  PTV3_REQUIRE(x_q && x_k && x_v && xyz && idx && out, "vector_attn_fwd: a NULL tensor");
  PTV3_REQUIRE(w_p1 && s_p && t_p && w_p2 && b_p2 && s_c && t_c && w_w1 && s_w && t_w && w_w2 && b_w2,
               "vector_attn_fwd: a NULL weight");
  const int cs = c / 8;
  // points per workgroup: about 1024 (row, column) outputs of the weight MLP, within the LDS budget
  int pt = 1024 / (ns * cs);
  pt = pt < 1 ? 1 : (pt > 64 ? 64 : pt);
  while (pt > 1 && va_layout(c, cs, ns, pt).floats * (int)sizeof(float) > VA_LDS_LIMIT) --pt;
  const VaLayout y = va_layout(c, cs, ns, pt);
  const int bytes = y.floats * (int)sizeof(float);
  PTV3_REQUIRE(bytes <= VA_LDS_LIMIT && ((y.R + 3) / 4) * cs <= VA_ITEMS * VA_THREADS,
               "vector_attn_fwd: c=%d ns=%d does not fit a workgroup", c, ns);
  VaArgs g{x_q, x_k, x_v, xyz, idx, w_p1, s_p, t_p, w_p2, b_p2, s_c, t_c, w_w1, s_w, t_w, w_w2, b_w2, out, n, c, cs, ns, pt};
  ensure_dynamic_lds((const void*)vector_attn_kernel, bytes);
  hipLaunchKernelGGL(vector_attn_kernel, dim3((unsigned)cdiv(n, pt)), dim3(VA_THREADS), bytes, (hipStream_t)stream, g);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
