// Eval forward of the Point Transformer V2 grouped vector attention (pointcept/models/point_transformer_v2/
// point_transformer_v2m2_base.py:116-136, pe_bias = True, pe_multiplier = False) as one kernel, fp32, no atomics.
// A workgroup of 256 threads (4 waves) owns a tile of `pt` points = R = pt * ns (point, neighbour) rows, padded to R16
// (a multiple of the 16-row matrix-core tile), and walks them through LDS:
//   0  per row: neighbour j (-1 = missing) and pos = xyz[j] - xyz[i]                            -> POS (R16, 4)
//   A  peb = W_p2 relu(s_p * (W_p1 pos) + t_p) + b_p2 on the matrix core (v_mfma_f32_16x16x4_f32): a wave owns a
//      16-column tile of peb for a set of row tiles; per 16-wide K chunk it reads its W_p2 fragment from global memory
//      once (W_p2 streams, it is never LDS-resident) and computes the A fragment h from POS in registers -> PEB (R16, C)
//   B  u = relu(s_w * (W_w1 (k[j] - q[i] + peb)) + t_w) on the matrix core: a wave owns a row tile and all G columns;
//      the A fragment is formed from PEB, the gathered k row and the q row                      -> U (R16, G)
//   C  logits = W_w2 u + b_w2 (W_w2 in LDS)                                                      -> L (R16, G)
//   D  softmax over the ns rows of a point, per group; THEN the weight of a missing neighbour is zeroed (it took part in
//      the softmax with pos = 0, k = v = 0, as the reference's grouping + mask give it; no renormalisation)
//   E  out[i, ch] = sum_s (v[j_s, ch] + peb[s, ch]) * w[s, ch / I], s ascending
// Every sum has a fixed order that does not depend on `pt`, so results are bitwise reproducible.
// The linear biases in front of a BatchNorm arrive folded into its shift.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int GVA_THREADS = 256;
constexpr int GVA_WAVES = GVA_THREADS / 64;
constexpr int GVA_MAX_TILES = 8;          // row tiles per workgroup: R16 <= 128
constexpr int GVA_MAX_C = 512;
constexpr int GVA_MAX_G = 64;
constexpr int GVA_LDS_LIMIT = 150 * 1024;

struct GvaArgs {
  const float *q, *k, *v, *xyz;
  const int* idx;
  const float *wp1, *sp, *tp, *wp2, *bp2, *ww1, *sw, *tw, *ww2, *bw2;
  float* out;
  int64_t n;
  int c, g, ns, pt;
};

struct GvaLayout {
  int R, R16, ldp, ldu, pos, peb, u, l, w2, floats;
};
__host__ __device__ inline GvaLayout gva_layout(int c, int g, int ns, int pt) {
  GvaLayout y;
  y.R = pt * ns;
  y.R16 = (y.R + 15) & ~15;
  y.ldp = c + 4;      // float4-aligned rows, consecutive rows one 16-byte slot apart in the banks
  y.ldu = g + 1;
  y.pos = 0;
  y.peb = y.pos + y.R16 * 4;
  y.u = y.peb + y.R16 * y.ldp;
  y.l = y.u + y.R16 * y.ldu;
  y.w2 = y.l + y.R16 * y.ldu;
  y.floats = y.w2 + g * (g + 1);
  return y;
}

__device__ __forceinline__ f32x4 gva_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__global__ void __launch_bounds__(GVA_THREADS) gva_kernel(GvaArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gva_smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int c = a.c, G = a.g, ns = a.ns, pt = a.pt, I = c / G;
  const GvaLayout y = gva_layout(c, G, ns, pt);
  const int R = y.R, R16 = y.R16, ldp = y.ldp, ldu = y.ldu;
  float* POS = gva_smem + y.pos;
  float* PEB = gva_smem + y.peb;
  float* U = gva_smem + y.u;
  float* L = gva_smem + y.l;
  float* W2 = gva_smem + y.w2;
  const int64_t i0 = (int64_t)blockIdx.x * pt;
  const int64_t last = a.n - 1;
  const int nrt = R16 >> 4;

  // ---- 0: neighbour and offset per row (rows past R, and points past n, are computed like real ones and never stored)
  for (int r = tid; r < R16; r += GVA_THREADS) {
    const int p = min(r / ns, pt - 1);
    const int64_t i = min(i0 + p, last);
    int j = r < R ? a.idx[i * ns + (r - p * ns)] : -1;
    if (j < 0 || j >= a.n) j = -1;
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (j >= 0) {
      rx = a.xyz[3 * (int64_t)j] - a.xyz[3 * i];
      ry = a.xyz[3 * (int64_t)j + 1] - a.xyz[3 * i + 1];
      rz = a.xyz[3 * (int64_t)j + 2] - a.xyz[3 * i + 2];
    }
    POS[4 * r] = rx;
    POS[4 * r + 1] = ry;
    POS[4 * r + 2] = rz;
    reinterpret_cast<int*>(POS)[4 * r + 3] = j;
  }
  for (int q = tid; q < G * G; q += GVA_THREADS) {
    const int t = q / G;
    W2[t * (G + 1) + (q - t * G)] = a.ww2[q];
  }
  __syncthreads();

  // ---- A: PEB = W_p2 h + b_p2.  item = (column tile, row-tile subset); narrow layers split the rows over the waves
  {
    const int nct = (c + 15) >> 4;
    const int nsplit = nct >= GVA_WAVES ? 1 : (nct >= 2 ? 2 : 4);
    for (int item = wave; item < nct * nsplit; item += GVA_WAVES) {
      const int ct = item % nct, sp = item / nct;
      const int col = 16 * ct + li;
      const bool colok = col < c;
      f32x4 acc[GVA_MAX_TILES];
#pragma unroll
      for (int t = 0; t < GVA_MAX_TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 ps[GVA_MAX_TILES];   // this lane's row of every row tile: does not depend on K
#pragma unroll
      for (int t = 0; t < GVA_MAX_TILES; ++t) {
        const int rt = sp + t * nsplit;
        ps[t] = rt < nrt ? gva_ld4(POS + 4 * (16 * rt + li)) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      for (int k0 = 0; k0 < c; k0 += 16) {
        const int kk = k0 + 4 * lg;     // c is a multiple of 8: this lane's 4 K values are all inside or all outside
        f32x4 b = f32x4{0.f, 0.f, 0.f, 0.f}, s4 = b, t4 = b, w0 = b, w1 = b, w2 = b;
        if (kk < c) {
          if (colok) b = gva_ld4(a.wp2 + (int64_t)col * c + kk);
          s4 = gva_ld4(a.sp + kk);
          t4 = gva_ld4(a.tp + kk);
          w0 = gva_ld4(a.wp1 + 3 * kk);       // rows kk .. kk+3 of W_p1 (C, 3), 12 consecutive floats
          w1 = gva_ld4(a.wp1 + 3 * kk + 4);
          w2 = gva_ld4(a.wp1 + 3 * kk + 8);
        }
#pragma unroll
        for (int t = 0; t < GVA_MAX_TILES; ++t) {
          const int rt = sp + t * nsplit;
          if (rt < nrt) {   // wave-uniform
            f32x4 h;
            h[0] = fmaxf(fmaf(s4[0], fmaf(w0[2], ps[t][2], fmaf(w0[1], ps[t][1], w0[0] * ps[t][0])), t4[0]), 0.f);
            h[1] = fmaxf(fmaf(s4[1], fmaf(w1[1], ps[t][2], fmaf(w1[0], ps[t][1], w0[3] * ps[t][0])), t4[1]), 0.f);
            h[2] = fmaxf(fmaf(s4[2], fmaf(w2[0], ps[t][2], fmaf(w1[3], ps[t][1], w1[2] * ps[t][0])), t4[2]), 0.f);
            h[3] = fmaxf(fmaf(s4[3], fmaf(w2[3], ps[t][2], fmaf(w2[2], ps[t][1], w2[1] * ps[t][0])), t4[3]), 0.f);
            acc[t] = mma16<float>(h, b, acc[t]);
          }
        }
      }
      const float bias = colok ? a.bp2[col] : 0.f;
#pragma unroll
      for (int t = 0; t < GVA_MAX_TILES; ++t) {
        const int rt = sp + t * nsplit;
        if (rt < nrt && colok) {
#pragma unroll
          for (int r = 0; r < 4; ++r) PEB[(16 * rt + 4 * lg + r) * ldp + col] = acc[t][r] + bias;
        }
      }
    }
  }
  __syncthreads();

  // ---- B: U = relu(s_w * (W_w1 (k[j] - q[i] + peb)) + t_w): a wave owns a row tile and every group column
  {
    const int nct = (G + 15) >> 4;    // <= 4
    for (int rt = wave; rt < nrt; rt += GVA_WAVES) {
      const int row = 16 * rt + li;
      const int64_t i = min(i0 + min(row / ns, pt - 1), last);
      const int j = reinterpret_cast<const int*>(POS)[4 * row + 3];
      const float* qrow = a.q + i * c;
      const float* krow = a.k + (int64_t)(j >= 0 ? j : 0) * c;
      const float* prow = PEB + row * ldp;
      f32x4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < c; k0 += 16) {
        const int kk = k0 + 4 * lg;
        const bool kok = kk < c;
        f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kok) {
          const f32x4 kv = j >= 0 ? gva_ld4(krow + kk) : x;
          x = (kv - gva_ld4(qrow + kk)) + gva_ld4(prow + kk);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < nct) {   // wave-uniform
            const int gc = 16 * t + li;
            f32x4 b = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kok && gc < G) b = gva_ld4(a.ww1 + (int64_t)gc * c + kk);
            acc[t] = mma16<float>(x, b, acc[t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int gc = 16 * t + li;
        if (t < nct && gc < G) {
          const float s = a.sw[gc], sh = a.tw[gc];
#pragma unroll
          for (int r = 0; r < 4; ++r) U[(16 * rt + 4 * lg + r) * ldu + gc] = fmaxf(fmaf(acc[t][r], s, sh), 0.f);
        }
      }
    }
  }
  __syncthreads();

  // ---- C: L = W_w2 U + b_w2
  for (int q = tid; q < R * G; q += GVA_THREADS) {
    const int r = q / G, t = q - r * G;
    const float* u = U + r * ldu;
    const float* w = W2 + t * (G + 1);
    float s = a.bw2[t];
    for (int k = 0; k < G; ++k) s = fmaf(w[k], u[k], s);
    L[r * ldu + t] = s;
  }
  __syncthreads();

  // ---- D: softmax over the neighbours, then the mask
  for (int q = tid; q < pt * G; q += GVA_THREADS) {
    const int p = q / G, t = q - p * G;
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
    for (int s = 0; s < ns; ++s) {
      const int j = reinterpret_cast<const int*>(POS)[4 * (p * ns + s) + 3];
      col[s * ldu] = j >= 0 ? col[s * ldu] * inv : 0.f;
    }
  }
  __syncthreads();

  // ---- E: weighted sum of (v + peb) per group
  for (int q = tid; q < pt * c; q += GVA_THREADS) {
    const int p = q / c, ch = q - p * c;
    const int64_t i = i0 + p;
    if (i > last) break;   // q ascends with p
    const int grp = ch / I;
    float o = 0.f;
    for (int s = 0; s < ns; ++s) {
      const int r = p * ns + s;
      const int j = reinterpret_cast<const int*>(POS)[4 * r + 3];
      const float v = j >= 0 ? a.v[(int64_t)j * c + ch] : 0.f;
      o = fmaf(v + PEB[r * ldp + ch], L[r * ldu + grp], o);
    }
    a.out[i * c + ch] = o;
  }
}

}  // namespace ptv3

using namespace ptv3;

// points per workgroup: as many as the LDS budget and the 8 row tiles hold, halved while the grid would leave compute
// units without a workgroup and a full 16-row tile remains
static int gva_points_per_group(int64_t n, int c, int g, int ns) {
  int pt = (16 * GVA_MAX_TILES) / ns;
  pt = pt < 1 ? 1 : pt;
  while (pt > 1 && gva_layout(c, g, ns, pt).floats * (int)sizeof(float) > GVA_LDS_LIMIT) --pt;
  while (pt > 1 && cdiv(n, pt) < 512 && (pt / 2) * ns >= 16) pt /= 2;
  return pt;
}

extern "C" int ptv3_gva_fwd(const float* q, const float* k, const float* v, const float* xyz, const int32_t* idx,
                            int64_t n, int c, int groups, int ns, const float* w_p1, const float* s_p,
                            const float* t_p, const float* w_p2, const float* b_p2, const float* w_w1,
                            const float* s_w, const float* t_w, const float* w_w2, const float* b_w2, float* out,
                            void* stream) {
  PTV3_REQUIRE(c >= 8 && c <= GVA_MAX_C && c % 8 == 0, "gva_fwd: c=%d unsupported (a multiple of 8 in [8, %d])", c,
               GVA_MAX_C);
  PTV3_REQUIRE(groups >= 1 && groups <= GVA_MAX_G && c % groups == 0,
               "gva_fwd: groups=%d unsupported for c=%d (a divisor of c in [1, %d])", groups, c, GVA_MAX_G);
  PTV3_REQUIRE(ns >= 1 && ns <= 32, "gva_fwd: ns=%d unsupported (1 to 32 neighbours)", ns);
  PTV3_REQUIRE(n >= 0 && n <= 0x7fffffff, "gva_fwd: n=%lld outside [0, 2^31)", (long long)n);
  if (n == 0) return PTV3_OK;
  PTV3_REQUIRE(q && k && v && xyz && idx && out, "gva_fwd: a NULL tensor");
  PTV3_REQUIRE(w_p1 && s_p && t_p && w_p2 && b_p2 && w_w1 && s_w && t_w && w_w2 && b_w2, "gva_fwd: a NULL weight");
  const int pt = gva_points_per_group(n, c, groups, ns);
  const GvaLayout y = gva_layout(c, groups, ns, pt);
  const int bytes = y.floats * (int)sizeof(float);
  PTV3_REQUIRE(bytes <= GVA_LDS_LIMIT && y.R16 <= 16 * GVA_MAX_TILES, "gva_fwd: c=%d groups=%d ns=%d does not fit a workgroup",
               c, groups, ns);
  GvaArgs g{q, k, v, xyz, idx, w_p1, s_p, t_p, w_p2, b_p2, w_w1, s_w, t_w, w_w2, b_w2, out, n, c, groups, ns, pt};
  ensure_dynamic_lds((const void*)gva_kernel, bytes);
  hipLaunchKernelGGL(gva_kernel, dim3((unsigned)cdiv(n, pt)), dim3(GVA_THREADS), bytes, (hipStream_t)stream, g);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
