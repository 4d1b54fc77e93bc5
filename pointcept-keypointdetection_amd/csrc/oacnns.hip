// OA-CNNs on gfx950: the kernel-2 / stride-2 sparse convolution pair and the adaptive aggregator of BasicBlock.forward
// (pointcept/models/oacnns/oacnns_v1m1_base.py:87-110, 130-141, 158-164, 184-194).  fp32, no float atomics.
//
// Strided pair.  With kernel 2 and stride 2 a fine site (b, x, y, z) has exactly one coarse parent (b, x>>1, y>>1, z>>1)
// and reaches it through exactly one tap (x&1)*4 + (y&1)*2 + (z&1), so there is no site hash: the parent keys are sorted
// (ptv3_argsort_i64), ranked (ptv3_pool_segments) and a scatter fills the (m_out, 8) child table.
//   down:  out[j] = sum_t W[:, t, :] x[child[j][t]]       one wave = 16 coarse rows x 64 (or 16) output channels, 8 taps of K
//   up:    out[i] = W[:, tap(i), :] y[parent(i)]          rows sorted by tap: a 16-row tile shares ONE weight slice
// Both run on v_mfma_f32_16x16x4_f32 with A (gathered feature rows) and B (weight rows) read straight from global memory
// as 16-byte fragments - K is contiguous in both - and fold BatchNorm + ReLU in the epilogue.
//
// Cluster kernels.  A partition arrives as the sorted order of its cell keys and the run starts (ptv3_pool_segments); the
// cluster COUNT stays on the device: grids are sized by the row count and a workgroup beyond the count returns.  One
// workgroup owns one cluster: its threads form (row lane, 4-channel group), every row lane walks the cluster's rows with
// a fixed stride and the lanes are combined by a fixed tree in LDS, so a result does not depend on scheduling.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int OA_THREADS = 256;
constexpr int OA_MAX_C = 512;

// ------------------------------------------------------------------------------------------------ plan
__global__ void down2_keys_kernel(const int32_t* __restrict__ idx, int64_t n, int sx, int sy, int sz, int64_t none_key,
                                  int64_t* __restrict__ key, int32_t* __restrict__ tap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = idx[4 * i], x = idx[4 * i + 1], y = idx[4 * i + 2], z = idx[4 * i + 3];
  const int px = x >> 1, py = y >> 1, pz = z >> 1;
  const bool ok = x >= 0 && y >= 0 && z >= 0 && px < sx && py < sy && pz < sz;
  key[i] = ok ? (((int64_t)b * sx + px) * sy + py) * sz + pz : none_key;
  tap[i] = (x & 1) * 4 + (y & 1) * 2 + (z & 1);
}

// counts: [0] coarse rows, [1 + t] sites of tap t, [9] sites without a parent (zeroed by the caller; integer atomics)
__global__ void down2_children_kernel(const int32_t* __restrict__ idx, const int64_t* __restrict__ key,
                                      const int32_t* __restrict__ tap, const int64_t* __restrict__ rank,
                                      const int64_t* __restrict__ order, const int32_t* __restrict__ seg_start,
                                      const int32_t* __restrict__ n_out, int64_t n, int64_t none_key,
                                      int32_t* __restrict__ parent, int32_t* __restrict__ child,
                                      int32_t* __restrict__ coarse, int64_t* __restrict__ up_key,
                                      int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0) counts[0] = *n_out - (key[order[n - 1]] == none_key ? 1 : 0);
  if (key[i] == none_key) {
    parent[i] = -1;
    up_key[i] = 8;
    atomicAdd(&counts[9], 1);
    return;
  }
  const int32_t r = (int32_t)rank[i];
  const int t = tap[i];
  parent[i] = r;
  up_key[i] = t;
  child[(int64_t)r * 8 + t] = (int32_t)i;   // sites are unique: one writer per slot
  atomicAdd(&counts[1 + t], 1);
  if (order[seg_start[r]] == i) {           // the run's first member writes the coarse site
    coarse[4 * (int64_t)r] = idx[4 * i];
    coarse[4 * (int64_t)r + 1] = idx[4 * i + 1] >> 1;
    coarse[4 * (int64_t)r + 2] = idx[4 * i + 2] >> 1;
    coarse[4 * (int64_t)r + 3] = idx[4 * i + 3] >> 1;
  }
}

// ------------------------------------------------------------------------------------------------ strided convs
// NT = 16-column tiles per wave: 4 (64 output channels, each gathered row fragment feeds four products) when that still
// gives every SIMD a wave, 1 otherwise (the deep levels have few rows: four times the waves, the rows come from L2)
constexpr int D2_SIMDS = 1024;

// acc[t] += A(16 x cin) * W[col0 + 16t .. +16][0..cin)^T.  Lane (i = l & 15, g = l >> 4) holds A[i][k + 4g ..] and
// W[col i][k + 4g ..] (common.h mma16).  arow: this lane's gathered row, or NULL for a zero row.
template <int NT>
__device__ __forceinline__ void d2_mac(f32x4 (&acc)[NT], const float* arow, const float* __restrict__ w, int64_t ldw,
                                       int cin, int col0, int cout, int i, int g) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if constexpr (NT > 1) {   // one K step per turn: two in flight cost registers here (measured slower: 0.50 against 0.41 ms)
    for (int k0 = 0; k0 < cin; k0 += 16) {
      const int k = k0 + 4 * g;
      const bool kin = k < cin;
      const f32x4 a = (arow && kin) ? *reinterpret_cast<const f32x4*>(arow + k) : zero;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = col0 + 16 * t + i;
        const f32x4 b = (col < cout && kin) ? *reinterpret_cast<const f32x4*>(w + (int64_t)col * ldw + k) : zero;
        acc[t] = mma16<float>(a, b, acc[t]);
      }
    }
    return;
  }
  for (int k0 = 0; k0 < cin; k0 += 32) {   // two K steps per turn: the second step's loads issue ahead of the first products
    const int ka = k0 + 4 * g, kb = ka + 16;
    const bool ina = ka < cin, inb = kb < cin;
    const f32x4 a0 = (arow && ina) ? *reinterpret_cast<const f32x4*>(arow + ka) : zero;
    const f32x4 a1 = (arow && inb) ? *reinterpret_cast<const f32x4*>(arow + kb) : zero;
    f32x4 b0[NT], b1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = col0 + 16 * t + i;
      const float* wr = w + (int64_t)col * ldw;
      b0[t] = (col < cout && ina) ? *reinterpret_cast<const f32x4*>(wr + ka) : zero;
      b1[t] = (col < cout && inb) ? *reinterpret_cast<const f32x4*>(wr + kb) : zero;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mma16<float>(a1, b1[t], mma16<float>(a0, b0[t], acc[t]));
  }
}

__device__ __forceinline__ float d2_epi(float v, const float* scale, const float* shift, int col, int act) {
  if (scale) v = v * scale[col] + shift[col];
  return act == PTV3_ACT_RELU ? fmaxf(v, 0.f) : v;
}

template <int NT>
__global__ void __launch_bounds__(OA_THREADS)
down2_conv_kernel(const float* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ child,
                  int64_t m_out, int cin, int cout, const float* __restrict__ scale, const float* __restrict__ shift,
                  int act, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
  if (row0 >= m_out) return;
  const int col0 = blockIdx.y * (16 * NT);
  const int64_t row = row0 + i;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < 8; ++t) {
    const int c = row < m_out ? child[row * 8 + t] : -1;
    if (__ballot(c >= 0) == 0) continue;   // no row of the tile has this child
    d2_mac<NT>(acc, c >= 0 ? x + (int64_t)c * cin : nullptr, w + (int64_t)t * cin, (int64_t)8 * cin, cin, col0, cout, i, g);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = col0 + 16 * t + i;
    if (col >= cout) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t orow = row0 + 4 * g + r;
      if (orow < m_out) out[orow * cout + col] = d2_epi(acc[t][r], scale, shift, col, act);
    }
  }
}

struct Up2Starts { int s[10]; };   // rows [s[t], s[t+1]) of up_rows use tap t; t = 8: no parent

template <int NT>
__global__ void __launch_bounds__(OA_THREADS)
up2_conv_kernel(const float* __restrict__ y, const float* __restrict__ w, const int32_t* __restrict__ parent,
                const int32_t* __restrict__ up_rows, Up2Starts st, int cin, int cout,
                const float* __restrict__ scale, const float* __restrict__ shift, int act, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  int tile = blockIdx.x * 4 + wave, t = 0;
  for (; t < 9; ++t) {
    const int tiles = (st.s[t + 1] - st.s[t] + 15) >> 4;
    if (tile < tiles) break;
    tile -= tiles;
  }
  if (t == 9) return;
  const int col0 = blockIdx.y * (16 * NT);
  const int p = st.s[t] + tile * 16 + i;
  const int row = p < st.s[t + 1] ? up_rows[p] : -1;
  f32x4 acc[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (t < 8) {
    const int par = row >= 0 ? parent[row] : -1;
    d2_mac<NT>(acc, par >= 0 ? y + (int64_t)par * cin : nullptr, w + (int64_t)t * cin, (int64_t)8 * cin, cin, col0, cout, i, g);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = __shfl(row, 4 * g + r);   // lanes 0..15 hold the tile's 16 rows
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int col = col0 + 16 * u + i;
      if (orow >= 0 && col < cout) out[(int64_t)orow * cout + col] = d2_epi(acc[u][r], scale, shift, col, act);
    }
  }
}

// ------------------------------------------------------------------------------------------------ clusters
__global__ void cluster_keys_kernel(const int32_t* __restrict__ idx, int64_t m, const int32_t* __restrict__ mn, int g,
                                    int64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int64_t b = idx[4 * i];
  const int64_t cx = (idx[4 * i + 1] - mn[0]) / g, cy = (idx[4 * i + 2] - mn[1]) / g, cz = (idx[4 * i + 3] - mn[2]) / g;
  key[i] = (b << 48) | (cx << 32) | (cy << 16) | cz;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// combine the row lanes' partial sums sm[rl * cv + c4] into sm[c4] by a fixed tree
__device__ __forceinline__ void oa_tree(f32x4* sm, int R, int cv, int rl, int c4) {
  int top = 1;
  while (top < R) top <<= 1;
  for (int s = top >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if (rl < s && rl + s < R) sm[rl * cv + c4] += sm[(rl + s) * cv + c4];
  }
  __syncthreads();
}

__global__ void __launch_bounds__(OA_THREADS)
cluster_center_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ order,
                      const int32_t* __restrict__ seg, const int32_t* __restrict__ n_out, int C,
                      float* __restrict__ out) {
  if ((int)blockIdx.x >= *n_out) return;
  __shared__ f32x4 sm[OA_THREADS];
  const int cv = C >> 2, R = OA_THREADS / cv, rl = threadIdx.x / cv, c4 = threadIdx.x - rl * cv;
  const int s = seg[blockIdx.x], e = seg[blockIdx.x + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (rl < R) {
    int p = s + rl;
    for (; p + 3 * R < e; p += 4 * R) {   // four rows in flight, added in row order
      const int64_t r0 = order[p], r1 = order[p + R], r2 = order[p + 2 * R], r3 = order[p + 3 * R];
      const f32x4 a0 = ld4(x + r0 * ldx + 4 * c4), a1 = ld4(x + r1 * ldx + 4 * c4);
      const f32x4 a2 = ld4(x + r2 * ldx + 4 * c4), a3 = ld4(x + r3 * ldx + 4 * c4);
      acc += a0; acc += a1; acc += a2; acc += a3;
    }
    for (; p < e; p += R) acc += ld4(x + order[p] * ldx + 4 * c4);
    sm[rl * cv + c4] = acc;
  }
  oa_tree(sm, R, cv, rl, c4);
  if (rl >= R) return;
  const float cnt = (float)(e - s);
  const f32x4 mean = sm[c4] / cnt;
  for (int p = s + rl; p < e; p += R) {
    const int64_t row = order[p];
    *reinterpret_cast<f32x4*>(out + row * C + 4 * c4) = ld4(x + row * ldx + 4 * c4) - mean;
  }
}

__global__ void __launch_bounds__(OA_THREADS)
cluster_softmax_sum_kernel(const float* __restrict__ pl, int64_t ldp, const float* __restrict__ v, int64_t ldv,
                           const float* __restrict__ gmax, const int64_t* __restrict__ order,
                           const int32_t* __restrict__ seg, const int32_t* __restrict__ n_out, int C,
                           float* __restrict__ agg) {
  if ((int)blockIdx.x >= *n_out) return;
  __shared__ f32x4 sm[2 * OA_THREADS];
  const int cv = C >> 2, R = OA_THREADS / cv, rl = threadIdx.x / cv, c4 = threadIdx.x - rl * cv;
  const int s = seg[blockIdx.x], e = seg[blockIdx.x + 1];
  const float M = *gmax;
  f32x4 se = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
  if (rl < R) {
    auto add = [&](f32x4 a, f32x4 b) {
      const f32x4 ex = {expf(a[0] - M), expf(a[1] - M), expf(a[2] - M), expf(a[3] - M)};
      se += ex;
      sv += b * ex;
    };
    int p = s + rl;
    for (; p + 3 * R < e; p += 4 * R) {   // four rows in flight, added in row order
      const int64_t r0 = order[p], r1 = order[p + R], r2 = order[p + 2 * R], r3 = order[p + 3 * R];
      const f32x4 a0 = ld4(pl + r0 * ldp + 4 * c4), b0 = ld4(v + r0 * ldv + 4 * c4);
      const f32x4 a1 = ld4(pl + r1 * ldp + 4 * c4), b1 = ld4(v + r1 * ldv + 4 * c4);
      const f32x4 a2 = ld4(pl + r2 * ldp + 4 * c4), b2 = ld4(v + r2 * ldv + 4 * c4);
      const f32x4 a3 = ld4(pl + r3 * ldp + 4 * c4), b3 = ld4(v + r3 * ldv + 4 * c4);
      add(a0, b0); add(a1, b1); add(a2, b2); add(a3, b3);
    }
    for (; p < e; p += R) {
      const int64_t row = order[p];
      add(ld4(pl + row * ldp + 4 * c4), ld4(v + row * ldv + 4 * c4));
    }
    sm[rl * cv + c4] = se;
    sm[OA_THREADS + rl * cv + c4] = sv;
  }
  {  // both accumulators through the same fixed tree
    int top = 1;
    while (top < R) top <<= 1;
    for (int st = top >> 1; st > 0; st >>= 1) {
      __syncthreads();
      if (rl < st && rl + st < R) {
        sm[rl * cv + c4] += sm[(rl + st) * cv + c4];
        sm[OA_THREADS + rl * cv + c4] += sm[OA_THREADS + (rl + st) * cv + c4];
      }
    }
    __syncthreads();
  }
  if (rl == 0)
    *reinterpret_cast<f32x4*>(agg + (int64_t)blockIdx.x * C + 4 * c4) = sm[OA_THREADS + c4] / (sm[c4] + 1e-6f);
}

struct MixArgs {
  const float* agg[4];
  const int64_t* cluster[4];
  const float* logits;
  const float* head;
  float* out;
  int64_t m, ldl, ldh, ldo;
  int C, L, ocol;
};

__global__ void __launch_bounds__(OA_THREADS) cluster_mix_kernel(MixArgs a) {
  const int cv = a.C >> 2;
  const int64_t q = (int64_t)blockIdx.x * OA_THREADS + threadIdx.x;
  const int64_t row = q / cv;
  if (row >= a.m) return;
  const int c4 = (int)(q - row * cv);
  float wgt[4];
  float mx = a.logits[row * a.ldl];
  for (int l = 1; l < a.L; ++l) mx = fmaxf(mx, a.logits[row * a.ldl + l]);
  float sum = 0.f;
  for (int l = 0; l < a.L; ++l) {
    wgt[l] = expf(a.logits[row * a.ldl + l] - mx);
    sum += wgt[l];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int l = 0; l < a.L; ++l) acc += (wgt[l] / sum) * ld4(a.agg[l] + a.cluster[l][row] * a.C + 4 * c4);
  *reinterpret_cast<f32x4*>(a.out + row * a.ldo + a.ocol + 4 * c4) = acc;
  if (a.head) *reinterpret_cast<f32x4*>(a.out + row * a.ldo + 4 * c4) = ld4(a.head + row * a.ldh + 4 * c4);
}

__global__ void add_act_kernel(const float* __restrict__ a, const float* __restrict__ b, int act, float* __restrict__ out,
                               int64_t count4) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count4) return;
  f32x4 v = ld4(a + 4 * i) + ld4(b + 4 * i);
  if (act == PTV3_ACT_RELU) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
  *reinterpret_cast<f32x4*>(out + 4 * i) = v;
}

static inline bool oa_c_ok(int c) { return c >= 4 && c <= OA_MAX_C && c % 4 == 0; }

}  // namespace ptv3

using namespace ptv3;

#define OA_ROWS(what, n) PTV3_REQUIRE((n) >= 0 && (n) <= 0x7fffffff, what ": rows=%lld outside [0, 2^31)", (long long)(n))

extern "C" int ptv3_down2_keys(const int32_t* indices, int64_t n, int sx, int sy, int sz, int64_t none_key,
                               int64_t* key, int32_t* tap, void* stream) {
  OA_ROWS("down2_keys", n);
  PTV3_REQUIRE(sx >= 1 && sy >= 1 && sz >= 1 && sx <= 32768 && sy <= 32768 && sz <= 32768,
               "down2_keys: coarse shape (%d, %d, %d) outside [1, 32768]", sx, sy, sz);
  PTV3_REQUIRE(none_key > 0, "down2_keys: none_key must exceed every parent key");
  PTV3_REQUIRE(indices && key && tap, "down2_keys: a NULL tensor");
  if (n == 0) return PTV3_OK;
  hipLaunchKernelGGL(down2_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, indices, n, sx,
                     sy, sz, none_key, key, tap);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_down2_children(const int32_t* indices, const int64_t* key, const int32_t* tap, const int64_t* rank,
                                   const int64_t* order, const int32_t* seg_start, const int32_t* n_out, int64_t n,
                                   int64_t none_key, int32_t* parent, int32_t* child, int32_t* coarse, int64_t* up_key,
                                   int32_t* counts, void* stream) {
  OA_ROWS("down2_children", n);
  PTV3_REQUIRE(indices && key && tap && rank && order && seg_start && n_out && parent && child && coarse && up_key &&
               counts, "down2_children: a NULL tensor");
  if (n == 0) return PTV3_OK;
  hipLaunchKernelGGL(down2_children_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, indices,
                     key, tap, rank, order, seg_start, n_out, n, none_key, parent, child, coarse, up_key, counts);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_down2_conv(const float* x, const float* w, const int32_t* child, int64_t n_in, int64_t m_out,
                               int cin, int cout, const float* bn_scale, const float* bn_shift, int act, float* out,
                               void* stream) {
  OA_ROWS("down2_conv", n_in);
  OA_ROWS("down2_conv", m_out);
  PTV3_REQUIRE(cin >= 4 && cin % 4 == 0, "down2_conv: cin=%d must be a positive multiple of 4", cin);
  PTV3_REQUIRE(cout >= 1, "down2_conv: cout=%d", cout);
  PTV3_REQUIRE(act == PTV3_ACT_NONE || act == PTV3_ACT_RELU, "down2_conv: act=%d (none or ReLU)", act);
  PTV3_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "down2_conv: bn_scale/bn_shift must come together");
  PTV3_REQUIRE(x && w && child && out, "down2_conv: a NULL tensor");
  if (m_out == 0) return PTV3_OK;
  if (cdiv(m_out, 16) * cdiv(cout, 64) >= D2_SIMDS)
    hipLaunchKernelGGL(down2_conv_kernel<4>, dim3((unsigned)cdiv(m_out, 64), (unsigned)cdiv(cout, 64)), dim3(OA_THREADS), 0,
                       (hipStream_t)stream, x, w, child, m_out, cin, cout, bn_scale, bn_shift, act, out);
  else
    hipLaunchKernelGGL(down2_conv_kernel<1>, dim3((unsigned)cdiv(m_out, 64), (unsigned)cdiv(cout, 16)), dim3(OA_THREADS), 0,
                       (hipStream_t)stream, x, w, child, m_out, cin, cout, bn_scale, bn_shift, act, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_up2_conv(const float* y, const float* w, const int32_t* parent, const int32_t* up_rows,
                             const int32_t* tap_start_host, int64_t n, int64_t m_in, int cin, int cout,
                             const float* bn_scale, const float* bn_shift, int act, float* out, void* stream) {
  OA_ROWS("up2_conv", n);
  OA_ROWS("up2_conv", m_in);
  PTV3_REQUIRE(cin >= 4 && cin % 4 == 0, "up2_conv: cin=%d must be a positive multiple of 4", cin);
  PTV3_REQUIRE(cout >= 1, "up2_conv: cout=%d", cout);
  PTV3_REQUIRE(act == PTV3_ACT_NONE || act == PTV3_ACT_RELU, "up2_conv: act=%d (none or ReLU)", act);
  PTV3_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "up2_conv: bn_scale/bn_shift must come together");
  PTV3_REQUIRE(y && w && parent && up_rows && tap_start_host && out, "up2_conv: a NULL tensor");
  Up2Starts st;
  int64_t tiles = 0;
  for (int t = 0; t < 10; ++t) st.s[t] = tap_start_host[t];
  PTV3_REQUIRE(st.s[0] == 0 && st.s[9] == n, "up2_conv: tap_start must run from 0 to n");
  for (int t = 0; t < 9; ++t) {
    PTV3_REQUIRE(st.s[t + 1] >= st.s[t], "up2_conv: tap_start must not decrease");
    tiles += (st.s[t + 1] - st.s[t] + 15) / 16;
  }
  if (n == 0) return PTV3_OK;
  if (tiles * cdiv(cout, 64) >= D2_SIMDS)
    hipLaunchKernelGGL(up2_conv_kernel<4>, dim3((unsigned)cdiv(tiles, 4), (unsigned)cdiv(cout, 64)), dim3(OA_THREADS), 0,
                       (hipStream_t)stream, y, w, parent, up_rows, st, cin, cout, bn_scale, bn_shift, act, out);
  else
    hipLaunchKernelGGL(up2_conv_kernel<1>, dim3((unsigned)cdiv(tiles, 4), (unsigned)cdiv(cout, 16)), dim3(OA_THREADS), 0,
                       (hipStream_t)stream, y, w, parent, up_rows, st, cin, cout, bn_scale, bn_shift, act, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cluster_keys(const int32_t* indices, int64_t m, const int32_t* min_xyz, int g, int64_t* key,
                                 void* stream) {
  OA_ROWS("cluster_keys", m);
  PTV3_REQUIRE(g >= 1 && g <= 128, "cluster_keys: grid size g=%d outside [1, 128]", g);
  PTV3_REQUIRE(indices && min_xyz && key, "cluster_keys: a NULL tensor");
  if (m == 0) return PTV3_OK;
  hipLaunchKernelGGL(cluster_keys_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, indices, m,
                     min_xyz, g, key);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cluster_center(const float* x, int64_t ldx, const int64_t* order, const int32_t* seg_start,
                                   const int32_t* n_clusters, int64_t m, int c, float* out, void* stream) {
  OA_ROWS("cluster_center", m);
  PTV3_REQUIRE(oa_c_ok(c), "cluster_center: C=%d unsupported (a multiple of 4 in [4, %d])", c, OA_MAX_C);
  PTV3_REQUIRE(ldx >= c && ldx % 4 == 0, "cluster_center: row stride %lld (a multiple of 4, at least C)", (long long)ldx);
  PTV3_REQUIRE(x && order && seg_start && n_clusters && out, "cluster_center: a NULL tensor");
  if (m == 0) return PTV3_OK;
  hipLaunchKernelGGL(cluster_center_kernel, dim3((unsigned)m), dim3(OA_THREADS), 0, (hipStream_t)stream, x, ldx, order,
                     seg_start, n_clusters, c, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cluster_softmax_sum(const float* p, int64_t ldp, const float* v, int64_t ldv, const float* global_max,
                                        const int64_t* order, const int32_t* seg_start, const int32_t* n_clusters,
                                        int64_t m, int c, float* agg, void* stream) {
  OA_ROWS("cluster_softmax_sum", m);
  PTV3_REQUIRE(oa_c_ok(c), "cluster_softmax_sum: C=%d unsupported (a multiple of 4 in [4, %d])", c, OA_MAX_C);
  PTV3_REQUIRE(ldp >= c && ldp % 4 == 0 && ldv >= c && ldv % 4 == 0,
               "cluster_softmax_sum: row strides %lld, %lld (multiples of 4, at least C)", (long long)ldp, (long long)ldv);
  PTV3_REQUIRE(p && v && global_max && order && seg_start && n_clusters && agg, "cluster_softmax_sum: a NULL tensor");
  if (m == 0) return PTV3_OK;
  hipLaunchKernelGGL(cluster_softmax_sum_kernel, dim3((unsigned)m), dim3(OA_THREADS), 0, (hipStream_t)stream, p, ldp, v,
                     ldv, global_max, order, seg_start, n_clusters, c, agg);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_cluster_mix(const float* logits, int64_t ldl, const float* const* agg_host,
                                const int64_t* const* cluster_host, int levels, const float* head, int64_t ldh,
                                int64_t m, int c, float* out, int64_t ldo, int out_col, void* stream) {
  OA_ROWS("cluster_mix", m);
  PTV3_REQUIRE(oa_c_ok(c), "cluster_mix: C=%d unsupported (a multiple of 4 in [4, %d])", c, OA_MAX_C);
  PTV3_REQUIRE(levels >= 1 && levels <= 4, "cluster_mix: L=%d aggregates unsupported (1 to 4)", levels);
  PTV3_REQUIRE(ldl >= levels, "cluster_mix: logit row stride %lld < L", (long long)ldl);
  PTV3_REQUIRE(out_col >= 0 && out_col % 4 == 0 && ldo % 4 == 0 && ldo >= out_col + c,
               "cluster_mix: output columns [%d, %d) do not fit a row stride of %lld", out_col, out_col + c, (long long)ldo);
  PTV3_REQUIRE(!head || (ldh >= c && ldh % 4 == 0 && out_col >= c), "cluster_mix: head copy needs ldh >= C and out_col >= C");
  PTV3_REQUIRE(logits && agg_host && cluster_host && out, "cluster_mix: a NULL tensor");
  MixArgs a{};
  for (int l = 0; l < levels; ++l) {
    PTV3_REQUIRE(agg_host[l] && cluster_host[l], "cluster_mix: aggregate %d is NULL", l);
    a.agg[l] = agg_host[l];
    a.cluster[l] = cluster_host[l];
  }
  if (m == 0) return PTV3_OK;
  a.logits = logits; a.head = head; a.out = out;
  a.m = m; a.ldl = ldl; a.ldh = ldh; a.ldo = ldo;
  a.C = c; a.L = levels; a.ocol = out_col;
  hipLaunchKernelGGL(cluster_mix_kernel, dim3((unsigned)cdiv(m * (c >> 2), OA_THREADS)), dim3(OA_THREADS), 0,
                     (hipStream_t)stream, a);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_add_act(const float* a, const float* b, int act, float* out, int64_t count, void* stream) {
  PTV3_REQUIRE(count >= 0 && count % 4 == 0, "add_act: count=%lld must be a non-negative multiple of 4", (long long)count);
  PTV3_REQUIRE(act == PTV3_ACT_NONE || act == PTV3_ACT_RELU, "add_act: act=%d (none or ReLU)", act);
  PTV3_REQUIRE(a && b && out, "add_act: a NULL tensor");
  if (count == 0) return PTV3_OK;
  hipLaunchKernelGGL(add_act_kernel, dim3((unsigned)cdiv(count / 4, 256)), dim3(256), 0, (hipStream_t)stream, a, b, act,
                     out, count / 4);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
