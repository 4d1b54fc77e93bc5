// Stratified Transformer window attention (ST-v1m2): group plan, fused attention, ball query.
//
// The reference (pointcept/models/stratified_transformer/stratified_transformer_v1m2_refine.py:388-450) expands every
// block's attention into an edge list of M (query, key) pairs and runs five pointops2 kernels and a scatter_softmax over
// it (:158-216).  Every query of one (small window, large window) pair has the same keys - the points of its small
// window and the sampled points of its large window that lie in another small window - so the work is a dense
// [queries x keys] tile per GROUP and the edge list is never needed:
//   r_a(i,j) = trunc((round((x_i - x_j)_a * 1e5) / 1e5 + 2w - 1e-4) / quant)                    a = x, y, z (:163-169)
//   e_ij     = qs_i . k_j + sum_a ( qs_i . Tq[r_a,h,:,a] + k_j . Tk[r_a,h,:,a] ),  qs = scale * q   (:157-204)
//   out_i    = sum_j softmax_j(e_ij) ( v_j + sum_a Tv[r_a,h,:,a] )                                 (:205-216)
// Decomposition as in swin_attn_mfma.hip, one axis at a time, every product on v_mfma_f32_16x16x4_f32 (exact fp32):
//   QT_a[i][r] = qs_i . Tq_a[r]   once per 16-query tile            KT_a[j][r] = k_j . Tk_a[r]   per 16-key chunk
//   e_ij += QT_a[i][r_a] + KT_a[j][r_a]                             two LDS words per pair and axis
//   out_i = sum_j p_ij v_j + sum_a sum_r H_a[i][r] Tv_a[r],         H_a[i][r_a(i,j)] += p_ij
// Keys stream through in chunks of 16 with a running maximum and sum (H_a and the output are rescaled when a row's
// maximum moves), so no bound on a group's keys depends on LDS.  One wave per (group, head); the workgroup is that one
// wave, so lanes hand data over through LDS without barriers.  H_a is a plain read-modify-write: lane (i, a) adds the
// 16 weights of its query to its own row, one after the other - no atomics, fixed order, bitwise reproducible.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int STRAT_MAX_ROWS = 80;   // 4 w / quant of the fork config at every level
constexpr int STRAT_MAXCT = 5;       // 16-row tiles of one axis' table
constexpr int STRAT_D = 16;          // head dimension

__device__ __forceinline__ void strat_lds_fence() { asm volatile("" ::: "memory"); }

// The quantized relative position exactly as torch evaluates WindowAttention.forward's expression in fp32: one rounding
// per operation (no contraction into FMA), correctly rounded divisions, round-half-even.  Clamped to the table.
__device__ __forceinline__ int strat_rel_index(float xi, float xj, float two_w, float quant, int rows) {
#pragma clang fp contract(off)
  const float d = xi - xj;
  const float m = d * 100000.0f;
  const float r = rintf(m);
  const float c = r / 100000.0f;
  const float s = c + two_w;
  const float t = s - 1e-4f;
  const float u = t / quant;
  const int idx = (int)u;
  return min(max(idx, 0), rows - 1);
}

// One window cell coordinate as torch_geometric's voxel_grid computes it: (pos - start) / size in fp32, truncated.
__device__ __forceinline__ int strat_cell(float x, float shift, float start, float size) {
#pragma clang fp contract(off)
  const float p = x + shift;     // shift = 0 in unshifted blocks: x + 0 = x
  const float d = p - start;
  const float c = d / size;
  return (int)c;
}

// key_small = scene << 51 | small cell (3 x 9 bits) << 24 | large cell (3 x 8 bits): groups and small windows are runs
// key_large = scene << 51 | large cell << 27 | small cell:                          groups and large windows are runs
// (in shifted blocks a small window straddles large windows, so neither order serves both)
__global__ void strat_cell_keys_kernel(const float* __restrict__ coord, int64_t n, const int* __restrict__ offset, int b,
                                       const float* __restrict__ cmin, float w, float w2, float shift_s, float shift_l,
                                       int64_t* __restrict__ key_small, int64_t* __restrict__ key_large,
                                       int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = b - 1;        // first scene whose end lies beyond i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (i < offset[mid]) hi = mid; else lo = mid + 1;
  }
  bool oob = false;
  int sc[3], lc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = coord[i * 3 + a], mn = cmin[a];
    sc[a] = strat_cell(x, shift_s, mn, w);
    lc[a] = strat_cell(x, shift_l, mn, w2);
    oob |= sc[a] < 0 || sc[a] >= 512 || lc[a] < 0 || lc[a] >= 256;
  }
  if (oob) {
    *bad = 1;
    key_small[i] = key_large[i] = 0;
    return;
  }
  const int64_t small = ((int64_t)sc[0] << 18) | ((int64_t)sc[1] << 9) | sc[2];
  const int64_t large = ((int64_t)lc[0] << 16) | ((int64_t)lc[1] << 8) | lc[2];
  key_small[i] = ((int64_t)lo << 51) | (small << 24) | large;
  key_large[i] = ((int64_t)lo << 51) | (large << 27) | small;
}

// sampled rows in key_large order: s_rows[sp[p]] = order_l[p] for every sorted position p that holds a sampled point
__global__ void strat_compact_kernel(const int64_t* __restrict__ order_l, const unsigned char* __restrict__ flag,
                                     const int* __restrict__ sp, int64_t n, int* __restrict__ s_rows) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t row = order_l[p];
  if (flag[row]) s_rows[sp[p]] = (int)row;
}

// Where group g finds its keys.  Dense part: its small window, the run [c0, c1) of order_s.  Sparse part: the sampled
// rows of its large window, s_rows[sp[a] .. sp[e]), without those of the group itself, s_rows[sp[c] .. sp[d]), where
// [a, e) is the window's run and [c, d) the group's run in key_large order.
struct StratGroup { int c0, c1, s0, s1, s2, s3; };
__device__ __forceinline__ StratGroup strat_group(int g, const int* __restrict__ q_ptr, const int64_t* __restrict__ order_s,
                                                  const int64_t* __restrict__ cell_of, const int* __restrict__ c_ptr,
                                                  const int64_t* __restrict__ lgroup_of, const int* __restrict__ lg_ptr,
                                                  const int64_t* __restrict__ window_of, const int* __restrict__ w_ptr,
                                                  const int* __restrict__ sp) {
  const int64_t first = order_s[q_ptr[g]];
  const int64_t cell = cell_of[first], lg = lgroup_of[first], wd = window_of[first];
  StratGroup r;
  r.c0 = c_ptr[cell];
  r.c1 = c_ptr[cell + 1];
  r.s0 = sp[w_ptr[wd]];
  r.s1 = sp[lg_ptr[lg]];
  r.s2 = sp[lg_ptr[lg + 1]];
  r.s3 = sp[w_ptr[wd + 1]];
  return r;
}

__global__ void strat_key_count_kernel(const int* __restrict__ q_ptr, const int64_t* __restrict__ order_s,
                                       const int64_t* __restrict__ cell_of, const int* __restrict__ c_ptr,
                                       const int64_t* __restrict__ lgroup_of, const int* __restrict__ lg_ptr,
                                       const int64_t* __restrict__ window_of, const int* __restrict__ w_ptr,
                                       const int* __restrict__ sp, const int* __restrict__ n_groups, int64_t n,
                                       int* __restrict__ count) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  if (g >= *n_groups) { count[g] = 0; return; }
  const StratGroup r = strat_group((int)g, q_ptr, order_s, cell_of, c_ptr, lgroup_of, lg_ptr, window_of, w_ptr, sp);
  count[g] = (r.c1 - r.c0) + (r.s1 - r.s0) + (r.s3 - r.s2);
}

__global__ __launch_bounds__(64) void strat_key_fill_kernel(
    const int* __restrict__ q_ptr, const int64_t* __restrict__ order_s, const int64_t* __restrict__ cell_of,
    const int* __restrict__ c_ptr, const int64_t* __restrict__ lgroup_of, const int* __restrict__ lg_ptr,
    const int64_t* __restrict__ window_of, const int* __restrict__ w_ptr, const int* __restrict__ sp,
    const int* __restrict__ s_rows, const int* __restrict__ k_ptr, int* __restrict__ k_rows) {
  const int g = blockIdx.x;
  const StratGroup r = strat_group(g, q_ptr, order_s, cell_of, c_ptr, lgroup_of, lg_ptr, window_of, w_ptr, sp);
  const int k0 = k_ptr[g], cnt = k_ptr[g + 1] - k0;
  const int dense = r.c1 - r.c0, before = r.s1 - r.s0;
  for (int t = threadIdx.x; t < cnt; t += 64) {
    int row;
    if (t < dense) {
      row = (int)order_s[r.c0 + t];
    } else {
      const int s = t - dense;
      row = s_rows[s < before ? r.s0 + s : r.s2 + (s - before)];
    }
    k_rows[k0 + t] = row;
  }
}

__global__ void strat_rel_index_kernel(const float* __restrict__ coord, const int* __restrict__ qi, const int* __restrict__ kj,
                                       int64_t m, float two_w, float quant, int rows, int* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int64_t i = qi[e], j = kj[e];
#pragma unroll
  for (int a = 0; a < 3; ++a) out[e * 3 + a] = strat_rel_index(coord[i * 3 + a], coord[j * 3 + a], two_w, quant, rows);
}

// q, k, v: rows of `ld` floats, head h at [16 h, 16 h + 16); tables (3, rows, heads, 16) axis-major slabs.
__global__ __launch_bounds__(64) void strat_attn_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t ld,
    const float* __restrict__ coord, const float* __restrict__ tq, const float* __restrict__ tk,
    const float* __restrict__ tv, const int* __restrict__ q_ptr, const int* __restrict__ q_rows,
    const int* __restrict__ k_ptr, const int* __restrict__ k_rows, float* __restrict__ out, int heads, int rows, int TS,
    float scale, float two_w, float quant) {
  constexpr int D = STRAT_D, PS = 20;
  extern __shared__ __align__(16) unsigned char strat_smem[];
  float* sA = reinterpret_cast<float*>(strat_smem);   // [3][16][TS] QT_a of the query tile
  float* sB = sA + 48 * TS;                           // [3][16][TS] KT_a of the key chunk
  float* sH = sB + 48 * TS;                           // [3][16][TS] weight histograms of the query tile
  float* sP = sH + 48 * TS;                           // [16][PS] weights of the chunk
  float* sKc = sP + 16 * PS;                          // [3][16] coordinates of the chunk's keys, axis-major
  int* sKrow = reinterpret_cast<int*>(sKc + 48);      // [16] rows of the chunk's keys
  unsigned char* sIdx = reinterpret_cast<unsigned char*>(sKrow + 16);   // [3][16][16] r_a of the chunk's pairs

  const int grp = blockIdx.x, h = blockIdx.y;
  const int lane = threadIdx.x, li = lane & 15, g = lane >> 4;
  const int q0 = q_ptr[grp], nq = q_ptr[grp + 1] - q0;
  const int k0 = k_ptr[grp], nk = k_ptr[grp + 1] - k0;
  if (nq <= 0 || nk <= 0) return;
  const int nct = (rows + 15) >> 4;
  const size_t hoff = (size_t)h * D, tstride = (size_t)heads * D;

  // the key table's fragments stay in registers for the whole group
  f32x4 tkf[3][STRAT_MAXCT];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int ct = 0; ct < STRAT_MAXCT; ++ct) {
      tkf[a][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ct < nct) {
        const int r = min(16 * ct + li, rows - 1);
        tkf[a][ct] = *reinterpret_cast<const f32x4*>(tk + ((size_t)a * rows + r) * tstride + hoff + 4 * g);
      }
    }

  for (int i0 = 0; i0 < nq; i0 += 16) {
    const int qrow = q_rows[q0 + min(i0 + li, nq - 1)];
    f32x4 qf = *reinterpret_cast<const f32x4*>(q + (size_t)qrow * ld + hoff + 4 * g);
    qf *= scale;
    float xi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) xi[a] = coord[(size_t)qrow * 3 + a];
    // ---- QT_a[i][r]
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int ct = 0; ct < STRAT_MAXCT; ++ct)
        if (ct < nct) {
          const int r = min(16 * ct + li, rows - 1);
          const f32x4 tf = *reinterpret_cast<const f32x4*>(tq + ((size_t)a * rows + r) * tstride + hoff + 4 * g);
          const f32x4 acc = mma16<float>(tf, qf, f32x4{0.f, 0.f, 0.f, 0.f});
          *reinterpret_cast<f32x4*>(sA + (a * 16 + li) * TS + 16 * ct + 4 * g) = acc;
        }
    for (int e = lane * 4; e < 48 * TS; e += 256) *reinterpret_cast<f32x4*>(sH + e) = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 oacc = f32x4{0.f, 0.f, 0.f, 0.f};
    strat_lds_fence();

    for (int kc = 0; kc < nk; kc += 16) {
      const int krow = k_rows[k0 + min(kc + li, nk - 1)];
      if (g == 0) sKrow[li] = krow;
      if (g < 3) sKc[g * 16 + li] = coord[(size_t)krow * 3 + g];
      const f32x4 kf = *reinterpret_cast<const f32x4*>(k + (size_t)krow * ld + hoff + 4 * g);
      // ---- KT_a[j][r]
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int ct = 0; ct < STRAT_MAXCT; ++ct)
          if (ct < nct) {
            const f32x4 acc = mma16<float>(tkf[a][ct], kf, f32x4{0.f, 0.f, 0.f, 0.f});
            *reinterpret_cast<f32x4*>(sB + (a * 16 + li) * TS + 16 * ct + 4 * g) = acc;
          }
      // ---- qs . k: lane (i = li, g) gets the pairs (i, kc + 4 g + e)
      f32x4 ev = mma16<float>(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f});
      strat_lds_fence();
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const f32x4 xj = *reinterpret_cast<const f32x4*>(sKc + a * 16 + 4 * g);
        unsigned pk = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int idx = strat_rel_index(xi[a], xj[e], two_w, quant, rows);
          ev[e] += sA[(a * 16 + li) * TS + idx] + sB[(a * 16 + 4 * g + e) * TS + idx];
          pk |= (unsigned)idx << (8 * e);
        }
        *reinterpret_cast<unsigned*>(sIdx + (a * 16 + li) * 16 + 4 * g) = pk;
      }
      // ---- running softmax of row i = li
      float cmax = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (kc + 4 * g + e >= nk) ev[e] = -INFINITY;
        cmax = fmaxf(cmax, ev[e]);
      }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
      const float m_new = fmaxf(m_run, cmax);          // finite: key 0 of the chunk is never masked
      const float alpha = expf(m_run - m_new);         // first chunk: exp(-inf) = 0
      f32x4 p;
      float psum = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = expf(ev[e] - m_new);
        psum += p[e];
      }
      psum += __shfl_xor(psum, 16);
      psum += __shfl_xor(psum, 32);
      l_run = l_run * alpha + psum;
      m_run = m_new;
      *reinterpret_cast<f32x4*>(sP + li * PS + 4 * g) = p;
      // ---- P V: the accumulator holds out[i = 4 g + e][d = li]
      f32x4 vf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        oacc[e] *= __shfl(alpha, 4 * g + e);
        vf[e] = v[(size_t)sKrow[4 * g + e] * ld + hoff + li];
      }
      oacc = mma16<float>(p, vf, oacc);
      strat_lds_fence();
      // ---- H_a[i][r_a(i,j)] += p_ij: lane (i = li, a = g) owns row i of axis a
      const bool rescale = kc > 0 && __any(alpha != 1.f);
      if (g < 3) {
        float* hrow = sH + (g * 16 + li) * TS;
        if (rescale)
          for (int r = 0; r < 16 * nct; r += 4) {
            f32x4 t = *reinterpret_cast<f32x4*>(hrow + r);
            t *= alpha;
            *reinterpret_cast<f32x4*>(hrow + r) = t;
          }
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
          const unsigned pk = *reinterpret_cast<const unsigned*>(sIdx + (g * 16 + li) * 16 + 4 * j4);
          const f32x4 pj = *reinterpret_cast<const f32x4*>(sP + li * PS + 4 * j4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int idx = (pk >> (8 * e)) & 0xff;
            hrow[idx] += pj[e];
          }
        }
      }
      strat_lds_fence();
    }
    // ---- value table: out_i += sum_a sum_r H_a[i][r] Tv_a[r]; columns r >= rows of H_a are zero
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int kb = 0; kb < STRAT_MAXCT; ++kb)
        if (kb < nct) {
          const f32x4 hf = *reinterpret_cast<const f32x4*>(sH + (a * 16 + li) * TS + 16 * kb + 4 * g);
          f32x4 tf;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = min(16 * kb + 4 * g + e, rows - 1);
            tf[e] = tv[((size_t)a * rows + r) * tstride + hoff + li];
          }
          oacc = mma16<float>(hf, tf, oacc);
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + 4 * g + e;
      const float den = __shfl(l_run, 4 * g + e);
      const int orow = __shfl(qrow, 4 * g + e);
      if (i < nq) out[((size_t)orow * heads + h) * D + li] = oacc[e] / den;
    }
    strat_lds_fence();
  }
}

// partial_dense ball query: thread per query, scan of its own scene in index order
__global__ void ball_query_kernel(const float* __restrict__ xyz, const int* __restrict__ offset, int b, int64_t n, float r2,
                                  int max_neighbor, int64_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = b - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (i < offset[mid]) hi = mid; else lo = mid + 1;
  }
  const int start = lo ? offset[lo - 1] : 0, end = offset[lo];
  const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  int64_t* row = idx + i * max_neighbor;
  int cnt = 0;
  for (int j = start; j < end && cnt < max_neighbor; ++j) {
    const float dx = x - xyz[(size_t)j * 3], dy = y - xyz[(size_t)j * 3 + 1], dz = z - xyz[(size_t)j * 3 + 2];
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < r2) row[cnt++] = j;
  }
  for (; cnt < max_neighbor; ++cnt) row[cnt] = -1;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_strat_attn_capable(int heads, int head_dim, int table_rows) {
  return heads >= 1 && heads <= 65535 && head_dim == STRAT_D && table_rows >= 1 && table_rows <= STRAT_MAX_ROWS;
}

extern "C" int ptv3_strat_cell_keys(const float* coord, int64_t n, const int32_t* offset, int num_scenes,
                                    const float* coord_min, float window, int shifted, int64_t* key_small,
                                    int64_t* key_large, int32_t* bad, void* stream) {
  PTV3_REQUIRE(coord && offset && coord_min && key_small && key_large && bad, "strat_cell_keys: a NULL pointer");
  PTV3_REQUIRE(n >= 1 && n < (1ll << 31), "strat_cell_keys: n=%lld rows (1 .. 2^31 - 1)", (long long)n);
  PTV3_REQUIRE(num_scenes >= 1 && num_scenes <= 4096, "strat_cell_keys: %d scenes (1 .. 4096)", num_scenes);
  PTV3_REQUIRE(window > 0.f, "strat_cell_keys: window %g", (double)window);
  // shift_size = window_size * 1 / 2 of the small and of the doubled window (:374, :382): both exact in fp32
  const float w2 = 2.f * window;
  hipLaunchKernelGGL(strat_cell_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, coord, n,
                     offset, num_scenes, coord_min, window, w2, shifted ? window * 0.5f : 0.f, shifted ? window : 0.f,
                     key_small, key_large, bad);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_strat_key_count(const int32_t* q_ptr, const int64_t* order_s, const int64_t* cell_of,
                                    const int32_t* c_ptr, const int64_t* lgroup_of, const int32_t* lg_ptr,
                                    const int64_t* window_of, const int32_t* w_ptr, const int32_t* sampled_prefix,
                                    const int32_t* n_groups, int64_t n, int32_t* count, void* stream) {
  PTV3_REQUIRE(q_ptr && order_s && cell_of && c_ptr && lgroup_of && lg_ptr && window_of && w_ptr && sampled_prefix &&
                   n_groups && count, "strat_key_count: a NULL pointer");
  PTV3_REQUIRE(n >= 1 && n < (1ll << 31), "strat_key_count: n=%lld rows", (long long)n);
  hipLaunchKernelGGL(strat_key_count_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, q_ptr,
                     order_s, cell_of, c_ptr, lgroup_of, lg_ptr, window_of, w_ptr, sampled_prefix, n_groups, n, count);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_strat_key_fill(const int32_t* q_ptr, const int64_t* order_s, const int64_t* cell_of,
                                   const int32_t* c_ptr, const int64_t* lgroup_of, const int32_t* lg_ptr,
                                   const int64_t* window_of, const int32_t* w_ptr, const int64_t* order_l,
                                   const uint8_t* sampled, const int32_t* sampled_prefix, int64_t n, int64_t n_groups,
                                   const int32_t* k_ptr, int32_t* s_rows, int32_t* k_rows, void* stream) {
  PTV3_REQUIRE(q_ptr && order_s && cell_of && c_ptr && lgroup_of && lg_ptr && window_of && w_ptr && order_l && sampled &&
                   sampled_prefix && k_ptr && s_rows && k_rows, "strat_key_fill: a NULL pointer");
  PTV3_REQUIRE(n >= 1 && n < (1ll << 31) && n_groups >= 1 && n_groups <= n, "strat_key_fill: n=%lld rows, %lld groups",
               (long long)n, (long long)n_groups);
  hipLaunchKernelGGL(strat_compact_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, order_l,
                     sampled, sampled_prefix, n, s_rows);
  PTV3_LAUNCH_CHECK();
  hipLaunchKernelGGL(strat_key_fill_kernel, dim3((unsigned)n_groups), dim3(64), 0, (hipStream_t)stream, q_ptr, order_s,
                     cell_of, c_ptr, lgroup_of, lg_ptr, window_of, w_ptr, sampled_prefix, s_rows, k_ptr, k_rows);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_strat_rel_index(const float* coord, const int32_t* qi, const int32_t* kj, int64_t m, float window,
                                    float quant, int table_rows, int32_t* out, void* stream) {
  PTV3_REQUIRE(coord && qi && kj && out, "strat_rel_index: a NULL pointer");
  PTV3_REQUIRE(m >= 0 && table_rows >= 1 && quant > 0.f, "strat_rel_index: m=%lld, table_rows=%d, quant=%g", (long long)m,
               table_rows, (double)quant);
  if (m == 0) return PTV3_OK;
  hipLaunchKernelGGL(strat_rel_index_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, coord, qi, kj,
                     m, (float)(2.0 * (double)window), quant, table_rows, out);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_strat_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, const float* coord,
                                   const float* tq, const float* tk, const float* tv, const int32_t* q_ptr,
                                   const int32_t* q_rows, const int32_t* k_ptr, const int32_t* k_rows, int64_t n_groups,
                                   int heads, int head_dim, int table_rows, float scale, float window, float quant,
                                   float* out, void* stream) {
  PTV3_REQUIRE(q && k && v && coord && tq && tk && tv && q_ptr && q_rows && k_ptr && k_rows && out,
               "strat_attn_fwd: a NULL pointer");
  PTV3_REQUIRE(ptv3_strat_attn_capable(heads, head_dim, table_rows),
               "strat_attn_fwd: heads=%d, head_dim=%d, table_rows=%d (head_dim 16, 1 .. 80 table rows)", heads, head_dim,
               table_rows);
  PTV3_REQUIRE(n_groups >= 0 && n_groups < (1ll << 31), "strat_attn_fwd: %lld groups", (long long)n_groups);
  PTV3_REQUIRE(ld >= (int64_t)heads * head_dim && ld % 4 == 0, "strat_attn_fwd: row stride %lld", (long long)ld);
  PTV3_REQUIRE(quant > 0.f && window > 0.f, "strat_attn_fwd: window=%g, quant=%g", (double)window, (double)quant);
  if (n_groups == 0) return PTV3_OK;
  const int TS = 16 * ((table_rows + 15) / 16) + 4;
  const size_t lds = ((size_t)3 * 48 * TS + 16 * 20 + 48 + 16) * 4 + 3 * 16 * 16;
  if (lds > 32 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(&strat_attn_kernel), 64 * 1024);
  hipLaunchKernelGGL(strat_attn_kernel, dim3((unsigned)n_groups, (unsigned)heads), dim3(64), lds, (hipStream_t)stream, q, k,
                     v, ld, coord, tq, tk, tv, q_ptr, q_rows, k_ptr, k_rows, out, heads, table_rows, TS, scale,
                     (float)(2.0 * (double)window), quant);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_ball_query(const float* xyz, const int32_t* offset, int num_scenes, int64_t n, float radius,
                               int max_neighbor, int64_t* idx, void* stream) {
  PTV3_REQUIRE(xyz && offset && idx, "ball_query: a NULL pointer");
  PTV3_REQUIRE(n >= 0 && n < (1ll << 31) && num_scenes >= 1 && max_neighbor >= 1 && radius > 0.f,
               "ball_query: n=%lld, %d scenes, max_neighbor=%d, radius=%g", (long long)n, num_scenes, max_neighbor,
               (double)radius);
  if (n == 0) return PTV3_OK;
  hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)cdiv(n, 128)), dim3(128), 0, (hipStream_t)stream, xyz, offset,
                     num_scenes, n, radius * radius, max_neighbor, idx);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
