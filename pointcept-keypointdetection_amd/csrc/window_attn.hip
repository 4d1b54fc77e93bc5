// Per-window QK^T / softmax / PV with the serialized-order gather and the inverse scatter fused in.
// One workgroup = (window, head, block of queries); K and V of the window stream through LDS in
// 64-key tiles (K row-major, V transposed), scores never leave registers (online softmax).
// Matrix-core layout (mma16, common.h): S^T tile = K_tile(16 keys x 16 d) * Q^T  -> query on the
// lane, keys in the 4 acc registers x 4 lane groups; that accumulator is directly the B operand
// of O^T += V^T * P^T, so P never touches LDS.
// Reference semantics: SerializedAttention.forward, point_transformer_v3m1_base.py:184-216.
#include <type_traits>
#include <algorithm>
#include "common.h"
#include <stdlib.h>
#include "profile.h"
#include "window_attn.h"

namespace ptv3 {

constexpr int WA_THREADS = 256;
constexpr int WA_WAVES = 4;
constexpr int WA_KT = 64;  // keys per LDS tile

template <typename T, int ND> struct WaCfg;
template <typename T> struct WaCfg<T, 1> { static constexpr int QT = 4; };
template <typename T> struct WaCfg<T, 2> { static constexpr int QT = 2; };
template <typename T> struct WaCfg<T, 4> { static constexpr int QT = 1; };

template <typename T, int ND>
__global__ void __launch_bounds__(WA_THREADS)
window_attn_kernel(const T* __restrict__ qkv, const int32_t* __restrict__ win_order,
                   const int32_t* __restrict__ win_inverse, T* __restrict__ out, int C, int H, int Kmax,
                   int nwin, int qsplit, float scale_log2e, const float* __restrict__ rpe,
                   const int32_t* __restrict__ cu, unsigned drop_thr = 0, unsigned drop_seed = 0, float drop_scale = 1.f,
                   float* __restrict__ lse_out = nullptr) {
  typedef typename Vec4<T>::type V4;
  constexpr int D = 16 * ND;
  constexpr int QT = WaCfg<T, ND>::QT;
  constexpr int QB = WA_WAVES * QT * 16;  // queries per workgroup
  constexpr int KS = D + 4;               // K tile row stride (elements)
  constexpr int VS = WA_KT + 4;           // V^T tile row stride (elements)

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sK = reinterpret_cast<T*>(smem);                      // [WA_KT][KS]
  T* sV = sK + WA_KT * KS;                                 // [D][VS]
  int32_t* sOrd = reinterpret_cast<int32_t*>(sV + D * VS);  // [K]

  const unsigned nwg = (unsigned)nwin * H * qsplit;
  const unsigned logical = xcd_remap(blockIdx.x, nwg);
  const int w = logical / (H * qsplit);
  const int rem = logical % (H * qsplit);
  const int h = rem / qsplit;
  const int qs = rem % qsplit;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  // varlen (cu != nullptr): window w holds the padded slots [cu[w], cu[w+1]), at most Kmax of them
  const int64_t wbase = cu ? (int64_t)cu[w] : (int64_t)w * Kmax;
  const int K = cu ? cu[w + 1] - cu[w] : Kmax;
  const int C3 = 3 * C;
  if (qs * QB >= K) return;  // workgroup-uniform: a short window needs fewer query blocks

  for (int i = tid; i < K; i += WA_THREADS) sOrd[i] = win_order[wbase + i];
  __syncthreads();

  // ---- Q fragments (B operand of the score product), pre-scaled by scale*log2(e)
  V4 qf[QT][ND];
  int qidx[QT];
  bool keep[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    qidx[t] = qs * QB + (wave * QT + t) * 16 + li;
    const bool qv = qidx[t] < K;
    const int row = qv ? sOrd[qidx[t]] : 0;
    keep[t] = qv && win_inverse[row] == (int32_t)(wbase + qidx[t]);
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      V4 raw = zero4<T>();
      if (qv) raw = *reinterpret_cast<const V4*>(qkv + (int64_t)row * C3 + h * D + 16 * c + 4 * g);
      float f[4];
      unpack4<T>(raw, f);
      qf[t][c] = pack4<T>(f[0] * scale_log2e, f[1] * scale_log2e, f[2] * scale_log2e, f[3] * scale_log2e);
    }
  }

  f32x4 o[QT][ND];
  float m[QT], l[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int c = 0; c < ND; ++c) o[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging map: thread -> (key row, 4-element chunk); D/4 chunks per row, 64 rows
  constexpr int CH = D / 4;                            // chunks per row
  constexpr int LOADS = (WA_KT * CH) / WA_THREADS;     // = ND
  V4 rk[LOADS], rv[LOADS];
  const int ntiles = (K + WA_KT - 1) / WA_KT;

  auto issue_loads = [&](int tile) {
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      int e = u * WA_THREADS + tid;
      int kk = e / CH, ch = e % CH;
      int key = tile * WA_KT + kk;
      rk[u] = zero4<T>();
      rv[u] = zero4<T>();
      if (key < K) {
        const T* base = qkv + (int64_t)sOrd[key] * C3 + h * D + 4 * ch;
        rk[u] = *reinterpret_cast<const V4*>(base + C);
        rv[u] = *reinterpret_cast<const V4*>(base + 2 * C);
      }
    }
  };
  auto write_lds = [&]() {
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      int e = u * WA_THREADS + tid;
      int kk = e / CH, ch = e % CH;
      *reinterpret_cast<V4*>(sK + kk * KS + 4 * ch) = rk[u];
      const T* pv = reinterpret_cast<const T*>(&rv[u]);
#pragma unroll
      for (int q = 0; q < 4; ++q) sV[(4 * ch + q) * VS + kk] = pv[q];
    }
  };

  issue_loads(0);
  for (int tile = 0; tile < ntiles; ++tile) {
    write_lds();
    __syncthreads();
    if (tile + 1 < ntiles) issue_loads(tile + 1);

    // fragments of this key tile shared by all query tiles of the wave
    V4 kf[4][ND], vf[ND][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        kf[kt][c] = *reinterpret_cast<const V4*>(sK + (16 * kt + li) * KS + 16 * c + 4 * g);
        vf[c][kt] = *reinterpret_cast<const V4*>(sV + (16 * c + li) * VS + 16 * kt + 4 * g);
      }
    const int key0 = tile * WA_KT;
    const bool tail = key0 + WA_KT > K;

#pragma unroll
    for (int t = 0; t < QT; ++t) {
      f32x4 s[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < ND; ++c) acc = mma16<T>(kf[kt][c], qf[t][c], acc);
        s[kt] = acc;
      }
      if (rpe != nullptr && qidx[t] < K) {
        const float* rb = rpe + (((int64_t)w * H + h) * K + qidx[t]) * K;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int key = key0 + 16 * kt + 4 * g + r;
            if (key < K) s[kt][r] += rb[key] * 1.44269504088896340736f;
          }
      }
      if (tail) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key0 + 16 * kt + 4 * g + r >= K) s[kt][r] = -INFINITY;
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m[t], mx);
      const float alpha = __builtin_amdgcn_exp2f(m[t] - mn);
      m[t] = mn;
      float ps = 0.f;
      V4 pf[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        float p0 = __builtin_amdgcn_exp2f(s[kt][0] - mn);
        float p1 = __builtin_amdgcn_exp2f(s[kt][1] - mn);
        float p2 = __builtin_amdgcn_exp2f(s[kt][2] - mn);
        float p3 = __builtin_amdgcn_exp2f(s[kt][3] - mn);
        ps += (p0 + p1) + (p2 + p3);
        if (drop_thr) {   // training with attn_drop > 0: the normaliser keeps every pair, the value sum the kept ones / (1 - p)
          const unsigned long long id = ((unsigned long long)((wbase + qidx[t]) * H + h) << 14) | (unsigned)(key0 + 16 * kt + 4 * g);
          p0 = drop_keep(id, drop_seed, drop_thr) ? p0 * drop_scale : 0.f;
          p1 = drop_keep(id + 1, drop_seed, drop_thr) ? p1 * drop_scale : 0.f;
          p2 = drop_keep(id + 2, drop_seed, drop_thr) ? p2 * drop_scale : 0.f;
          p3 = drop_keep(id + 3, drop_seed, drop_thr) ? p3 * drop_scale : 0.f;
        }
        pf[kt] = pack4<T>(p0, p1, p2, p3);
      }
      l[t] = l[t] * alpha + ps;
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        o[t][c] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) o[t][c] = mma16<T>(vf[c][kt], pf[kt], o[t][c]);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: normalise, scatter back through the inverse map (dropping borrowed duplicates)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    float lt = l[t];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const float inv = 1.0f / lt;
    // training: log2-domain log-sum-exp of every slot's row (borrowed duplicates included: the backward walks slots)
    if (lse_out && g == 0 && qidx[t] < K) lse_out[(wbase + qidx[t]) * H + h] = m[t] + __log2f(lt);
    if (keep[t]) {
      const int row = sOrd[qidx[t]];
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        V4 v = pack4<T>(o[t][c][0] * inv, o[t][c][1] * inv, o[t][c][2] * inv, o[t][c][3] * inv);
        *reinterpret_cast<V4*>(out + (int64_t)row * C + h * D + 16 * c + 4 * g) = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Resident-window variant: the K and V of the whole (window, head) are staged into LDS ONCE
// (bf16, K=1024, head_dim 16: 40 KB + 33 KB), then every wave streams its 64 queries over all key
// tiles with no further barrier.  The walk keeps no running maximum: the first key tile pins every
// row's reference to its maximum there, the later tiles add exp2(score - reference) as it comes
// (softmax is shift invariant; fp32 and bf16 keep their relative precision whatever the exponent).
// After the walk every 16-query tile checks that its sums stayed in range; one that did not - logits
// that rise by more than 64 log2 units along the keys - is walked again with the lazy rescale: the
// cross-lane max exchange and the O / l rescale run (wave-uniformly) when some row maximum grew by
// more than 2^8 since the last rescale.  Used whenever the window fits LDS; the tiled kernel above
// is the fallback.
// ------------------------------------------------------------------------------------------------
constexpr float WA_RESCALE_THR = 8.0f;  // log2 units: probabilities stay <= 256 between rescales (exact walk)
// Deferred walk: a query tile passes when every row sum l = sum_keys p, p = exp2(score - reference) >= 0, is below
// 2^64.  Then every single p is below 2^64 as well (so none was rounded to infinity, in fp32 or in bf16, and l, 1 / l
// and log2 l are ordinary numbers), and |o| <= sum p |v| < 2^64 max |v| is finite for |v| < 2^63, a factor 2 of room
// for the rounding of the sum below the fp32 limit 2^128.  Larger v are caught by the test of o itself.  The bound is
// compared on the bits of l: exponent field >= 127 + 64, which also holds for infinity and NaN.
constexpr unsigned WA_DEFER_BOUND_BITS = (127u + 64u) << 23;
enum { WA_PIN = 0, WA_DEFER = 1, WA_EXACT = 2 };

__device__ __forceinline__ float lanes_max_groups(float x) {
  // all-reduce max over the 4 lane groups g = lane >> 4 that share one query (lanes l, l^16, l^32, l^48);
  // only on the rare rescale path, so the LDS-crossbar shuffle is fine here
  x = fmaxf(x, __shfl_xor(x, 16, 64));
  return fmaxf(x, __shfl_xor(x, 32, 64));
}
__device__ __forceinline__ float lanes_sum_groups(float x) {
  x += __shfl_xor(x, 16, 64);
  return x + __shfl_xor(x, 32, 64);
}

// fmaxf(fmaxf(a, b), c) lowers to v_max3_f32 (an asm form reading MFMA results directly would need its own
// hazard padding: the compiler does not pad inside asm statements)
__device__ __forceinline__ float max3_raw(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

template <typename T> struct WaFull {
  static constexpr int VPAD = sizeof(T) == 2 ? 8 : 4;  // V^T row padding (elements): conflict-free fragment reads
};

// row sums of P: bf16 puts them on the matrix core (A = all-ones tile: every row of the product is the
// column sum of P^T, already summed over the 4 lane groups), fp32 keeps lane-partial VALU sums
template <typename T> struct RowSum;
template <> struct RowSum<__bf16> {
  static constexpr bool kOnMfma = true;
  static __device__ __forceinline__ s16x4 ones() { return s16x4{0x3F80, 0x3F80, 0x3F80, 0x3F80}; }
};
template <> struct RowSum<float> {
  static constexpr bool kOnMfma = false;
  static __device__ __forceinline__ f32x4 ones() { return f32x4{1.f, 1.f, 1.f, 1.f}; }
};

// RPE: 0 none; 1 dense bias tensor (windows, H, K, K) streamed from memory; 2 the reference's table lookup
// (RPE.forward, point_transformer_v3m1_base.py:29-48 on get_rel_pos :104-112) evaluated in the kernel:
// bias(q, k) = sum_axis table[axis*rpe_num + clamp(grid[q][axis] - grid[k][axis], -bnd, bnd) + bnd][head]
// from the window's voxel coordinates and the head's table column, both resident in LDS.
struct RpeTable { const int32_t* grid; const float* table; int pos_bnd; };

template <typename T, int ND, int RPE, int QT>
__global__ void __launch_bounds__(512)
window_attn_full_kernel(const T* __restrict__ qkv, const int32_t* __restrict__ win_order,
                        const int32_t* __restrict__ win_inverse, T* __restrict__ out, int C, int H, int Kmax,
                        int Kpad, int nwin, int qsplit, float scale_log2e, const float* __restrict__ rpe,
                        RpeTable rt, const int32_t* __restrict__ cu, float* __restrict__ lse_out) {
  typedef typename Vec4<T>::type V4;
  constexpr int D = 16 * ND;
  constexpr int KS = D + 4;
  constexpr bool SUM_MFMA = RowSum<T>::kOnMfma;
  const int VS = Kpad + WaFull<T>::VPAD;
  const int nthreads = blockDim.x;
  const int QB = (nthreads >> 6) * QT * 16;  // queries per workgroup

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sK = reinterpret_cast<T*>(smem);                         // [Kpad][KS]
  T* sV = sK + (size_t)Kpad * KS;                             // [D][VS]
  int32_t* sOrd = reinterpret_cast<int32_t*>(sV + (size_t)D * VS);  // [Kpad]
  int32_t* sGC = sOrd + Kpad;                                       // RPE == 2: [Kpad][3] voxel coordinates
  const int rpe_num = 2 * rt.pos_bnd + 1;
  float* sTab = reinterpret_cast<float*>(sGC + 3 * Kpad);           // RPE == 2: [3*rpe_num] this head's column

  const unsigned nwg = (unsigned)nwin * H * qsplit;
  const unsigned logical = xcd_remap(blockIdx.x, nwg);
  const int w = logical / (H * qsplit);
  const int rem = logical % (H * qsplit);
  const int h = rem / qsplit;
  const int qs = rem % qsplit;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  // varlen (cu != nullptr; flash_attn_varlen semantics, v3m1_base.py:207-215): window w holds the padded slots
  // [cu[w], cu[w+1]), at most Kmax of them; the LDS layout stays that of a Kmax-key window
  const int64_t wbase = cu ? (int64_t)cu[w] : (int64_t)w * Kmax;
  const int K = cu ? cu[w + 1] - cu[w] : Kmax;
  const int Kst = (K + WA_KT - 1) / WA_KT * WA_KT;  // staged rows of THIS window (<= Kpad)
  const int C3 = 3 * C;
  if (qs * QB >= K) return;  // workgroup-uniform: a short window needs fewer query blocks

  for (int i = tid; i < Kst; i += nthreads) sOrd[i] = i < K ? win_order[wbase + i] : -1;
  __syncthreads();
  if constexpr (RPE == 2) {
    for (int i = tid; i < Kst; i += nthreads) {
      const int row = sOrd[i];
#pragma unroll
      for (int d = 0; d < 3; ++d) sGC[3 * i + d] = row >= 0 ? rt.grid[(int64_t)row * 3 + d] : 0;
    }
    for (int j = tid; j < 3 * rpe_num; j += nthreads) sTab[j] = rt.table[(int64_t)j * H + h] * 1.44269504088896340736f;
  }

  // ---- stage the whole window: K row-major, V transposed.  All gathers of a pass are issued before the first LDS
  // write; a 1024-key window at head_dim 16 is ONE pass of 8 loads per thread for an 8-wave workgroup (the gathers
  // are latency-bound: two dependent passes cost two round trips)
  constexpr int CH = D / 4;
  const int total = Kst * CH;
  auto stage_pass = [&](const int e0, auto unroll_tag) {
    constexpr int U = decltype(unroll_tag)::value;
    V4 rk[U], rv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * nthreads;
      rk[u] = zero4<T>();
      rv[u] = zero4<T>();
      if (e < total) {
        const int row = sOrd[e / CH];
        if (row >= 0) {
          const T* base = qkv + (int64_t)row * C3 + h * D + 4 * (e % CH);
          rk[u] = *reinterpret_cast<const V4*>(base + C);
          rv[u] = *reinterpret_cast<const V4*>(base + 2 * C);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * nthreads;
      if (e < total) {
        const int kk = e / CH, ch = e % CH;
        *reinterpret_cast<V4*>(sK + (size_t)kk * KS + 4 * ch) = rk[u];
        const T* pv = reinterpret_cast<const T*>(&rv[u]);
#pragma unroll
        for (int q = 0; q < 4; ++q) sV[(size_t)(4 * ch + q) * VS + kk] = pv[q];
      }
    }
  };
  {
    int e0 = tid;
    for (; e0 + 4 * nthreads < total; e0 += 8 * nthreads) stage_pass(e0, std::integral_constant<int, 8>{});
    for (; e0 < total; e0 += 4 * nthreads) stage_pass(e0, std::integral_constant<int, 4>{});
  }

  // ---- Q fragments of this wave (global loads overlap the staging above)
  V4 qf[QT][ND];
  int qidx[QT];
  int qg[QT][3];
  bool keep[QT];   // this slot is the point's own (not a borrowed duplicate): fetched NOW - a load issued between the
                   // stores of the epilogue would wait for every earlier store to be acknowledged (one in-order counter)
  bool any_q = false;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    qidx[t] = qs * QB + (wave * QT + t) * 16 + li;
    const bool qv = qidx[t] < K;
    any_q |= qv;
    const int row = qv ? sOrd[qidx[t]] : 0;
    keep[t] = qv && win_inverse[row] == (int32_t)(wbase + qidx[t]);
    if constexpr (RPE == 2) {
#pragma unroll
      for (int d = 0; d < 3; ++d) qg[t][d] = qv ? rt.grid[(int64_t)row * 3 + d] : 0;
    }
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      V4 raw = zero4<T>();
      if (qv) raw = *reinterpret_cast<const V4*>(qkv + (int64_t)row * C3 + h * D + 16 * c + 4 * g);
      float f[4];
      unpack4<T>(raw, f);
      qf[t][c] = pack4<T>(f[0] * scale_log2e, f[1] * scale_log2e, f[2] * scale_log2e, f[3] * scale_log2e);
    }
  }
  __syncthreads();
  if (!__any(any_q)) return;  // whole wave past the window end: nothing left to synchronise with

  // softmax state per query tile.  negm = -(running reference max) is the INITIAL ACCUMULATOR of the score
  // product, so the matrix core hands back (score - max) and no subtraction is issued per score.
  f32x4 o[QT][ND], negm[QT], lacc[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    negm[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    lacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < ND; ++c) o[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // the all-ones A operand of the row-sum product, made opaque once: as a known constant the compiler re-creates it
  // from scalar registers (two v_mov_b64) in front of every use
  V4 ones = RowSum<T>::ones();
  asm volatile("" : "+v"(ones));

  // One 64-key tile against the wave's query tiles, in one of three modes:
  //   WA_PIN    first tile of the deferred walk: the reference of every row becomes its maximum in this tile
  //   WA_DEFER  later tiles of the deferred walk: no maximum, no compare, no branch - the score product starts from
  //             negm, then exp2, pack, row sum and P V.  Whether the unscaled sums stayed in range is checked once
  //             per query tile after the walk (below)
  //   WA_EXACT  the lazy-rescale body, for the query tiles that have to be walked again
  // `redo` (wave-uniform, WA_EXACT only): the query tiles of the wave that are walked
  auto tile_body = [&](const int tile, auto mask_tag, auto mode_tag, const unsigned redo) {
    constexpr bool MASK = decltype(mask_tag)::value;
    constexpr int MODE = decltype(mode_tag)::value;
    const int key0 = tile * WA_KT;
    V4 kf[4][ND], vf[ND][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        kf[kt][c] = *reinterpret_cast<const V4*>(sK + (size_t)(key0 + 16 * kt + li) * KS + 16 * c + 4 * g);
        vf[c][kt] = *reinterpret_cast<const V4*>(sV + (size_t)(16 * c + li) * VS + key0 + 16 * kt + 4 * g);
      }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (MODE == WA_EXACT && !((redo >> t) & 1u)) continue;
      f32x4 s[4];  // score - reference max, log2 domain
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 acc = negm[t];
#pragma unroll
        for (int c = 0; c < ND; ++c) acc = mma16<T>(kf[kt][c], qf[t][c], acc);
        s[kt] = acc;
      }
      if constexpr (RPE == 2) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int* kg = sGC + 3 * (key0 + 16 * kt + 4 * g + r);
            float bias = 0.f;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              const int rel = min(max(qg[t][d] - kg[d], -rt.pos_bnd), rt.pos_bnd) + rt.pos_bnd;
              bias += sTab[d * rpe_num + rel];
            }
            s[kt][r] += bias;
          }
      }
      if constexpr (RPE == 1) {
        if (qidx[t] < K) {
          const float* rb = rpe + (((int64_t)w * H + h) * K + qidx[t]) * K;
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int key = key0 + 16 * kt + 4 * g + r;
              if (key < K) s[kt][r] += rb[key] * 1.44269504088896340736f;
            }
        }
      }
      if constexpr (MASK) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key0 + 16 * kt + 4 * g + r >= K) s[kt][r] = -INFINITY;
      }
      if constexpr (MODE != WA_DEFER) {
        // 16 values -> 8 x v_max3_f32
        float mx = max3_raw(s[0][0], s[0][1], s[0][2]);
        mx = max3_raw(mx, s[0][3], s[1][0]);
        mx = max3_raw(mx, s[1][1], s[1][2]);
        mx = max3_raw(mx, s[1][3], s[2][0]);
        mx = max3_raw(mx, s[2][1], s[2][2]);
        mx = max3_raw(mx, s[2][3], s[3][0]);
        mx = max3_raw(mx, s[3][1], s[3][2]);
        mx = fmaxf(mx, s[3][3]);
        // The first tile pins the reference to its row maximum.  WA_EXACT, lazy rescale (wave-uniform): afterwards
        // the exchange + rescale only run when some row maximum outgrew the reference by more than 2^THR.
        if (MODE == WA_PIN || __builtin_expect(tile == 0 || __any(mx > WA_RESCALE_THR), 0)) {
          float d = lanes_max_groups(mx);      // new max - old reference (same for the 4 lanes of a query)
          if (MODE == WA_EXACT && tile > 0) {
            d = fmaxf(d, 0.f);                 // the reference never moves down after the first tile
            const float alpha = __builtin_amdgcn_exp2f(-d);
            lacc[t] *= alpha;
#pragma unroll
            for (int c = 0; c < ND; ++c) o[t][c] *= alpha;
          }
          negm[t] -= d;
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) s[kt] -= d;
        }
      }
      float ps = 0.f;
      V4 pf[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const float p0 = __builtin_amdgcn_exp2f(s[kt][0]);
        const float p1 = __builtin_amdgcn_exp2f(s[kt][1]);
        const float p2 = __builtin_amdgcn_exp2f(s[kt][2]);
        const float p3 = __builtin_amdgcn_exp2f(s[kt][3]);
        if constexpr (!SUM_MFMA) ps += (p0 + p1) + (p2 + p3);
        pf[kt] = pack4<T>(p0, p1, p2, p3);
      }
      // P V and the row sums in 32-key steps (bf16: v_mfma_f32_16x16x32_bf16, half the matrix-core issues of the
      // 16-key form; the 32 keys of a step are the two 16-key score tiles side by side, in registers as they are)
      if constexpr (SUM_MFMA) {
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) lacc[t] = mma16x2<T>(ones, ones, pf[2 * kp], pf[2 * kp + 1], lacc[t]);
      } else {
        lacc[t][0] += ps;
      }
#pragma unroll
      for (int c = 0; c < ND; ++c)
#pragma unroll
        for (int kp = 0; kp < 2; ++kp)
          o[t][c] = mma16x2<T>(vf[c][2 * kp], vf[c][2 * kp + 1], pf[2 * kp], pf[2 * kp + 1], o[t][c]);
    }
  };

  const int full_tiles = K / WA_KT;
  const bool tail = full_tiles * WA_KT < K;
  using Pin = std::integral_constant<int, WA_PIN>;
  using Defer = std::integral_constant<int, WA_DEFER>;
  using Exact = std::integral_constant<int, WA_EXACT>;
  // ---- deferred walk.  The pin tile always takes the masked form (on a full tile the mask changes nothing): one
  // instantiation less, off the steady-state loop.
  tile_body(0, std::true_type{}, Pin{}, 0u);
  for (int tile = 1; tile < full_tiles; ++tile) tile_body(tile, std::false_type{}, Defer{}, 0u);
  if (tail && full_tiles > 0) tile_body(full_tiles, std::true_type{}, Defer{}, 0u);

  // ---- did the unscaled sums stay in range?  Decided per 16-query tile (its 64 lanes are this wave's), never per
  // wave: a tile's bits must not depend on the tiles it shares a wave with.  A tile is walked again, exactly, when
  // its row sum is NaN or at or above 2^64 (WA_DEFER_BOUND_BITS), or a component of o is not finite, in any lane.
  unsigned redo = 0;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const float lsum = SUM_MFMA ? lacc[t][0] : lanes_sum_groups(lacc[t][0]);
    // on the bits: this file is compiled without NaNs in its floating-point model
    bool bad = (__float_as_uint(lsum) & 0x7fffffffu) >= WA_DEFER_BOUND_BITS;
#pragma unroll
    for (int c = 0; c < ND; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) bad |= (__float_as_uint(o[t][c][r]) & 0x7f800000u) == 0x7f800000u;
    if (__any(bad)) redo |= 1u << t;
  }
  if (__builtin_expect(redo != 0, 0)) {
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (!((redo >> t) & 1u)) continue;
      negm[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      lacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < ND; ++c) o[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int tile = 0; tile < full_tiles; ++tile) tile_body(tile, std::false_type{}, Exact{}, redo);
    if (tail) tile_body(full_tiles, std::true_type{}, Exact{}, redo);
  }

#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const float lsum = SUM_MFMA ? lacc[t][0] : lanes_sum_groups(lacc[t][0]);
    const float inv = 1.0f / lsum;
    if (lse_out && g == 0 && qidx[t] < K) lse_out[(wbase + qidx[t]) * H + h] = __log2f(lsum) - negm[t][0];   // training
    if (keep[t]) {
      const int row = sOrd[qidx[t]];
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        V4 v = pack4<T>(o[t][c][0] * inv, o[t][c][1] * inv, o[t][c][2] * inv, o[t][c][3] * inv);
        *reinterpret_cast<V4*>(out + (int64_t)row * C + h * D + 16 * c + 4 * g) = v;
      }
    }
  }
}


// ---- launch configuration of the resident-window kernel.
// A wave walks all key tiles of its QT query tiles serially, so the pair (waves per workgroup, QT) trades
// per-wave serial length (deep levels: few windows, the launch lasts as long as ONE wave) against redundant
// staging of the window (every workgroup of a (window, head) pair stages all of K/V) and against the number of
// rounds the grid needs (LDS bounds the workgroups resident per CU).  full_config() evaluates a small cost model
// (cycles on the busiest CU) over the candidates; PTV3_ATTN_WAVES / PTV3_ATTN_QT force a choice for experiments.
template <typename T> struct FullArgs {
  const T* qkv; const int32_t* wo; const int32_t* wi; T* out; int C, H, K, Kpad, nwin; float scale_log2e;
  const float* rpe; RpeTable rt; int waves; size_t lds; hipStream_t s; const int32_t* cu; float* lse;
};

template <typename T, int ND, int RPE, int QT>
static void launch_full(const FullArgs<T>& a) {
  ensure_dynamic_lds(reinterpret_cast<const void*>(&window_attn_full_kernel<T, ND, RPE, QT>), 160 * 1024);
  const int QB = a.waves * QT * 16;
  const int qsplit = (a.K + QB - 1) / QB;
  const unsigned nwg = (unsigned)a.nwin * a.H * qsplit;
  hipLaunchKernelGGL((window_attn_full_kernel<T, ND, RPE, QT>), dim3(nwg), dim3(a.waves * 64), a.lds, a.s, a.qkv, a.wo,
                     a.wi, a.out, a.C, a.H, a.K, a.Kpad, a.nwin, qsplit, a.scale_log2e, a.rpe, a.rt, a.cu, a.lse);
}

template <typename T, int ND, int QT>
static void launch_full_rpe(const FullArgs<T>& a, int rpe_mode) {
  by_value<0, 1, 2>(rpe_mode, [&](auto RPE) { launch_full<T, ND, RPE(), QT>(a); });
}

static void full_config(int64_t pairs, int K, int qt_max, size_t lds, int* waves_out, int* qt_out) {
  const char* ew = getenv("PTV3_ATTN_WAVES");
  const char* eq = getenv("PTV3_ATTN_QT");
  const int fw = ew ? atoi(ew) : 0, fq = eq ? atoi(eq) : 0;
  const int cap_lds = (int)std::max<size_t>(1, (160 * 1024) / lds);
  const double tiles = (K + WA_KT - 1) / WA_KT;
  double best = 1e300;
  int bw = 8, bq = qt_max;
  for (int waves = 8; waves >= 4; waves >>= 1) {
    if (fw && waves != fw) continue;
    for (int qt = qt_max; qt >= 1; qt >>= 1) {
      if (fq && qt != fq) continue;
      const int cap = std::min(cap_lds, 32 / waves);  // workgroups resident per CU (LDS, wave slots)
      const int QB = waves * qt * 16;
      const int64_t nwg = pairs * ((K + QB - 1) / QB);
      const int64_t per_round = 256LL * cap;
      const int64_t full_rounds = nwg / per_round;
      const int64_t rest = nwg - full_rounds * per_round;
      // one round with b workgroups on the busiest CU: staging (latency-bound, shared by the b workgroups only
      // partly) + the serial walk of a wave, stretched by the waves sharing its SIMD
      auto round_cost = [&](int64_t b) {
        const double wps = std::max(1.0, (double)b * waves / 4.0);           // waves per SIMD
        const double eff = wps >= 4 ? 0.70 : (wps >= 2 ? 0.50 : 0.35);        // issue efficiency seen in profiles
        const double walk = tiles * qt * 244.0 * wps / eff;                    // cycles
        const double stage = 2500.0 + 4.0 * K * (8.0 / waves) * std::max<double>(1.0, (double)b * 0.5);
        return walk + stage;
      };
      double cost = full_rounds * round_cost(cap);
      if (rest) cost += round_cost((rest + 255) / 256);
      if (cost < best) { best = cost; bw = waves; bq = qt; }
    }
  }
  *waves_out = bw;
  *qt_out = bq;
}

// The resident-window kernel when the window fits LDS, the tiled kernel otherwise.  Attention dropout always takes the
// tiled kernel (the mask costs ~12 integer operations per score; the resident-window kernel stays free of it); the RPE
// table lookup exists in the resident-window kernel only.  a.tiled tells the caller which one ran.
template <typename T, int ND>
static int launch_window_attn(WindowAttnCall& a) {
  constexpr int D = 16 * ND;
  constexpr int QT = WaCfg<T, ND>::QT;
  const int C = a.c, H = a.heads, K = a.patch, nwin = a.nwin;
  const float scale_log2e = a.scale * 1.44269504088896340736f;
  const RpeTable rt{a.grid_coord, a.rpe_table, a.pos_bnd};
  const bool drop = a.p_drop > 0.f;
  const int Kpad = (K + WA_KT - 1) / WA_KT * WA_KT;
  size_t lds_full = ((size_t)Kpad * (D + 4) + (size_t)D * (Kpad + WaFull<T>::VPAD)) * sizeof(T) + (size_t)Kpad * 4;
  if (rt.table) lds_full += (size_t)Kpad * 12 + (size_t)3 * (2 * rt.pos_bnd + 1) * 4;
  if (rt.table && lds_full > 160 * 1024) {
    set_error("window_attn_rpe: window of %d keys does not fit the resident-window kernel", K);
    return PTV3_ERR_UNSUPPORTED;
  }
  a.tiled = drop || lds_full > 160 * 1024;
  if (!a.tiled) {
    int waves, qt;
    full_config(nwin * (int64_t)H, K, WaCfg<T, ND>::QT, lds_full, &waves, &qt);
    const FullArgs<T> fa{(const T*)a.qkv, a.win_order, a.win_inverse, (T*)a.out, C, H, K, Kpad, nwin, scale_log2e,
                         a.rpe_bias, rt, waves, lds_full, a.stream, a.cu_seqlens, a.lse};
    const int rpe_mode = rt.table ? 2 : (a.rpe_bias ? 1 : 0);
    constexpr int QTMAX = WaCfg<T, ND>::QT;
    if (qt >= 4 && QTMAX >= 4) launch_full_rpe<T, ND, (QTMAX >= 4 ? 4 : QTMAX)>(fa, rpe_mode);
    else if (qt >= 2 && QTMAX >= 2) launch_full_rpe<T, ND, (QTMAX >= 2 ? 2 : QTMAX)>(fa, rpe_mode);
    else launch_full_rpe<T, ND, 1>(fa, rpe_mode);
    PTV3_LAUNCH_CHECK();
    return PTV3_OK;
  }
  constexpr int QB = WA_WAVES * QT * 16;
  const int qsplit = (K + QB - 1) / QB;
  const size_t lds = (size_t)(WA_KT * (D + 4) + D * (WA_KT + 4)) * sizeof(T) + (size_t)K * 4;
  if (lds > 64 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(&window_attn_kernel<T, ND>), 160 * 1024);
  const unsigned nwg = (unsigned)nwin * H * qsplit;
  const unsigned thr = drop ? (unsigned)std::min(4294967295.0, (double)a.p_drop * 4294967296.0) : 0u;
  hipLaunchKernelGGL((window_attn_kernel<T, ND>), dim3(nwg), dim3(WA_THREADS), lds, a.stream, (const T*)a.qkv,
                     a.win_order, a.win_inverse, (T*)a.out, C, H, K, nwin, qsplit, scale_log2e, a.rpe_bias, a.cu_seqlens,
                     thr, drop ? a.seed : 0u, drop ? 1.f / (1.f - a.p_drop) : 1.f, a.lse);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

int window_attn_validate(WindowAttnCall& a, const WindowAttnSpec& spec, bool backward, bool* empty) {
  const char* nm = spec.name;
  PTV3_REQUIRE(a.heads > 0 && a.c % a.heads == 0, "%s: c=%d not divisible by heads=%d", nm, a.c, a.heads);
  PTV3_REQUIRE(a.patch >= 1 && a.patch <= 16384, "%s: %s %d outside [1,16384]", nm,
               spec.ragged == WA_RAGGED_REQUIRED ? "max_seqlen" : "patch", a.patch);
  if (spec.ragged == WA_RAGGED_NO) a.cu_seqlens = nullptr;
  if (spec.ragged == WA_RAGGED_REQUIRED) {
    PTV3_REQUIRE(a.cu_seqlens != nullptr && a.num_windows >= 1, "%s: cu_seqlens with >= 1 window required", nm);
    PTV3_REQUIRE(a.n_pad <= (int64_t)a.num_windows * a.patch && a.n_pad >= a.num_windows,
                 "%s: n_pad=%lld cannot be split into %d windows of 1..%d slots", nm, (long long)a.n_pad, a.num_windows,
                 a.patch);
  } else {
    PTV3_REQUIRE(a.cu_seqlens != nullptr || a.n_pad % a.patch == 0, "%s: n_pad=%lld is not a multiple of patch=%d%s", nm,
                 (long long)a.n_pad, a.patch, spec.ragged == WA_RAGGED_NO ? " (this entry takes uniform windows only)" : "");
  }
  PTV3_REQUIRE(a.p_drop == 0.f ? !spec.drop : (a.p_drop > 0.f && a.p_drop < 1.f), "%s: p_drop %g outside (0,1)", nm,
               (double)a.p_drop);
  PTV3_REQUIRE(!spec.lse || a.lse != nullptr, "%s: lse (n_pad x heads floats) is required", nm);
  PTV3_REQUIRE(a.dtype == PTV3_F32 || a.dtype == PTV3_BF16, "%s: bad dtype %d", nm, a.dtype);
  if (spec.rpe) {
    PTV3_REQUIRE(a.grid_coord && a.rpe_table && a.pos_bnd >= 0, "%s: grid_coord, rpe_table and pos_bnd >= 0 are required", nm);
    if (!backward) PTV3_REQUIRE(a.pos_bnd <= 4096, "%s: pos_bnd %d outside [0,4096]", nm, a.pos_bnd);
    if (backward) PTV3_REQUIRE(a.dtable != nullptr, "%s: dtable is required", nm);
    if (backward && 3 * (2 * a.pos_bnd + 1) > AB_MAX_TAB) {
      set_error("%s: table column of %d entries exceeds %d", nm, 3 * (2 * a.pos_bnd + 1), AB_MAX_TAB);
      return PTV3_ERR_UNSUPPORTED;
    }
  }
  if (backward) {
    const size_t need = a.rpe_table
        ? ptv3_window_attn_rpe_bwd_workspace_bytes(a.n, a.n_pad, a.c, a.heads, a.patch, a.pos_bnd, a.dtype)
        : ptv3_window_attn_bwd_workspace_bytes(a.n, a.n_pad, a.c, a.heads, a.dtype);
    PTV3_REQUIRE(a.workspace_bytes >= need, "%s: workspace too small", nm);
  }
  a.nwin = a.cu_seqlens ? a.num_windows : (int)(a.n_pad / a.patch);
  *empty = a.n == 0;
  if (*empty && (!backward || spec.rpe)) return PTV3_OK;
  const int d = a.c / a.heads;
  if (d != 16 && d != 32 && d != 64) {
    set_error("%s: head_dim %d unsupported (16, 32, 64)", nm, d);
    return PTV3_ERR_UNSUPPORTED;
  }
  return PTV3_OK;
}

int window_attn_forward(WindowAttnCall& a, const WindowAttnSpec& spec) {
  bool empty;
  const int ok = window_attn_validate(a, spec, false, &empty);
  if (ok != PTV3_OK || empty) return ok;
  const int esz = dtype_bytes(a.dtype);
  // algorithmic work: 4 * sum_w len_w^2 * c flops; qkv read + out write + the two index maps (+ the
  // voxel coordinates of the RPE table lookup)
  const double len_sq = a.cu_seqlens && a.sum_len_sq > 0 ? a.sum_len_sq : (double)a.n_pad * a.patch;
  const double bytes = (double)a.n_pad * 3 * a.c * esz + (double)a.n * a.c * esz + 4.0 * (a.n_pad + a.n);
  const int prof = prof_begin(a.stream, PROF_WINDOW_ATTN, 4.0 * len_sq * a.c, a.rpe_table ? bytes + 12.0 * a.n_pad : bytes,
                              nullptr, 0, 0.0);
  const int rc = window_attn_dispatch(a.dtype, a.c / a.heads, [&](auto t, auto nd) {
    return launch_window_attn<typename decltype(t)::type, decltype(nd)::value>(a);
  });
  prof_kernel(prof, a.tiled ? PK_ATTN_TILED : PK_ATTN_FULL);
  prof_end(prof, a.stream);
  return rc;
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_window_attn_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                                    void* out, int64_t n, int64_t n_pad, int c, int heads, int patch,
                                    float scale, const float* rpe_bias, int dtype, void* stream) {
  WindowAttnCall a = window_attn_call(qkv, win_order, win_inverse, out, n, n_pad, c, heads, patch, scale, dtype, stream);
  a.rpe_bias = rpe_bias;
  return window_attn_forward(a, {"window_attn", WA_RAGGED_NO});
}

extern "C" int ptv3_window_attn_varlen_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                                           const int32_t* cu_seqlens, int num_windows, void* out, int64_t n,
                                           int64_t n_pad, int c, int heads, int max_seqlen, float scale,
                                           double sum_len_sq, int dtype, void* stream) {
  WindowAttnCall a = window_attn_call(qkv, win_order, win_inverse, out, n, n_pad, c, heads, max_seqlen, scale, dtype, stream);
  a.cu_seqlens = cu_seqlens; a.num_windows = num_windows; a.sum_len_sq = sum_len_sq;
  return window_attn_forward(a, {"window_attn_varlen", WA_RAGGED_REQUIRED});
}

extern "C" int ptv3_window_attn_train_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                                          const int32_t* cu_seqlens, int num_windows, void* out, float* lse, int64_t n,
                                          int64_t n_pad, int c, int heads, int patch, float scale, double sum_len_sq,
                                          int dtype, void* stream) {
  WindowAttnCall a = window_attn_call(qkv, win_order, win_inverse, out, n, n_pad, c, heads, patch, scale, dtype, stream);
  a.cu_seqlens = cu_seqlens; a.num_windows = num_windows; a.sum_len_sq = sum_len_sq; a.lse = lse;
  return window_attn_forward(a, {"window_attn_train", WA_RAGGED_OPTIONAL, /*lse*/ true});
}

extern "C" int ptv3_window_attn_drop_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                                         const int32_t* cu_seqlens, int num_windows, void* out, int64_t n, int64_t n_pad,
                                         int c, int heads, int patch, float scale, float p_drop, uint32_t seed, int dtype,
                                         void* stream) {
  WindowAttnCall a = window_attn_call(qkv, win_order, win_inverse, out, n, n_pad, c, heads, patch, scale, dtype, stream);
  a.cu_seqlens = cu_seqlens; a.num_windows = num_windows; a.p_drop = p_drop; a.seed = seed;
  return window_attn_forward(a, {"window_attn_drop", WA_RAGGED_OPTIONAL, false, false, /*drop*/ true});
}

extern "C" int ptv3_window_attn_rpe_fwd(const void* qkv, const int32_t* win_order, const int32_t* win_inverse,
                                        void* out, int64_t n, int64_t n_pad, int c, int heads, int patch, float scale,
                                        const int32_t* grid_coord, const float* rpe_table, int pos_bnd, int dtype,
                                        void* stream) {
  WindowAttnCall a = window_attn_call(qkv, win_order, win_inverse, out, n, n_pad, c, heads, patch, scale, dtype, stream);
  a.grid_coord = grid_coord; a.rpe_table = rpe_table; a.pos_bnd = pos_bnd;
  return window_attn_forward(a, {"window_attn_rpe", WA_RAGGED_NO, false, /*rpe*/ true});
}

