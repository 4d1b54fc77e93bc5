// Validation hooks on the device: the counting the reference's SemSegEvaluator / ClsEvaluator / InsSegEvaluator do per
// batch and per scene (pointcept/engines/hooks/evaluator.py, pointcept/utils/misc.py:53-65).
//   seg_argmax_kernel<T, G>      a G-lane group per row of logits: argmax with the lowest index among the maxima; either
//                                counted at once (no `inverse`) or written out as an int32 prediction per row
//   seg_count_kernel             one element of `target` per thread and pass: prediction (through `inverse`), the ignore
//                                overwrite, the three histograms
//   insseg_associate_kernel<T>   a workgroup per (proposal, chunk of IA_CHUNK mask entries): the set entries counted by
//                                the ground-truth code of the evaluated points they stand for
// Both count in an LDS histogram of 32-bit integers (ds_add_u32) that a workgroup adds to the global table at its end,
// non-zero bins only, with integer atomics: integer sums do not depend on the order, so two runs are bitwise equal and a
// row split over several workgroups gives what one workgroup would.  Every index read from memory (a prediction, a
// target, an `inverse` entry, a column's range, a code) is compared with its range before it addresses anything.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int EV_THREADS = 256;
constexpr int IA_ITEMS = 32;                        // mask entries per thread of one workgroup
constexpr int IA_CHUNK = EV_THREADS * IA_ITEMS;     // ptv3_insseg_chunk()

template <int D> struct ElemOf;
template <> struct ElemOf<PTV3_F32> { using type = float; };
template <> struct ElemOf<PTV3_BF16> { using type = __bf16; };
template <> struct ElemOf<PTV3_F16> { using type = _Float16; };
template <> struct ElemOf<PTV3_I32> { using type = int32_t; };
template <> struct ElemOf<PTV3_I64> { using type = int64_t; };
template <> struct ElemOf<PTV3_U8> { using type = uint8_t; };

// an int32 or int64 array read as int64 (wide: uniform over the launch)
__device__ __forceinline__ int64_t load_index(const void* p, bool wide, int64_t i) {
  return wide ? ((const int64_t*)p)[i] : (int64_t)((const int32_t*)p)[i];
}

// misc.py:59-63 for one element: bins[0..K) intersection, [K..2K) predicted area, [2K..3K) target area
__device__ __forceinline__ void seg_count_one(int* bins, int K, int64_t pred, int64_t tgt, int64_t ignore_index) {
  if (tgt == ignore_index) pred = ignore_index;
  const bool pin = pred >= 0 && pred < (int64_t)K;
  if (pin) atomicAdd(&bins[K + (int)pred], 1);
  if (tgt >= 0 && tgt < (int64_t)K) atomicAdd(&bins[2 * K + (int)tgt], 1);
  if (pin && pred == tgt) atomicAdd(&bins[(int)pred], 1);
}

__device__ __forceinline__ void seg_bins_clear(int* bins, int K) {
  for (int b = threadIdx.x; b < 3 * K; b += EV_THREADS) bins[b] = 0;
  __syncthreads();
}

__device__ __forceinline__ void seg_bins_flush(const int* bins, int K, int64_t* counts) {
  __syncthreads();
  for (int b = threadIdx.x; b < 3 * K; b += EV_THREADS) {
    const int v = bins[b];
    if (v) atomicAdd((unsigned long long*)(counts + b), (unsigned long long)v);
  }
}

// output.max(1)[1] (evaluator.py:39, :141) for rows of K logits; lane l of the row's group takes classes l, l + G, ...
// pred_out != NULL: the prediction of every row is stored (the caller gathers it through `inverse`); else it is counted
// against target[row] here and the logits are the only thing read twice by nobody.
template <typename T, int G>
__global__ void __launch_bounds__(EV_THREADS) seg_argmax_kernel(const T* __restrict__ logits, int64_t n, int K,
                                                                 const void* __restrict__ target, int tgt_wide,
                                                                 int64_t ignore_index, int32_t* __restrict__ pred_out,
                                                                 int64_t* __restrict__ counts) {
  extern __shared__ __align__(16) int ev_bins[];
  constexpr int RPB = EV_THREADS / G;
  const int l = threadIdx.x % G, rl = threadIdx.x / G;
  if (!pred_out) seg_bins_clear(ev_bins, K);
  for (int64_t rb = (int64_t)blockIdx.x * RPB; rb < n; rb += (int64_t)gridDim.x * RPB) {
    const int64_t r = rb + rl;
    const bool active = r < n;
    float best = 0.f;
    int arg = K;   // no class seen yet
    if (active) {
      const T* x = logits + r * K;
      for (int c = l; c < K; c += G) {
        const float v = (float)x[c];
        if (arg == K || v > best) { best = v; arg = c; }
      }
    }
#pragma unroll
    for (int m = G >> 1; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(best, m, 64);
      const int oa = __shfl_xor(arg, m, 64);
      if (oa < K && (arg == K || ov > best || (ov == best && oa < arg))) { best = ov; arg = oa; }
    }
    if (!active || l != 0) continue;
    if (pred_out) pred_out[r] = arg;
    else seg_count_one(ev_bins, K, arg, load_index(target, tgt_wide != 0, r), ignore_index);
  }
  if (!pred_out) seg_bins_flush(ev_bins, K, counts);
}

// pred (n) int32 / int64, read at inverse[e] when `inverse` is given (evaluator.py:145); an entry outside [0, n) is a
// violated precondition and its element is counted nowhere
__global__ void __launch_bounds__(EV_THREADS) seg_count_kernel(const void* __restrict__ pred, int pred_wide, int64_t n,
                                                                const int64_t* __restrict__ inverse,
                                                                const void* __restrict__ target, int tgt_wide, int64_t m,
                                                                int K, int64_t ignore_index,
                                                                int64_t* __restrict__ counts) {
  extern __shared__ __align__(16) int ev_bins[];
  seg_bins_clear(ev_bins, K);
  for (int64_t e = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; e < m; e += (int64_t)gridDim.x * EV_THREADS) {
    const int64_t r = inverse ? inverse[e] : e;
    if (r < 0 || r >= n) continue;
    seg_count_one(ev_bins, K, load_index(pred, pred_wide != 0, r), load_index(target, tgt_wide != 0, e), ignore_index);
  }
  seg_bins_flush(ev_bins, K, counts);
}

// evaluator.py:317-331 for one proposal and IA_CHUNK of its mask entries.  bins[0..G] = set entries by the code of their
// point, bins[G + 1] = set entries, bins[G + 2] = set entries on void points.  A thread reads 16 bytes of the row at a time
// where the row allows it; a group of zeros (nearly all of them: masks are a few percent dense) costs no more than that
// load, and a wavefront whose groups are all zero branches over the counting as a whole.  With col_start the evaluated
// cloud is another one (evaluator.py:569-579): mask column j stands for the evaluated points col_start[j] ..
// col_start[j + 1], whose codes are stored in that order, so the row is still read once, in order, and never gathered.
template <typename T>
__global__ void __launch_bounds__(EV_THREADS) insseg_associate_kernel(const T* __restrict__ masks, int64_t nm,
                                                                       const int32_t* __restrict__ col_start,
                                                                       const int32_t* __restrict__ code, int64_t n, int G,
                                                                       int vec_ok, int32_t* __restrict__ inter,
                                                                       int32_t* __restrict__ vert_count,
                                                                       int32_t* __restrict__ void_inter) {
  extern __shared__ __align__(16) int ev_bins[];
  constexpr int VEC = 16 / (int)sizeof(T);
  const int64_t p = blockIdx.x;
  const int64_t j0 = (int64_t)blockIdx.y * IA_CHUNK;
  const int64_t j1 = j0 + IA_CHUNK < nm ? j0 + IA_CHUNK : nm;
  const T* row = masks + p * nm;
  for (int b = threadIdx.x; b < G + 3; b += EV_THREADS) ev_bins[b] = 0;
  __syncthreads();
  int verts = 0, voids = 0;
  auto count_point = [&](int64_t i) {   // evaluated point i carries a set entry
    const int32_t c = code[i];
    const int g = c & 0x7fffffff;
    ++verts;
    voids += c < 0 ? 1 : 0;
    if (g <= G) atomicAdd(&ev_bins[g], 1);
  };
  auto count = [&](int64_t j) {         // mask column j is set
    if (!col_start) return count_point(j);
    int64_t t0 = col_start[j], t1 = col_start[j + 1];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > n ? n : t1;
    for (int64_t t = t0; t < t1; ++t) count_point(t);
  };
  if (vec_ok) {   // nm a multiple of VEC, masks 16-byte aligned, and IA_CHUNK is a multiple of VEC
    for (int64_t j = j0 + (int64_t)threadIdx.x * VEC; j < j1; j += (int64_t)EV_THREADS * VEC) {
      union { uint4 q; T e[VEC]; } u;
      u.q = *(const uint4*)(row + j);
      if ((u.q.x | u.q.y | u.q.z | u.q.w) == 0u) continue;
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (u.e[k] != (T)0) count(j + k);
    }
  } else {
    for (int64_t j = j0 + threadIdx.x; j < j1; j += EV_THREADS)
      if (row[j] != (T)0) count(j);
  }
  if (verts) atomicAdd(&ev_bins[G + 1], verts);
  if (voids) atomicAdd(&ev_bins[G + 2], voids);
  __syncthreads();
  for (int b = threadIdx.x; b <= G; b += EV_THREADS) {
    const int v = ev_bins[b];
    if (v) atomicAdd(&inter[p * (G + 1) + b], v);
  }
  if (threadIdx.x == 0) {
    if (ev_bins[G + 1]) atomicAdd(&vert_count[p], ev_bins[G + 1]);
    if (ev_bins[G + 2]) atomicAdd(&void_inter[p], ev_bins[G + 2]);
  }
}

static bool ev_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool ev_is_int(int dtype) { return dtype == PTV3_I32 || dtype == PTV3_I64; }
static int ev_group(int K) {
  int g = 2;
  while (g < K && g < 64) g <<= 1;
  return g;
}
static unsigned ev_blocks(int64_t work, int per_block) {
  const int64_t b = cdiv(work, per_block);
  return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_insseg_chunk(void) { return IA_CHUNK; }

extern "C" int ptv3_seg_confusion(const void* src, int src_dtype, int64_t n, const int64_t* inverse, const void* target,
                                  int target_dtype, int64_t m, int K, int64_t ignore_index, int64_t* counts,
                                  int32_t* pred_ws, void* stream) {
  PTV3_REQUIRE(K >= 1 && K <= PTV3_SEG_CONFUSION_MAX_K, "seg_confusion: K=%d unsupported (1 to %d classes)", K,
               PTV3_SEG_CONFUSION_MAX_K);
  PTV3_REQUIRE(n >= 0 && m >= 0 && n < (1ll << 31) && m < (1ll << 31), "seg_confusion: n=%lld, m=%lld: below 2^31",
               (long long)n, (long long)m);
  PTV3_REQUIRE(ev_is_int(target_dtype), "seg_confusion: target dtype %d (PTV3_I32 or PTV3_I64)", target_dtype);
  const bool from_logits = src_dtype == PTV3_F32 || src_dtype == PTV3_BF16 || src_dtype == PTV3_F16;
  PTV3_REQUIRE(from_logits || ev_is_int(src_dtype), "seg_confusion: src dtype %d is neither logits nor a prediction",
               src_dtype);
  PTV3_REQUIRE(inverse || m == n, "seg_confusion: target holds %lld elements for %lld rows and no inverse", (long long)m,
               (long long)n);
  PTV3_REQUIRE(counts, "seg_confusion: counts is NULL");
  if (m == 0) return PTV3_OK;
  PTV3_REQUIRE(target && (n == 0 || src), "seg_confusion: src / target is NULL");
  PTV3_REQUIRE(!(from_logits && inverse) || pred_ws, "seg_confusion: logits with an inverse need pred_ws (n) int32");
  if (n == 0) return PTV3_OK;   // every inverse entry is out of range
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)3 * K * sizeof(int);
  const int tgt_wide = target_dtype == PTV3_I64;
  if (from_logits) {
    int32_t* pred_out = inverse ? pred_ws : nullptr;
    const int g = ev_group(K);
    by_value<PTV3_F32, PTV3_BF16, PTV3_F16>(src_dtype, [&](auto D) {
      using T = typename ElemOf<D()>::type;
      by_value<2, 4, 8, 16, 32, 64>(g, [&](auto Gv) {
        hipLaunchKernelGGL((seg_argmax_kernel<T, Gv()>), dim3(ev_blocks(n, EV_THREADS / Gv())), dim3(EV_THREADS),
                           pred_out ? 0 : lds, s, (const T*)src, n, K, target, tgt_wide, ignore_index, pred_out, counts);
      });
    });
    if (pred_out)
      hipLaunchKernelGGL(seg_count_kernel, dim3(ev_blocks(m, EV_THREADS * 8)), dim3(EV_THREADS), lds, s,
                         (const void*)pred_out, 0, n, inverse, target, tgt_wide, m, K, ignore_index, counts);
  } else {
    hipLaunchKernelGGL(seg_count_kernel, dim3(ev_blocks(m, EV_THREADS * 8)), dim3(EV_THREADS), lds, s, src,
                       (int)(src_dtype == PTV3_I64), n, inverse, target, tgt_wide, m, K, ignore_index, counts);
  }
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_insseg_associate(const void* masks, int mask_dtype, int64_t P, int64_t nm, const int32_t* col_start,
                                     const int32_t* code, int64_t n, int G, int32_t* inter, int32_t* vert_count,
                                     int32_t* void_inter, void* stream) {
  PTV3_REQUIRE(G >= 0 && G <= PTV3_INSSEG_MAX_GT, "insseg_associate: G=%d unsupported (0 to %d instances)", G,
               PTV3_INSSEG_MAX_GT);
  PTV3_REQUIRE(P >= 0 && P < (1ll << 31) && nm >= 0 && nm < (1ll << 31) - 1 && n >= 0 && n < (1ll << 31),
               "insseg_associate: P=%lld, nm=%lld, n=%lld: below 2^31", (long long)P, (long long)nm, (long long)n);
  PTV3_REQUIRE(P * (int64_t)(G + 1) < (1ll << 31), "insseg_associate: P * (G + 1) must stay below 2^31");
  PTV3_REQUIRE(mask_dtype == PTV3_I32 || mask_dtype == PTV3_U8 || mask_dtype == PTV3_I64,
               "insseg_associate: mask dtype %d (PTV3_I32, PTV3_U8 or PTV3_I64)", mask_dtype);
  PTV3_REQUIRE(col_start || n == nm, "insseg_associate: %lld codes for masks of %lld points and no col_start",
               (long long)n, (long long)nm);
  PTV3_REQUIRE(cdiv(nm, IA_CHUNK) <= 65535, "insseg_associate: nm=%lld is more than 65535 chunks", (long long)nm);
  if (P == 0) return PTV3_OK;
  PTV3_REQUIRE(inter && vert_count && void_inter, "insseg_associate: inter / vert_count / void_inter is NULL");
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(inter, 0, (size_t)P * (G + 1) * sizeof(int32_t), s);
  (void)hipMemsetAsync(vert_count, 0, (size_t)P * sizeof(int32_t), s);
  (void)hipMemsetAsync(void_inter, 0, (size_t)P * sizeof(int32_t), s);
  if (n > 0 && nm > 0) {
    PTV3_REQUIRE(masks && code, "insseg_associate: masks / code is NULL");
    const dim3 grid((unsigned)P, (unsigned)cdiv(nm, IA_CHUNK));
    const size_t lds = (size_t)(G + 3) * sizeof(int);
    by_value<PTV3_I32, PTV3_U8, PTV3_I64>(mask_dtype, [&](auto D) {
      using T = typename ElemOf<D()>::type;
      const int vec_ok = ev_aligned16(masks) && nm % (16 / (int)sizeof(T)) == 0;
      hipLaunchKernelGGL(insseg_associate_kernel<T>, grid, dim3(EV_THREADS), lds, s, (const T*)masks, nm, col_start, code,
                         n, G, vec_ok, inter, vert_count, void_inter);
    });
  }
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
