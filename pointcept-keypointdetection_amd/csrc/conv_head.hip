// The halo-tile 3^3 convolution fused with the block head at C in {32, 64}:
//   x = conv(x) + bias ; f1 = LayerNorm_cpe(x) + shortcut ; qkv = Linear_qkv(LayerNorm_1(f1))
// conv_halo_kernel (gemm.hip) stages its output tile through LDS, writes it, and block_head_kernel (block_fused.hip)
// reads it straight back in a launch of its own.  But the conv's accumulator acc[m][j] - channels 16 j + 4 g .. + 3 of
// site li - IS the v[j] block_head_kernel starts its register chain from, and after the last tap the halo image in
// LDS is dead and larger than the qkv weight.  So this kernel runs the tile body of conv_halo_kernel
// (halo_tile_body.inc: the same statements), then stages the chain-permuted qkv weight and the per-channel vectors over
// the dead halo and finishes both 16-site tiles of each wave as block_head_kernel would.  Every value goes through the
// operations of the two kernels in their order, with the same roundings to T: f1 and qkv are bitwise those of
// ptv3_conv_halo followed by ptv3_block_head.  The conv output is never written.
#include <stdlib.h>
#include <algorithm>
#include "common.h"
#include "profile.h"
#include "block_args.h"
#include "halo_plan.h"
#include "halo_tile.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

// Rows from which the policy takes the fused kernel; PTV3_CONV_HEAD_MIN_ROWS moves it.  Measured at 21 823 rows (171
// tiles, level 1 of the 100k-point scene: ahead of the split-K pair) and at 100 000 (profiles/conv_head); nothing was
// measured below, where the tiles fill less of the chip and the old conv splits deeper, so the bound sits just under.
constexpr int64_t CONV_HEAD_MIN_ROWS = 20480;

template <typename T, int C>
struct ConvHeadShape {
  static constexpr int LDW = C + WPad<T>::V;                       // row stride of the qkv weight in LDS
  static constexpr int WQKV = 3 * C * LDW * (int)sizeof(T);
  static constexpr int VEC = 7 * C * 4;                            // g0, b0, g1, b1, bqkv[3C]
  static constexpr int RS = 64 * (int)sizeof(T) + 16;              // row stride of a wave's output buffer: 4 tiles + padding
  static constexpr int OUT_AT = WQKV + VEC;                        // four buffers of 32 rows
  static_assert(WQKV % 16 == 0 && VEC % 16 == 0 && OUT_AT + 4 * 32 * RS <= HaloShape<T, C>::EPI_AT,
                "the qkv weight, the vectors and the output buffers overlay the dead halo, below the parked conv bias");
};

// Output rows through LDS, wave by wave.  The accumulator layout leaves a lane with 4 channels of one site: stored from
// there a wave instruction writes 16 rows x 32 bytes (bf16), and with a row_order those rows are scattered - partial
// lines (see the coalesced epilogue of gemm.hip).  Instead the wave parks NTL 16-channel tiles of its 32 sites in a
// buffer of its own (row stride RS bytes: 16 bytes of padding) and reads them back row-contiguously, 16 bytes per
// lane: an instruction then writes whole 64 .. 256-byte row segments.  No workgroup barrier: the buffer is the wave's,
// and a wave's LDS instructions execute in order.  val[m][jj]: tile jj of site 16 m + li; oid[m]: that site's output
// row, fetched from the lane that owns it; sites from `nsites` on are not stored.
template <typename T, int NTL, int RS>
__device__ __forceinline__ void wave_rows_out(char* buf, const f32x4 (&val)[2][4], T* dst, int ld, int col0,
                                              const int (&oid)[2], int nsites, int lane) {
  typedef typename Frag<T>::type FR;
  typedef typename Vec4<T>::type V4;
  constexpr int CPRW = NTL * (int)sizeof(T);              // 16-byte chunks per row segment: 4 | 8 | 16
  constexpr int RPI = 64 / CPRW, U = 32 / RPI;            // rows per wave instruction, instructions
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int jj = 0; jj < NTL; ++jj)
      *reinterpret_cast<V4*>(buf + (16 * m + li) * RS + (16 * jj + 4 * g) * (int)sizeof(T)) =
          pack4<T>(val[m][jj][0], val[m][jj][1], val[m][jj][2], val[m][jj][3]);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int r = u * RPI + lane / CPRW, ch = lane % CPRW;
    const int o0 = __shfl(oid[0], r & 15, 64), o1 = __shfl(oid[1], r & 15, 64);
    const FR chunk = *reinterpret_cast<const FR*>(buf + r * RS + 16 * ch);
    if (r < nsites)
      *reinterpret_cast<FR*>(dst + (int64_t)(r < 16 ? o0 : o1) * ld + col0 + ch * Frag<T>::E) = chunk;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename T, int C>
__global__ void __launch_bounds__(256) conv_head_halo_kernel(GemmArgs a, HaloArgs h, HeadArgs hd) {
  // Output rows of the lane's two sites (32 wave + 16 m + li of the tile).  They depend on the tile alone, so they are
  // fetched in front of the tap loop and cost no round trip behind it.  Without a row_order the load still goes out,
  // to the neighbour table (m x 27 entries: always there), and its result is dropped: no load behind a branch.
  const int64_t site0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * HALO_T + (threadIdx.x >> 6) * 32 + (threadIdx.x & 15);
  const int32_t* ro = a.row_order ? a.row_order : a.nbr;
  bool valid[2];
  int64_t prow[2];
  int32_t oid[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    valid[m] = site0 + 16 * m < a.m;
    prow[m] = valid[m] ? site0 + 16 * m : a.m - 1;
    oid[m] = ro[prow[m]];
  }

#include "halo_tile_body.inc"

  // ---- every thread is past the barrier behind the last tap: the halo image, weight stages and slot table are dead
  typedef typename Vec4<T>::type V4;
  typedef ConvHeadShape<T, C> HS;
  constexpr int NT = NJ, KC = F::KC, LDW = HS::LDW;
  constexpr int NKC = ChainFrag<T, NT>::NKC;
  T* sWq = reinterpret_cast<T*>(hc_smem);
  float* sVec = reinterpret_cast<float*>(hc_smem + HS::WQKV);
  const float *vg0 = sVec, *vb0 = sVec + C, *vg1 = sVec + 2 * C, *vb1 = sVec + 3 * C, *vbq = sVec + 4 * C;
  int64_t orow[MI];
#pragma unroll
  for (int m = 0; m < MI; ++m) orow[m] = a.row_order ? (int64_t)oid[m] : prow[m];
  // all loads of the epilogue in one batch, in front of its first store: the shortcut rows of both site tiles, the
  // vectors, the qkv weight (stage_matrix: one batch per thread)
  const T* sc = reinterpret_cast<const T*>(hd.shortcut);
  V4 sraw[MI][NT];
#pragma unroll
  for (int m = 0; m < MI; ++m)
#pragma unroll
    for (int j = 0; j < NT; ++j) sraw[m][j] = *reinterpret_cast<const V4*>(sc + orow[m] * C + 16 * j + 4 * g);
  const float fg0 = vec_fetch(hd.g0, C), fb0 = vec_fetch(hd.b0, C), fg1 = vec_fetch(hd.g1, C), fb1 = vec_fetch(hd.b1, C),
              fbq = vec_fetch(hd.bqkv, 3 * C);
  stage_matrix<T>(sWq, reinterpret_cast<const T*>(hd.wqkv), 3 * C, C, LDW);
  vec_put(sVec, fg0, hd.g0, C); vec_put(sVec + C, fb0, hd.b0, C); vec_put(sVec + 2 * C, fg1, hd.g1, C);
  vec_put(sVec + 3 * C, fb1, hd.b1, C); vec_put(sVec + 4 * C, fbq, hd.bqkv, 3 * C);

  // x = the conv output as conv_halo_kernel parks it (bias -> folded BN -> activation, rounded to T)
  f32x4 v[MI][NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const EpiVec ev = load_epi(sEpi, C, 16 * j + 4 * g);
#pragma unroll
    for (int m = 0; m < MI; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[m][j][r] = round_to<T>(epi_value(acc[m][j][r], ev, r, a.act));
  }
  __syncthreads();

  // ---- block_head_kernel's chain for the wave's two site tiles; f1 and qkv leave through the wave's row buffer
  T* f1 = reinterpret_cast<T*>(hd.f1);
  char* sOut = hc_smem + HS::OUT_AT + wave * (32 * HS::RS);
  const int out_row[2] = {(int)orow[0], (int)orow[1]};
  const int nsites = (int)min((int64_t)32, a.m - (row0 + 32 * wave));   // of the wave's 32 sites (<= 0: none)
  FR xf[MI][NKC];
#pragma unroll
  for (int m = 0; m < MI; ++m) {
    float mean, rstd;
    row_norm<NT>(v[m], hd.eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int ch = 16 * j + 4 * g;
      const f32x4 gm = *reinterpret_cast<const f32x4*>(vg0 + ch), bt = *reinterpret_cast<const f32x4*>(vb0 + ch);
      float s[4];
      unpack4<T>(sraw[m][j], s);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[m][j][r] = round_to<T>((v[m][j][r] - mean) * rstd * gm[r] + bt[r] + s[r]);
    }
  }
  {
    f32x4 t[MI][4];
#pragma unroll
    for (int m = 0; m < MI; ++m)
#pragma unroll
      for (int j = 0; j < NT; ++j) t[m][j] = v[m][j];
    wave_rows_out<T, NT, HS::RS>(sOut, t, f1, C, 0, out_row, nsites, lane);
  }
#pragma unroll
  for (int m = 0; m < MI; ++m) {
    float mean, rstd;
    row_norm<NT>(v[m], hd.eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int ch = 16 * j + 4 * g;
      const f32x4 gm = *reinterpret_cast<const f32x4*>(vg1 + ch), bt = *reinterpret_cast<const f32x4*>(vb1 + ch);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[m][j][r] = round_to<T>((v[m][j][r] - mean) * rstd * gm[r] + bt[r]);
    }
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) xf[m][kc] = ChainFrag<T, NT>::get(v[m], kc);
  }

  // qkv = t3 @ Wqkv^T + b : 3*NT output tiles, 4 at a time; a weight fragment feeds both site tiles
  T* qkv = reinterpret_cast<T*>(hd.qkv);
  constexpr int OT = 3 * NT;
  static_for<0, (OT + 3) / 4>([&](auto gc) {
    constexpr int o0 = 4 * decltype(gc)::value, NTL = OT - o0 < 4 ? OT - o0 : 4;
    f32x4 o[MI][4];
#pragma unroll
    for (int m = 0; m < MI; ++m)
#pragma unroll
      for (int jj = 0; jj < NTL; ++jj) o[m][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
      for (int jj = 0; jj < NTL; ++jj) {
        const FR wa = *reinterpret_cast<const FR*>(sWq + (16 * (o0 + jj) + li) * LDW + KC * kc + E * g);
#pragma unroll
        for (int m = 0; m < MI; ++m) o[m][jj] = F::mma(wa, xf[m][kc], o[m][jj]);
      }
#pragma unroll
    for (int jj = 0; jj < NTL; ++jj) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(vbq + 16 * (o0 + jj) + 4 * g);
#pragma unroll
      for (int m = 0; m < MI; ++m) o[m][jj] += b;
    }
    wave_rows_out<T, NTL, HS::RS>(sOut, o, qkv, 3 * C, 16 * o0, out_row, nsites, lane);
  });
}

// Policy: bf16, C = 64, rows from CONV_HEAD_MIN_ROWS; the kernel never splits over K, so whether ptv3_gemm would does
// not matter.  C = 32 (encoder 0) runs and is tested, but its fall at 100 000 rows, 4.8 us, did not exceed the spread of
// the two kernels it replaces, so it stays on them.  PTV3_CONV_HEAD: 0 off, 1 policy (default), 2 force (tests, tools: every shape the kernel can
// run); PTV3_CONV_HEAD_MIN_ROWS moves the row bound.  Both are read per call like their siblings.
static bool use_conv_head(int64_t m, int c, int dtype) {
  const char* env = getenv("PTV3_CONV_HEAD");
  const int mode = env ? atoi(env) : 1;
  if (mode == 0 || (c != 32 && c != 64)) return false;
  if (dtype != PTV3_F32 && dtype != PTV3_BF16) return false;
  if (mode == 2) return true;
  const char* rows = getenv("PTV3_CONV_HEAD_MIN_ROWS");
  return dtype == PTV3_BF16 && c == 64 && m >= (rows ? atoll(rows) : CONV_HEAD_MIN_ROWS);
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_conv_head_halo_policy(int64_t m, int c, int dtype) { return use_conv_head(m, c, dtype) ? 1 : 0; }

extern "C" int ptv3_conv_head_halo(const void* x, const void* w, const float* conv_bias, int64_t m, int c,
                                   const int32_t* nbr, const int32_t* row_order, const void* plan, size_t plan_bytes,
                                   const void* shortcut, const float* g0, const float* b0, const float* g1,
                                   const float* b1, const void* wqkv, const float* bqkv, void* f1, void* qkv, float eps,
                                   int dtype, void* stream) {
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "conv_head_halo: bad dtype %d", dtype);
  PTV3_REQUIRE(c == 32 || c == 64, "conv_head_halo: c = %d must be 32 or 64", c);
  PTV3_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "conv_head_halo: m=%lld out of range", (long long)m);
  if (m == 0) return PTV3_OK;
  PTV3_REQUIRE(x && w && nbr, "conv_head_halo: x, w and the 27-tap neighbour table are required");
  PTV3_REQUIRE(shortcut && g0 && b0 && g1 && b1 && wqkv && bqkv && f1 && qkv,
               "conv_head_halo: shortcut, the two LayerNorms, the qkv linear, f1 and qkv are required");
  PTV3_REQUIRE(plan && plan_bytes >= halo_plan_bytes(m) && ((uintptr_t)plan & 15) == 0,
               "conv_head_halo: plan must be the one ptv3_halo_plan_build wrote for these m rows");
  const HaloPlan p = halo_layout(const_cast<void*>(plan), m);
  GemmArgs a{x, w, nullptr, nullptr, nullptr, nbr, row_order, nullptr, conv_bias, nullptr, nullptr, nullptr,
             m, c, c, HALO_TAPS, 0, c == 32 ? 5 : 6, 0, 0, 0};
  const HaloArgs h{p.count, p.rows, p.slots};
  const HeadArgs hd{nullptr, nullptr, 0, nullptr, shortcut, g0, b0, g1, b1, wqkv, bqkv, f1, qkv, m, eps};
  hipStream_t s = (hipStream_t)stream;
  const int esz = dtype_bytes(dtype);
  const int prof = prof_begin(s, PROF_SUBM_CONV, 2.0 * m * HALO_TAPS * c * c + 2.0 * m * c * 3 * c,
                              ((double)m * c * 6 + (double)(HALO_TAPS + 3) * c * c) * esz, nbr, m * HALO_TAPS, 2.0 * c * c);
  prof_kernel(prof, PK_CONV_HEAD_HALO);
  const dim3 grid((unsigned)p.tiles);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_value<32, 64>(c, [&](auto C) {
      const int lds = HaloShape<T, C()>::LDS;
      ensure_dynamic_lds(reinterpret_cast<const void*>(&conv_head_halo_kernel<T, C()>), lds);
      hipLaunchKernelGGL((conv_head_halo_kernel<T, C()>), grid, dim3(256), lds, s, a, h, hd);
    });
  });
  prof_end(prof, s);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
