// What the two kernels built on the halo tile of the narrow 3^3 convolutions share: conv_halo_kernel (gemm.hip) and
// conv_head_halo_kernel (conv_head.hip), which feeds the accumulators to the block head's register chain instead of
// storing them.  The tile body itself is halo_tile_body.inc; here are the GEMM argument block and the epilogue-vector
// helpers of gemm.hip (the body parks those vectors), static_for, and the tile's arguments and LDS layout.
#pragma once
#include <type_traits>
#include "common.h"
#include "halo_plan.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

struct GemmArgs {
  const void* x; const void* w; void* out; void* out2; const void* res;
  const int32_t* nbr; const int32_t* row_order; const int32_t* res_index;
  const float* bias; const float* bn_scale; const float* bn_shift;
  float* slab;  // split-K partial sums [splits][m][cout] fp32 (NULL: direct epilogue)
  int64_t m; int cin; int cout; int kvol; int act; int cin_shift; int steps_per_split;
  int64_t x_bytes;   // size of x in bytes when it is known to be < 2^31 (buffer-descriptor addressing), else 0
  int ablate;        // tools only (PTV3_CONV_ABLATE): bit 0 no matrix-core work / fragment reads, 1 no operand copies, 2 no waits / barriers
};

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == PTV3_ACT_GELU) return gelu_erf(v);
  if (act == PTV3_ACT_RELU) return fmaxf(v, 0.f);
  return v;
}

// The per-channel epilogue vectors of one accumulator fragment (channels ch0..ch0+3; cout % 4 == 0 on this path), as
// three 16-byte loads.  All fragments' vectors are fetched back to back BEFORE any is used: one memory round trip.
// (Fetched one channel at a time inside the value loop - the first form of this epilogue - every element paid its
// own s_waitcnt vmcnt(0): ~60 dependent round trips per wave, 2/3 of a short-K linear's run time.)
struct EpiVec { f32x4 bias, scale, shift; };
// The tile's bn channels of the three vectors are parked in LDS at kernel start (sEpi: [3][bn] floats, visible after
// the first barrier of the K loop): the epilogue reads them back with three ds_read_b128 per fragment - no registers
// held across the K loop, no global load between the output stores.
__device__ __forceinline__ void park_epi(const GemmArgs& a, float* sEpi, int bn, int n0, int tid, int nthreads) {
  for (int t = tid; t < bn; t += nthreads) {
    const int ch = n0 + t;
    const bool in = ch < a.cout;
    sEpi[t] = (in && a.bias) ? a.bias[ch] : 0.f;
    sEpi[bn + t] = (in && a.bn_scale) ? a.bn_scale[ch] : 1.f;
    sEpi[2 * bn + t] = (in && a.bn_scale) ? a.bn_shift[ch] : 0.f;
  }
}
__device__ __forceinline__ EpiVec load_epi(const float* sEpi, int bn, int cl) {
  return EpiVec{*reinterpret_cast<const f32x4*>(sEpi + cl), *reinterpret_cast<const f32x4*>(sEpi + bn + cl),
                *reinterpret_cast<const f32x4*>(sEpi + 2 * bn + cl)};
}
// bias -> folded BN -> activation of one accumulator element, in fp32 (the caller rounds to T)
__device__ __forceinline__ float epi_value(float acc, const EpiVec& e, int r, int act) {
  return apply_act((acc + e.bias[r]) * e.scale[r] + e.shift[r], act);
}

template <int N, int END, class Fn>
__device__ __forceinline__ void static_for(Fn&& f) {
  if constexpr (N < END) {
    f(std::integral_constant<int, N>{});
    static_for<N + 1, END>(f);
  }
}

struct HaloArgs { const int32_t* count; const int32_t* rows; const uint16_t* slots; };

template <typename T, int C>
struct HaloShape {
  static constexpr int RB = C * (int)sizeof(T);           // bytes per halo / weight row
  static constexpr int TPS = RB == 64 ? 2 : 1;            // taps per weight stage: a stage is at least 4 KB (one chunk per thread)
  static constexpr int NSTG = (HALO_TAPS + TPS - 1) / TPS;
  static constexpr int HALO = (HALO_CAP + 1) * RB;        // rows 0..CAP-1 + the zero row
  static constexpr int WBUF = TPS * C * RB;               // one weight stage
  static constexpr int SLOT = HALO_T * HALO_TAPS * 2;     // 6912 bytes: a multiple of 16
  static constexpr int EPI = 3 * C * 4;
  static constexpr int LDS = HALO + 2 * WBUF + SLOT + EPI;
  static constexpr int EPI_AT = HALO + 2 * WBUF + SLOT;   // byte offset of the parked epilogue vectors
  static_assert(HALO >= HALO_T * (RB + 16), "the staged output tile overlays the halo");
  static_assert(LDS <= 160 * 1024, "conv_halo_kernel: LDS");
};

}  // namespace ptv3
