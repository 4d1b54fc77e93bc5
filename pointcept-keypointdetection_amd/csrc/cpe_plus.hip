// Bottleneck xCPE of PT-v3m1-Plus (pointcept/models/keypoint_ptv3_plus.py:68-94): a narrow-channel, many-tap gather
// GEMM whose epilogue is the LayerNorm + ReLU that follows it.  One kernel serves both entry points:
//   ptv3_subm_conv_ln   cin = cout = c in {16..128}, kvol in {27, 125}, rows gathered through the neighbour table
//   ptv3_rows_linear_ln kvol = 1, no table: the 1x1 "down" conv in front of it
// Tiling: a wave owns 16 * RT whole output rows and all cout columns, so the LayerNorm
// statistics never leave the wave and no LDS or barrier is needed.  The A fragment of a matrix-core step is the
// gather itself: lane (i, g) loads the 16 bytes x[nbr[row_i][tap]][ch .. ch+E) with K index k = tap * cin + ch =
// k0 + E * g, straight into the register the MFMA reads (rows are 32..512 bytes: one to sixteen 16-byte pieces, no
// piece crosses a row).  A K step whose taps are absent for every row of the wave is skipped (wave-uniform ballot),
// which is most of a 125-tap table.  Weights (cout, kvol * cin) are read in the same 16-byte fragments from L2.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

struct ConvLnArgs {
  const void* x; const void* w; void* out;
  const int32_t* nbr; const int32_t* row_order;
  const float* bias; const float* gamma; const float* beta;
  int64_t m, rows_x;
  int cin, cin_shift, kvol, act;
  float eps;
};

// sum over the 16 lanes that share a lane group g (the columns of one output row), fixed butterfly order
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <typename T, int NT, int RT>
__global__ void __launch_bounds__(256) conv_ln_kernel(ConvLnArgs a) {
  typedef Frag<T> F;
  typedef typename F::type FR;
  constexpr int E = F::E, KC = F::KC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
  if (p0 >= a.m) return;   // wave-uniform
  const T* __restrict__ x = (const T*)a.x;
  const T* __restrict__ w = (const T*)a.w;
  const int K = a.kvol * a.cin;

  // the row this lane gathers for, per row tile (-1: past the end, or a row_order entry outside [0, m))
  int64_t arow[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t p = p0 + 16 * rt + i;
    int64_t r = -1;
    if (p < a.m) {
      r = a.row_order ? (int64_t)a.row_order[p] : p;
      if (r < 0 || r >= a.m) r = -1;
    }
    arow[rt] = r;
  }

  // blocked summation: the matrix core adds into `acc` for FLUSH executed steps, then `acc` is added to `tot` and
  // cleared - a dense row sums kvol * c = 4000 products at c = 32, and one serial fp32 chain of that length lost four
  // times the accuracy of the tiled GEMM's partial sums
  constexpr int FLUSH = 16;
  f32x4 acc[RT][NT], tot[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = tot[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int pending = 0;

  // source row of (row tile, K step): the table entry, or the row itself for the table-free linear; anything outside
  // [0, rows_x) counts as an absent tap.  A lane whose K index lies past K (c = 16 in bf16: K = 2000 is no multiple of
  // the 32-wide step, the last step holds one real tap) reads neither the table nor x nor w.
  auto source = [&](int rt, int k) -> int64_t {
    if (k >= K || arow[rt] < 0) return -1;
    if (a.nbr == nullptr) return arow[rt] < a.rows_x ? arow[rt] : -1;
    const int32_t s = a.nbr[arow[rt] * a.kvol + (k >> a.cin_shift)];
    return (s >= 0 && (int64_t)s < a.rows_x) ? (int64_t)s : -1;
  };

  int64_t src[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) src[rt] = source(rt, E * g);

  for (int k0 = 0; k0 < K; k0 += KC) {
    const int k = k0 + E * g;
    const int ch = k & (a.cin - 1);
    FR af[RT];
    bool any = false;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      af[rt] = F::zero();
      if (src[rt] >= 0) {
        af[rt] = *reinterpret_cast<const FR*>(x + src[rt] * a.cin + ch);
        any = true;
      }
    }
    // table entries of the next step, in flight under this step's multiply
    if (k0 + KC < K) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) src[rt] = source(rt, k + KC);
    }
    if (__ballot(any) == 0) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      FR bf = F::zero();
      if (k < K) bf = *reinterpret_cast<const FR*>(w + (int64_t)(16 * nt + i) * K + k);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt][nt] = F::mma(af[rt], bf, acc[rt][nt]);
    }
    if (++pending == FLUSH || k0 + KC >= K) {   // wave-uniform
      pending = 0;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { tot[rt][nt] += acc[rt][nt]; acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
  }
  // the last step may have been skipped: what is still pending
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tot[rt][nt] += acc[rt][nt];

  // epilogue: tot[rt][nt][r] is output row 4g + r of row tile rt, column 16 nt + i.  + bias, LayerNorm over the cout
  // columns (two passes, fp32: columns of a lane in nt order, then the 16 lanes by sum16), activation, store.
  constexpr int COUT = 16 * NT;
  float bs[NT], gm[NT], bt[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    bs[nt] = a.bias ? a.bias[16 * nt + i] : 0.f;
    gm[nt] = a.gamma[16 * nt + i];
    bt[nt] = a.beta[16 * nt + i];
  }
  T* __restrict__ out = (T*)a.out;
  const float inv_c = 1.0f / (float)COUT;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // arow of output row 4g + r lives in the lanes with i = 4g + r
      const int lo = __shfl((int)(arow[rt] & 0xffffffff), 4 * g + r, 64);
      const int hi = __shfl((int)(arow[rt] >> 32), 4 * g + r, 64);
      const int64_t orow = ((int64_t)hi << 32) | (unsigned)lo;
      float v[NT];
      float s = 0.f;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) { v[nt] = tot[rt][nt][r] + bs[nt]; s += v[nt]; }
      const float mean = sum16(s) * inv_c;
      float q = 0.f;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) { const float d = v[nt] - mean; q += d * d; }
      const float rstd = rsqrtf(sum16(q) * inv_c + a.eps);
      if (orow < 0) continue;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float y = (v[nt] - mean) * rstd * gm[nt] + bt[nt];
        if (a.act == PTV3_ACT_RELU) y = fmaxf(y, 0.f);
        else if (a.act == PTV3_ACT_GELU) y = gelu_erf(y);
        out[orow * COUT + 16 * nt + i] = from_f32<T>(y);
      }
    }
  }
}

template <typename T, int NT>
static void launch_nt(const ConvLnArgs& a, hipStream_t s) {
  // two row tiles per wave halve the weight reads per row; below one full wave of the chip prefer more waves
  if (a.m >= (int64_t)256 * 4 * 32) {
    hipLaunchKernelGGL((conv_ln_kernel<T, NT, 2>), dim3((unsigned)cdiv(a.m, 4 * 32)), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((conv_ln_kernel<T, NT, 1>), dim3((unsigned)cdiv(a.m, 4 * 16)), dim3(256), 0, s, a);
  }
}

template <typename T>
static int launch_conv_ln(const ConvLnArgs& a, int cout, hipStream_t s) {
  by_value<16, 32, 64, 128>(cout, [&](auto C) { launch_nt<T, C() / 16>(a, s); });   // width_ok()
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

static int shift_of(int c) {
  int s = 0;
  while ((1 << s) < c) ++s;
  return s;
}

static bool width_ok(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_subm_conv_ln_capable(int c, int kvol, int dtype) {
  return width_ok(c) && (kvol == 27 || kvol == 125) && (dtype == PTV3_F32 || dtype == PTV3_BF16);
}

extern "C" int ptv3_rows_linear_ln_capable(int c, int cout, int dtype) {
  return (width_ok(c) || c == 256 || c == 512) && width_ok(cout) && (dtype == PTV3_F32 || dtype == PTV3_BF16);
}

extern "C" int ptv3_subm_conv_ln(const void* x, const void* w, const int32_t* nbr, const int32_t* row_order,
                                 const float* bias, const float* gamma, const float* beta, void* out, int64_t m, int c,
                                 int kvol, float eps, int act, int dtype, void* stream) {
  if (!ptv3_subm_conv_ln_capable(c, kvol, dtype)) {
    set_error("subm_conv_ln: c=%d kvol=%d dtype=%d is not served (c in {16,32,64,128}, kvol in {27,125})", c, kvol, dtype);
    return PTV3_ERR_UNSUPPORTED;
  }
  PTV3_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "subm_conv_ln: m=%lld out of range", (long long)m);
  PTV3_REQUIRE(act == PTV3_ACT_NONE || act == PTV3_ACT_RELU || act == PTV3_ACT_GELU, "subm_conv_ln: bad act %d", act);
  if (m == 0) return PTV3_OK;
  PTV3_REQUIRE(x && w && nbr && gamma && beta && out, "subm_conv_ln: x, w, nbr, gamma, beta and out are required");
  ConvLnArgs a{x, w, out, nbr, row_order, bias, gamma, beta, m, m, c, shift_of(c), kvol, act, eps};
  int rc = PTV3_OK;
  by_dtype(dtype, [&](auto t) { rc = launch_conv_ln<typename decltype(t)::type>(a, c, (hipStream_t)stream); });
  return rc;
}

extern "C" int ptv3_rows_linear_ln(const void* x, const void* w, const float* bias, const float* gamma,
                                   const float* beta, void* out, int64_t m, int c, int cout, float eps, int act,
                                   int dtype, void* stream) {
  if (!ptv3_rows_linear_ln_capable(c, cout, dtype)) {
    set_error("rows_linear_ln: c=%d cout=%d dtype=%d is not served (c in {16..512}, cout in {16,32,64,128}, powers of "
              "two)", c, cout, dtype);
    return PTV3_ERR_UNSUPPORTED;
  }
  PTV3_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "rows_linear_ln: m=%lld out of range", (long long)m);
  PTV3_REQUIRE(act == PTV3_ACT_NONE || act == PTV3_ACT_RELU || act == PTV3_ACT_GELU, "rows_linear_ln: bad act %d", act);
  if (m == 0) return PTV3_OK;
  PTV3_REQUIRE(x && w && gamma && beta && out, "rows_linear_ln: x, w, gamma, beta and out are required");
  ConvLnArgs a{x, w, out, nullptr, nullptr, bias, gamma, beta, m, m, c, shift_of(c), 1, act, eps};
  int rc = PTV3_OK;
  by_dtype(dtype, [&](auto t) { rc = launch_conv_ln<typename decltype(t)::type>(a, cout, (hipStream_t)stream); });
  return rc;
}
