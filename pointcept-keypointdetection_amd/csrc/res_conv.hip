// Residual-block convolution of SpUNet's BasicBlock (pointcept/models/sparse_unet/spconv_unet_v1m1_base.py:72-85) with
// the decoder's skip concatenation (:269-273) folded into the gather.  One launch computes
//   x[i]       = concat(xa[i], xb[i])                                   never written: the gather picks the source
//   y[i][o]    = sum_{d<27} sum_{c<ca+cb} w[o][d][c] * x[nbr[i][d]][c]
//   out[i][o]  = act(y * bn_scale[o] + bn_shift[o] + res[i][o])         residual BEFORE the activation
//   proj[i][o] = (sum_c w_proj[o][c] * x[i][c]) * proj_scale[o] + proj_shift[o]      optional second output
// fp32, exact-fp32 matrix-core steps (4 x v_mfma_f32_16x16x4_f32 per 16 K elements), as ptv3_gemm's parity mode.
//
// Tiling: a 4-wave workgroup owns 64 * RT points x BN = 16 * NT output channels; a wave holds
// 16 * RT points against ALL BN channels, so one LDS fragment read feeds RT * NT / (RT + NT) matrix-core steps (0.86 at
// 16 x 96, 1.5 at 32 x 96; gemm_kernel's 16 x 64 wave tile: 0.8).  96 output channels are ONE 96-wide column block
// (NT = 6): no half-empty second block and every site row gathered once.  cout > 128 runs in 128-wide blocks.
// K runs in steps of 32 floats over k = tap * (ca + cb) + channel; a 16-byte chunk never straddles a tap or the source
// boundary (ca, cb multiples of 4), a step may straddle both: tap and source are worked out per chunk.  The K steps that
// overlap the centre tap (k in [13 cin, 14 cin)) hold x[i] itself: the projection multiplies the same A tile by a second
// weight tile that is zero outside the centre tap's columns, into its own accumulators; x is not gathered again.
// Long sums are blocked as in csrc/cpe_plus.hip: the matrix core adds into `acc` for RC_FLUSH steps (512 products),
// then `acc` moves into `tot`: K = 27 * 384 would otherwise be one fp32 chain of 2592 matrix-core additions.
#include "common.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int RC_THREADS = 256;
constexpr int RC_BK = 32;            // K floats per step: 128 bytes per LDS row
constexpr int RC_LS = RC_BK + 4;     // LDS row stride (floats): +16 bytes keeps ds_read_b128 conflict-free
constexpr int RC_CPR = RC_BK / 4;    // 16-byte chunks per row
constexpr int RC_KVOL = 27;
constexpr int RC_CENTRE = 13;
constexpr int RC_FLUSH = 16;
constexpr int RC_MAX_COUT = 512;
constexpr int RC_MAX_CIN = 1024;

struct ResConvArgs {
  const float* xa; const float* xb; const float* w; const float* w_proj;
  const int32_t* nbr; const int32_t* row_order;
  const float* bn_scale; const float* bn_shift; const float* res;
  const float* proj_scale; const float* proj_shift;
  float* out; float* proj_out;
  int64_t m;
  int ca, cb, cout, act;
};

static size_t rc_lds_bytes(int nt, int rt, bool proj) {
  const int bm = 64 * rt, bn = 16 * nt;
  return (size_t)(bm * RC_LS + bn * RC_LS * (proj ? 2 : 1)) * sizeof(float) + (size_t)bm * RC_KVOL * sizeof(int32_t);
}

// Called before vector instructions read accumulators that a matrix-core instruction may still be writing.  A
// v_mfma_f32_16x16x4_f32 writes its four result registers over several passes; inside one basic block the compiler
// puts the wait states in front of a reader, but the flush of `acc` is reached through the branch that skips the
// projection's matrix-core steps, and across that branch it did not.  Seen in NT = 1 with the projection: the
// v_pk_add_f32 of the flush read result registers 2 and 3 five scalar instructions after the last MFMA, and channels
// 4g + 2, 4g + 3 of `tot` missed one K chunk (MI355X: the 16+16 -> 16 decoder front's conv output off by 2.7e-2 to
// 4.2e-2, which two layers on is the 5.8e-3 of DESIGN.md section 17).
// Compiler: AMD clang 22.0.0git, roc-7.2.0 (HIP 7.2.26015), gfx950, -O3.  Not tied to the Makefile's
// -mllvm -amdgpu-mfma-vgpr-form: without the flag the same place becomes v_accvgpr_read_b32 of the four results
// straight behind the branch, again with no s_nop (seen in the ISA; only the flag's form has run on the device).
// To re-check with a later compiler: take the s_nop line out, build, and look in res_conv_kernel<1, 1, true> at the
// block behind the second "s_cbranch_vccnz" after the MFMAs; tests/test_hip_res_conv.py case (16, 16, 16) fails
// without the wait states.  32 wait states cover the longest pass count; the empty asms make every later read of `acc`
// depend on them.  Once per 16 K steps and once in front of the epilogue.
template <int RT, int NT>
__device__ __forceinline__ void settle(f32x4 (&acc)[RT][NT]) {
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int j = 0; j < NT; ++j) asm volatile("" : "+v"(acc[rt][j]));
}

template <int NT, int RT, bool PROJ>
__global__ void __launch_bounds__(RC_THREADS) res_conv_kernel(ResConvArgs a) {
  constexpr int BM = 64 * RT, BN = 16 * NT;
  constexpr int A_LOADS = BM * RC_CPR / RC_THREADS;                      // 2 RT
  constexpr int B_LOADS = (BN * RC_CPR + RC_THREADS - 1) / RC_THREADS;   // 1 .. 4
  extern __shared__ __attribute__((aligned(16))) float rc_smem[];
  float* sA = rc_smem;
  float* sB = sA + BM * RC_LS;
  float* sP = sB + BN * RC_LS;
  int32_t* sNbr = reinterpret_cast<int32_t*>(sP + (PROJ ? BN * RC_LS : 0));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int cin = a.ca + a.cb;
  const int ktot = RC_KVOL * cin;
  const int nsteps = (ktot + RC_BK - 1) / RC_BK;
  const int c_lo = RC_CENTRE * cin, c_hi = c_lo + cin;   // K range of the centre tap

  // the row a tile position works on: row_order[p] or p; -1 past the end or for an entry outside [0, m)
  auto site = [&](int64_t p) -> int64_t {
    if (p >= a.m) return -1;
    const int64_t r = a.row_order ? (int64_t)a.row_order[p] : p;
    return (r >= 0 && r < a.m) ? r : -1;
  };

  // neighbour rows of the tile's points; an entry outside [0, m) counts as an absent tap
  for (int e = tid; e < BM * RC_KVOL; e += RC_THREADS) {
    const int pr = e / RC_KVOL, d = e - pr * RC_KVOL;
    const int64_t r = site(row0 + pr);
    int32_t s = -1;
    if (r >= 0) {
      s = a.nbr[r * RC_KVOL + d];
      if (s < 0 || (int64_t)s >= a.m) s = -1;
    }
    sNbr[e] = s;
  }
  __syncthreads();

  // staging: chunk e = tid + 256 u -> tile row (tid >> 3) + 32 u, 16-byte column tid & 7: one K index, hence one tap
  // and one source, for all chunks of a thread
  const int s_r = tid >> 3, s_c = tid & 7;
  f32x4 ra[A_LOADS], rb[B_LOADS], rp[PROJ ? B_LOADS : 1];
  unsigned ok = 0;
  // loads are issued unconditionally from a valid dummy address and zeroed on the way to LDS (see gemm_kernel)
  auto issue = [&](int step) {
    const int kk = step * RC_BK + 4 * s_c;
    const bool in = kk < ktot;
    const int d = in ? kk / cin : 0;
    const int c = in ? kk - d * cin : 0;
    const bool second = c >= a.ca;
    const float* __restrict__ px = second ? a.xb : a.xa;
    const int ld = second ? a.cb : a.ca;
    const int cc = second ? c - a.ca : c;
    ok = 0;
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) {
      const int32_t s = sNbr[(s_r + 32 * u) * RC_KVOL + d];
      const bool v = in && s >= 0;
      ok |= (unsigned)v << u;
      ra[u] = *reinterpret_cast<const f32x4*>(px + (int64_t)(v ? s : 0) * ld + cc);
    }
#pragma unroll
    for (int u = 0; u < B_LOADS; ++u) {
      const int br = s_r + 32 * u;
      const int o = n0 + br;
      const bool v = in && br < BN && o < a.cout;
      ok |= (unsigned)v << (8 + u);
      rb[u] = *reinterpret_cast<const f32x4*>(a.w + (int64_t)(v ? o : 0) * ktot + (v ? kk : 0));
    }
    if constexpr (PROJ) {
      if (step * RC_BK < c_hi && step * RC_BK + RC_BK > c_lo) {   // workgroup-uniform
#pragma unroll
        for (int u = 0; u < B_LOADS; ++u) {
          const int br = s_r + 32 * u;
          const int o = n0 + br;
          const bool v = in && d == RC_CENTRE && br < BN && o < a.cout;
          ok |= (unsigned)v << (16 + u);
          rp[u] = *reinterpret_cast<const f32x4*>(a.w_proj + (int64_t)(v ? o : 0) * cin + (v ? c : 0));
        }
      }
    }
  };
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  auto stash = [&](bool pstep) {
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u)
      *reinterpret_cast<f32x4*>(sA + (s_r + 32 * u) * RC_LS + 4 * s_c) = ((ok >> u) & 1u) ? ra[u] : zero;
#pragma unroll
    for (int u = 0; u < B_LOADS; ++u)
      if (s_r + 32 * u < BN)
        *reinterpret_cast<f32x4*>(sB + (s_r + 32 * u) * RC_LS + 4 * s_c) = ((ok >> (8 + u)) & 1u) ? rb[u] : zero;
    if constexpr (PROJ) {
      if (pstep) {
#pragma unroll
        for (int u = 0; u < B_LOADS; ++u)
          if (s_r + 32 * u < BN)
            *reinterpret_cast<f32x4*>(sP + (s_r + 32 * u) * RC_LS + 4 * s_c) = ((ok >> (16 + u)) & 1u) ? rp[u] : zero;
      }
    }
  };

  f32x4 acc[RT][NT], tot[RT][NT], accp[PROJ ? RT : 1][PROJ ? NT : 1];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      acc[rt][j] = tot[rt][j] = zero;
      if constexpr (PROJ) accp[rt][j] = zero;
    }
  int pending = 0;

  issue(0);
  for (int step = 0; step < nsteps; ++step) {
    const bool pstep = PROJ && step * RC_BK < c_hi && step * RC_BK + RC_BK > c_lo;   // workgroup-uniform
    stash(pstep);
    __syncthreads();
    if (step + 1 < nsteps) issue(step + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f32x4 xf[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        xf[rt] = *reinterpret_cast<const f32x4*>(sA + (16 * RT * wave + 16 * rt + li) * RC_LS + 16 * ks + 4 * g);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const f32x4 wf = *reinterpret_cast<const f32x4*>(sB + (16 * j + li) * RC_LS + 16 * ks + 4 * g);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][j] = mma16<float>(wf, xf[rt], acc[rt][j]);   // D[channel 4g+r][point li]
      }
      if constexpr (PROJ) {
        if (pstep) {
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const f32x4 pf = *reinterpret_cast<const f32x4*>(sP + (16 * j + li) * RC_LS + 16 * ks + 4 * g);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) accp[rt][j] = mma16<float>(pf, xf[rt], accp[rt][j]);
          }
        }
      }
    }
    if (++pending == RC_FLUSH) {
      pending = 0;
      settle(acc);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < NT; ++j) { tot[rt][j] += acc[rt][j]; acc[rt][j] = zero; }
    }
    __syncthreads();
  }

  // epilogue: the lane owns point 16 RT wave + 16 rt + li, channels n0 + 16 j + 4 g .. + 3
  settle(acc);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t orow = site(row0 + 16 * RT * wave + 16 * rt + li);
    if (orow < 0) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int ch0 = n0 + 16 * j + 4 * g;
      if (ch0 >= a.cout) continue;           // cout % 4 == 0: a group of 4 channels is inside or outside
      f32x4 v = tot[rt][j] + acc[rt][j];
      if (a.bn_scale) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(a.bn_scale + ch0);
        const f32x4 t = *reinterpret_cast<const f32x4*>(a.bn_shift + ch0);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] * s[r] + t[r];
      }
      if (a.res) v += *reinterpret_cast<const f32x4*>(a.res + orow * a.cout + ch0);
      if (a.act == PTV3_ACT_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      } else if (a.act == PTV3_ACT_GELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
      }
      *reinterpret_cast<f32x4*>(a.out + orow * a.cout + ch0) = v;
      if constexpr (PROJ) {
        f32x4 p = accp[rt][j];
        if (a.proj_scale) {
          const f32x4 s = *reinterpret_cast<const f32x4*>(a.proj_scale + ch0);
          const f32x4 t = *reinterpret_cast<const f32x4*>(a.proj_shift + ch0);
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = p[r] * s[r] + t[r];
        }
        *reinterpret_cast<f32x4*>(a.proj_out + orow * a.cout + ch0) = p;
      }
    }
  }
}

template <int NT, int RT, bool PROJ>
static void launch_rc(const ResConvArgs& a, hipStream_t s) {
  const size_t lds = rc_lds_bytes(NT, RT, PROJ);
  ensure_dynamic_lds(reinterpret_cast<const void*>(&res_conv_kernel<NT, RT, PROJ>), (int)lds);
  dim3 grid((unsigned)cdiv(a.m, 64 * RT), (unsigned)cdiv(a.cout, 16 * NT));
  hipLaunchKernelGGL((res_conv_kernel<NT, RT, PROJ>), grid, dim3(RC_THREADS), lds, s, a);
}

// column block: 16 NT channels, the narrowest that holds cout up to 128; wider outputs run in 128-wide blocks
static int rc_nt(int cout) { return cout <= 16 ? 1 : cout <= 32 ? 2 : cout <= 64 ? 4 : cout <= 96 ? 6 : 8; }

// 16-point row tiles per wave: 2 (128-point workgroups) once they still give every CU two workgroups, else 1
static int rc_row_tiles(int64_t m, int cout) { return cdiv(m, 128) * cdiv(cout, 16 * rc_nt(cout)) >= 512 ? 2 : 1; }

template <int NT>
static void launch_nt(const ResConvArgs& a, hipStream_t s) {
  // 128-point tiles once they still give every CU two workgroups; fewer rows prefer more, smaller tiles
  const bool wide = rc_row_tiles(a.m, a.cout) == 2;
  const bool proj = a.w_proj != nullptr;
  if (wide) { if (proj) launch_rc<NT, 2, true>(a, s); else launch_rc<NT, 2, false>(a, s); }
  else      { if (proj) launch_rc<NT, 1, true>(a, s); else launch_rc<NT, 1, false>(a, s); }
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_res_conv_capable(int64_t m, int ca, int cb, int cout, int kvol) {
  return m >= 1 && m < ((int64_t)1 << 31) && kvol == RC_KVOL && ca >= 4 && ca % 4 == 0 && cb >= 0 && cb % 4 == 0 &&
         ca + cb <= RC_MAX_CIN && cout >= 4 && cout % 4 == 0 && cout <= RC_MAX_COUT;
}

extern "C" int ptv3_res_conv_row_tiles(int64_t m, int cout) {
  return (m >= 1 && cout >= 4 && cout <= RC_MAX_COUT) ? rc_row_tiles(m, cout) : 0;
}

extern "C" int ptv3_res_conv(const float* xa, const float* xb, const float* w, const int32_t* nbr,
                             const int32_t* row_order, const float* bn_scale, const float* bn_shift, const float* res,
                             int act, float* out, const float* w_proj, const float* proj_scale,
                             const float* proj_shift, float* proj_out, int64_t m, int ca, int cb, int cout, int kvol,
                             void* stream) {
  PTV3_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "res_conv: m=%lld out of range", (long long)m);
  PTV3_REQUIRE(ca >= 4 && ca % 4 == 0 && cb >= 0 && cb % 4 == 0, "res_conv: ca=%d, cb=%d must be multiples of 4 (ca >= 4)",
               ca, cb);
  PTV3_REQUIRE(cout >= 4 && cout % 4 == 0, "res_conv: cout=%d must be a positive multiple of 4", cout);
  PTV3_REQUIRE(kvol == RC_KVOL && nbr != nullptr, "res_conv: kvol=%d: a 3^3 neighbour table (kvol = 27) is required", kvol);
  PTV3_REQUIRE(act == PTV3_ACT_NONE || act == PTV3_ACT_RELU || act == PTV3_ACT_GELU, "res_conv: bad act %d", act);
  PTV3_REQUIRE(xa && w && out, "res_conv: xa, w and out are required");
  PTV3_REQUIRE((cb == 0) == (xb == nullptr), "res_conv: xb must be given exactly when cb > 0");
  PTV3_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "res_conv: bn_scale and bn_shift come together");
  PTV3_REQUIRE((w_proj == nullptr) == (proj_out == nullptr), "res_conv: w_proj and proj_out come together");
  PTV3_REQUIRE((proj_scale == nullptr) == (proj_shift == nullptr) && (w_proj != nullptr || proj_scale == nullptr),
               "res_conv: proj_scale and proj_shift come together and need w_proj");
  if (m == 0) return PTV3_OK;
  if (!ptv3_res_conv_capable(m, ca, cb, cout, kvol)) {
    set_error("res_conv: m=%lld ca=%d cb=%d cout=%d is not served (ca + cb <= %d, cout <= %d)", (long long)m, ca, cb,
              cout, RC_MAX_CIN, RC_MAX_COUT);
    return PTV3_ERR_UNSUPPORTED;
  }
  ResConvArgs a{xa, xb, w, w_proj, nbr, row_order, bn_scale, bn_shift, res, proj_scale, proj_shift, out, proj_out,
                m, ca, cb, cout, act};
  hipStream_t s = (hipStream_t)stream;
  by_value<1, 2, 4, 6, 8>(rc_nt(cout), [&](auto NT) { launch_nt<NT()>(a, s); });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
