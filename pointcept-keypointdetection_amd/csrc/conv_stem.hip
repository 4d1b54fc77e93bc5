// The stem's k^3 submanifold convolution (k = 5; 3 for tests) straight from the table of 4 x 4 x 4 blocks: no (n, k^3)
// neighbour table exists in memory.  A workgroup takes 64 sites, resolves their up-to-8 candidate blocks once, fills the
// tile's 64 x k^3 neighbour rows into LDS (32 000 bytes at 125 taps) with the rules of bt_neighbors_kernel (block_taps.h)
// and then runs the K loop of gemm_kernel<T, NT, GATHER = true> (gemm.hip): the same K order, LDS staging, matrix-core
// chain and epilogue, so the output is byte-equal to ptv3_gemm over the table of ptv3_subm_neighbors_blocks.  That
// includes the shapes ptv3_gemm splits over K: the K ranges of its slabs are accumulated apart and summed in slab order.
// With the rows in LDS a K stage has no dependent global read, where the table form at 125 taps fetched the neighbour
// index from memory in every stage.
#include "common.h"
#include "profile.h"
#include "halo_tile.h"
#include "block_taps.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

constexpr int ST_THREADS = 256;
constexpr int ST_BM = 64;   // sites per workgroup (4 waves x 16)
// K steps fetched ahead into a register ring.  With no dependent read in a stage the depth hardly matters: 54.1 / 53.8 us
// at depth 1 / 2 on the 100k-site scene in bf16 (67.5 of 2 ahead of 68.1 of 1 and 69.7 of 4 with the first form of the
// table fill; profiles/stem_blocks/stem_kernel_alone.txt)
constexpr int ST_PD = 2;

struct StemArgs {
  const int32_t* indices; const BlockSlot* slots; uint64_t smask; const uint32_t* payload;
  int splits;   // K slabs ptv3_gemm would sum for this shape (1: single pass)
};

template <typename T, int NT, int K, int PD>
__global__ void __launch_bounds__(ST_THREADS) stem_conv_kernel(GemmArgs a, StemArgs g) {
  constexpr int BN = 16 * NT;
  constexpr int KVOL = K * K * K, H = K / 2;
  typedef Frag<T> F;
  typedef typename F::type FR;
  constexpr int E = F::E;
  constexpr int BK = 2 * F::KC;
  constexpr int LS = BK + E;
  constexpr int CPR = BK / E;
  constexpr int A_LOADS = (ST_BM * CPR) / ST_THREADS;
  constexpr int B_LOADS = (BN * CPR) / ST_THREADS;
  constexpr int OS = BN + 16 / (int)sizeof(T);
  constexpr int SM_OPER = (ST_BM + BN) * LS, SM_OUT = ST_BM * OS;
  constexpr int SM_ALL = SM_OPER > SM_OUT ? SM_OPER : SM_OUT;
  constexpr int NCAND = ST_BM * BT_NC;               // 512 block lookups per tile, two per thread
  constexpr int CAND_PER = NCAND / ST_THREADS;
  constexpr int ENT = ST_BM * KVOL;
  constexpr int LINES = ST_BM * K * K, LIT = (LINES + ST_THREADS - 1) / ST_THREADS;   // lines of K taps along z
  __shared__ __attribute__((aligned(16))) T smem_all[SM_ALL];
  __shared__ __attribute__((aligned(16))) float sEpi[3 * BN];
  __shared__ int32_t sNbr[ENT];
  __shared__ int32_t sRow[ST_BM];   // the tile's output rows, -1 past the end
  // the lookup results live in the operand buffers, which the K loop fills only after the table is complete
  static_assert(NCAND * 12 + ST_BM * 16 <= SM_ALL * (int)sizeof(T), "candidate staging overlays the operand tiles");
  unsigned long long* s_mask = reinterpret_cast<unsigned long long*>(smem_all);
  int4* s_site = reinterpret_cast<int4*>(s_mask + NCAND);
  int32_t* s_base = reinterpret_cast<int32_t*>(s_site + ST_BM);

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ w = reinterpret_cast<const T*>(a.w);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g4 = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * ST_BM;
  const int n0 = blockIdx.y * BN;
  const int ktot = KVOL * a.cin;
  const int nsteps = (ktot + BK - 1) / BK;
  // K steps per slab: ptv3_gemm's split rule ends on splits = ceil(nsteps / sps), and its sps is the least such value
  const int sps = g.splits > 1 ? (nsteps + g.splits - 1) / g.splits : nsteps;

  int a_r[A_LOADS], a_ch[A_LOADS];
#pragma unroll
  for (int u = 0; u < A_LOADS; ++u) {
    const int e = tid * A_LOADS + u;
    a_r[u] = e / CPR;
    a_ch[u] = e % CPR;
  }
  int b_r[B_LOADS], b_ch[B_LOADS];
#pragma unroll
  for (int u = 0; u < B_LOADS; ++u) {
    const int e = tid * B_LOADS + u;
    b_r[u] = e / CPR;
    b_ch[u] = e % CPR;
  }
  park_epi(a, sEpi, BN, n0, tid, ST_THREADS);

  // ---- lookup: candidate c = 8 * site + block; the first probes of a thread's candidates are issued together and
  // unconditionally (a dead candidate reads slot 0), only a first slot that holds another block's key probes on
  {
    int4 p[CAND_PER];
    int64_t orow[CAND_PER];
    bool in[CAND_PER];
#pragma unroll
    for (int u = 0; u < CAND_PER; ++u) {
      const int64_t r = row0 + ((tid + u * ST_THREADS) >> 3);
      in[u] = r < a.m;
      orow[u] = in[u] ? (a.row_order ? (int64_t)a.row_order[r] : r) : 0;
    }
#pragma unroll
    for (int u = 0; u < CAND_PER; ++u) p[u] = reinterpret_cast<const int4*>(g.indices)[orow[u]];
    uint64_t key[CAND_PER], slot[CAND_PER];
    bool live[CAND_PER];
    unsigned long long k0[CAND_PER], m0[CAND_PER];
    int32_t b0[CAND_PER];
#pragma unroll
    for (int u = 0; u < CAND_PER; ++u) {
      live[u] = bt_candidate(p[u], H, (tid + u * ST_THREADS) & 7, g.smask, key[u], slot[u]) && in[u];
      k0[u] = g.slots[slot[u]].key;
      m0[u] = g.slots[slot[u]].mask;
      b0[u] = g.slots[slot[u]].base;
    }
#pragma unroll
    for (int u = 0; u < CAND_PER; ++u) {
      const int c = tid + u * ST_THREADS;
      unsigned long long m = 0;
      int32_t base = 0;
      if (live[u]) {
        if (k0[u] == key[u]) { m = m0[u]; base = b0[u]; }
        else if (k0[u] != 0) bt_probe_on(g.slots, g.smask, key[u], slot[u], m, base);
      }
      s_mask[c] = m;
      s_base[c] = base;
      if ((c & 7) == 0) { s_site[c >> 3] = p[u]; sRow[c >> 3] = in[u] ? (int32_t)orow[u] : -1; }
    }
  }
  __syncthreads();
  // ---- the tile's table, a line of K taps along z per item: item = K^2 site + K dx + dy.  The line lies in the two
  // candidates (cxy, 0) and (cxy, 1); per candidate one 64-bit shift gives the four voxels of the line's row in that
  // block and one 64-bit popcount the rank in front of them, a tap is then a bit test and a popcount in eight bits.
  // A tap outside the coordinate range falls into a dead candidate (mask 0).  All payload reads of a thread are in
  // flight together; an absent tap reads payload[0].  A present tap's index is base + rank of a slot whose key matched
  // and whose bit is set, below the number of sites by the invariant of bt_payload_kernel; the clamp keeps the read
  // inside the payload for any table.
  {
    uint32_t v[LIT][K];
    unsigned has[LIT];
#pragma unroll
    for (int it = 0; it < LIT; ++it) {
      const int item = min(tid + it * ST_THREADS, LINES - 1);
      const int s = item / (K * K), l = item - s * (K * K);
      BtLine ln;
      bt_line(s_site[s], H, l / K, l % K, s_mask + s * BT_NC, s_base + s * BT_NC, ln);
      has[it] = 0;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        int rank;
        const bool hit = bt_line_tap(ln, i, rank);
        const int64_t at = hit ? (rank < 0 ? 0 : (rank < a.m ? (int64_t)rank : a.m - 1)) : 0;
        has[it] |= (unsigned)hit << i;
        v[it][i] = g.payload[at];
      }
    }
#pragma unroll
    for (int it = 0; it < LIT; ++it) {
      const int item = tid + it * ST_THREADS;
      const int ic = min(item, LINES - 1);
      const int s = ic / (K * K), l = ic - s * (K * K);
      const int32_t self = sRow[s];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        int32_t nb = ((has[it] >> i) & 1) ? (int32_t)~v[it][i] : -1;
        if (l == (K * K) / 2 && i == H) nb = self;   // the centre tap is the site itself, also among duplicate coordinates
        if (self < 0) nb = -1;
        if (item < LINES) sNbr[ic * K + i] = nb;
      }
    }
  }
  __syncthreads();

  // ---- K loop of gemm_kernel: every load of a stage is issued unconditionally (a missing neighbour, a channel or K
  // index past the end read a valid dummy address and are zeroed on the way to LDS)
  FR rra[PD][A_LOADS], rrb[PD][B_LOADS];
  unsigned rok[PD];
  auto issue = [&](int step, FR (&ra)[A_LOADS], FR (&rb)[B_LOADS], unsigned& ok) {
    const int k0 = step * BK;
    ok = 0;
    int64_t src[A_LOADS];
    int cc[A_LOADS];
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) {
      const int kk = k0 + E * a_ch[u];
      const bool in = kk < ktot;
      const int kks = in ? kk : 0;
      const int d = a.cin_shift >= 0 ? (kks >> a.cin_shift) : (kks / a.cin);
      cc[u] = kks - d * a.cin;
      src[u] = (int64_t)sNbr[a_r[u] * KVOL + d];
      const bool v = in && src[u] >= 0;
      ok |= (unsigned)v << u;
      if (!v) src[u] = 0;
    }
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) ra[u] = *reinterpret_cast<const FR*>(x + src[u] * a.cin + cc[u]);
#pragma unroll
    for (int u = 0; u < B_LOADS; ++u) {
      const int kk = k0 + E * b_ch[u];
      const int o = n0 + b_r[u];
      const bool v = o < a.cout && kk < ktot;
      ok |= (unsigned)v << (8 + u);
      rb[u] = *reinterpret_cast<const FR*>(w + (int64_t)(v ? o : 0) * ktot + (v ? kk : 0));
    }
  };
  auto stash = [&](const FR (&ra)[A_LOADS], const FR (&rb)[B_LOADS], unsigned ok) {
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u)
      *reinterpret_cast<FR*>(smem_all + a_r[u] * LS + E * a_ch[u]) = ((ok >> u) & 1u) ? ra[u] : F::zero();
#pragma unroll
    for (int u = 0; u < B_LOADS; ++u)
      *reinterpret_cast<FR*>(smem_all + (ST_BM + b_r[u]) * LS + E * b_ch[u]) = ((ok >> (8 + u)) & 1u) ? rb[u] : F::zero();
  };
  const T* sA = smem_all;
  const T* sB = smem_all + ST_BM * LS;

  // acc: the running K range; tot: the sum of the finished ranges in slab order (the split-K reduce of ptv3_gemm starts
  // from 0.0f and adds slab after slab)
  f32x4 acc[NT], tot[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) { acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; tot[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }

#pragma unroll
  for (int p = 0; p < PD; ++p)
    if (p < nsteps) issue(p, rra[p], rrb[p], rok[p]);
  int left = sps;   // steps until the running range ends
  for (int base = 0; base < nsteps; base += PD) {
#pragma unroll
    for (int p = 0; p < PD; ++p) {
      const int step = base + p;
      if (step >= nsteps) break;   // workgroup-uniform
      stash(rra[p], rrb[p], rok[p]);
      __syncthreads();
      if (step + PD < nsteps) issue(step + PD, rra[p], rrb[p], rok[p]);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        FR xf = *reinterpret_cast<const FR*>(sA + (16 * wave + li) * LS + F::KC * ks + E * g4);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          FR wf = *reinterpret_cast<const FR*>(sB + (16 * j + li) * LS + F::KC * ks + E * g4);
          acc[j] = F::mma(wf, xf, acc[j]);  // D[channel 4g+r][point li]
        }
      }
      if (g.splits > 1 && (--left == 0 || step == nsteps - 1)) {
#pragma unroll
        for (int j = 0; j < NT; ++j) { tot[j] += acc[j]; acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        left = sps;
      }
      __syncthreads();
    }
  }
  if (g.splits > 1) {
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = tot[j];
  }

  // ---- epilogue: lane owns point (16*wave + li), channels n0 + 16j + 4g .. +3
  typedef typename Vec4<T>::type V4;
  constexpr int N = 16 / (int)sizeof(T);   // elements of a 16-byte chunk
  T* out = reinterpret_cast<T*>(a.out);
  if ((a.cout % N) == 0) {
    // whole rows of the tile through LDS (the operand tiles are dead: the K loop ended on a barrier), then row
    // segments of 16 bytes per lane
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const EpiVec ev = load_epi(sEpi, BN, 16 * j + 4 * g4);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = epi_value(acc[j][r], ev, r, a.act);
      *reinterpret_cast<V4*>(smem_all + (size_t)(16 * wave + li) * OS + 16 * j + 4 * g4) = pack4<T>(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    constexpr int cpr = BN / N, total = ST_BM * cpr;
#pragma unroll
    for (int e = tid; e < total; e += ST_THREADS) {
      const int rl = e / cpr, col = n0 + (e - rl * cpr) * N;
      const int32_t orow = sRow[rl];
      if (orow >= 0 && col < a.cout)
        *reinterpret_cast<FR*>(out + (int64_t)orow * a.cout + col) = *reinterpret_cast<const FR*>(smem_all + (size_t)rl * OS + (col - n0));
    }
    return;
  }
  const int32_t orow = sRow[16 * wave + li];
  if (orow < 0) return;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int ch0 = n0 + 16 * j + 4 * g4;
    const EpiVec ev = load_epi(sEpi, BN, 16 * j + 4 * g4);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ch0 + r < a.cout) out[(int64_t)orow * a.cout + ch0 + r] = from_f32<T>(epi_value(acc[j][r], ev, r, a.act));
  }
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int ptv3_stem_conv_blocks(const void* x, const void* w, void* out, int64_t n, int cin, int cout, int ksize,
                                     const int32_t* indices, const void* table, size_t table_bytes,
                                     const int32_t* row_order, const float* bias, const float* bn_scale,
                                     const float* bn_shift, int act, int dtype, void* stream) {
  PTV3_REQUIRE(dtype == PTV3_F32 || dtype == PTV3_BF16, "stem_conv_blocks: bad dtype %d", dtype);
  const int gran = dtype_granule(dtype);
  PTV3_REQUIRE(cin > 0 && cin % gran == 0, "stem_conv_blocks: cin=%d must be a positive multiple of %d for this dtype", cin, gran);
  PTV3_REQUIRE(cout > 0, "stem_conv_blocks: cout=%d", cout);
  PTV3_REQUIRE(ksize == 3 || ksize == 5, "stem_conv_blocks: ksize %d must be 3 or 5", ksize);
  PTV3_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "stem_conv_blocks: bn_scale/bn_shift must come together");
  PTV3_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "stem_conv_blocks: n=%lld out of range", (long long)n);
  if (n == 0) return PTV3_OK;
  PTV3_REQUIRE(x && w && out && indices, "stem_conv_blocks: x, w, out and indices are required");
  PTV3_REQUIRE(table && table_bytes >= ptv3_subm_block_table_bytes(n) && ((uintptr_t)table & 15) == 0 &&
                   ((uintptr_t)indices & 15) == 0,
               "stem_conv_blocks: table must be the one ptv3_subm_build_block_table built for these n sites");
  const int kvol = ksize * ksize * ksize;
  int cin_shift = -1;
  if ((cin & (cin - 1)) == 0) { cin_shift = 0; while ((1 << cin_shift) < cin) ++cin_shift; }
  GemmArgs a{x, w, out, nullptr, nullptr, nullptr, row_order, nullptr, bias, bn_scale, bn_shift, nullptr,
             n, cin, cout, kvol, act, cin_shift, 0, 0, 0};
  // the table's layout as sparse.hip lays it out: S block slots, then the payload of n rows.  The split count is the
  // one ptv3_gemm's policy gives the shape when it has its workspace (the executor and ops.gemm always hand it one); the
  // environment switches with which tests and tools force a tile or a single pass there do not reach this kernel
  const int64_t S = ptv3_subm_table_slots(n);
  StemArgs g{indices, (const BlockSlot*)table, (uint64_t)(S - 1),
             (const uint32_t*)((const char*)table + (size_t)S * sizeof(BlockSlot)),
             ptv3_gemm_splits(n, cin, cout, kvol, dtype)};
  hipStream_t s = (hipStream_t)stream;
  const int nt = cout <= 32 ? 2 : 4;
  const int esz = dtype_bytes(dtype);
  // flops of a full neighbourhood: the taps that exist are not counted anywhere without a table
  const int prof = prof_begin(s, PROF_SUBM_CONV, 2.0 * n * kvol * cin * cout,
                              ((double)n * cin + (double)cout * kvol * cin + (double)n * cout) * esz, nullptr, 0, 0.0);
  prof_kernel(prof, nt == 2 ? PK_GEMM32_CONV : PK_GEMM64_CONV);
  const dim3 grid((unsigned)cdiv(n, ST_BM), (unsigned)cdiv(cout, 16 * nt)), block(ST_THREADS);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_value<2, 4>(nt, [&](auto NT) {
      by_value<3, 5>(ksize, [&](auto K) {
        hipLaunchKernelGGL((stem_conv_kernel<T, NT(), K(), ST_PD>), grid, block, 0, s, a, g);
      });
    });
  });
  prof_end(prof, s);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
