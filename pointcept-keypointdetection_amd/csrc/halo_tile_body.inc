// The halo tile body: what conv_halo_kernel (gemm.hip) does up to and including the barrier after its tap loop.
// Included as text at the top of a __global__ function template <typename T, int C> of 256 threads whose parameters are
// `GemmArgs a, HaloArgs h` (halo_tile.h) - conv_halo_kernel and conv_head_halo_kernel (conv_head.hip) - so that both
// compile the very same statements and conv_halo_kernel's code stays what it was before the second kernel existed (as
// an inlined function the body came out with another block layout and register assignment).
// Declares the workgroup's dynamic LDS hc_smem[HaloShape<T, C>::LDS] and leaves in scope: F, FR, S, E, MI, NJ, tid,
// lane, wave, li, g, tile, row0, sEpi (the parked epilogue vectors) and acc[m][j] = channels 16 j + 4 g .. + 3 of site
// 32 wave + 16 m + li of the tile, before bias.  Behind it everything in hc_smem but sEpi is dead.
  typedef Frag<T> F;
  typedef typename F::type FR;
  typedef HaloShape<T, C> S;
  constexpr int E = F::E;
  constexpr int RB = S::RB, CPR = RB / 16;                // 16-byte chunks per row: 4 | 8 | 16
  constexpr int KQ = C / F::KC;                           // matrix-core K chunks per tap
  constexpr int MI = 2, NJ = C / 16;                      // accumulator fragments per wave: sites x channels
  constexpr int TPS = S::TPS, NSTG = S::NSTG;
  constexpr int WCH = C * CPR;                            // chunks of a weight tap
  constexpr int W_LOADS = TPS * WCH / 256;                // chunks per thread and stage: 1 | 2 | 4
  constexpr int RING = 3;                                 // weight stages in flight in registers
  constexpr int RPP = 256 / CPR;                          // halo rows per pass of the workgroup
  constexpr int G_LOADS = HALO_T / RPP;                   // slow path: chunks per thread of the 128 gathered rows
  constexpr int NP = (HALO_CAP + RPP - 1) / RPP;          // passes that cover the whole row list: 7 | 14 | 27
  constexpr int FB = NP > 14 ? 14 : NP;                   // passes in flight: 14 x 16 bytes of registers per thread
  constexpr int NB = (NP + FB - 1) / FB;                  // batches: 1 | 2
  static_assert(HALO_T * RB + HALO_T * HALO_TAPS * 4 <= (HALO_CAP + 1) * RB, "slow path: rows 0..127 + the table fit the halo image");
  static_assert(TPS * WCH % 256 == 0, "a weight stage is a whole number of chunks per thread");
  extern __shared__ __attribute__((aligned(16))) char hc_smem[];
  char* sHalo = hc_smem;
  char* sW = sHalo + S::HALO;
  unsigned short* sSlot = reinterpret_cast<unsigned short*>(sW + 2 * S::WBUF);
  float* sEpi = reinterpret_cast<float*>(sW + 2 * S::WBUF + S::SLOT);

  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ w = reinterpret_cast<const T*>(a.w);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  // consecutive tiles (neighbours in Morton order: they share halo rows) on one XCD, behind one L2
  const int64_t tile = xcd_remap(blockIdx.x, gridDim.x), row0 = tile * HALO_T;
  // the tile's row list is fetched beside its count: all NP passes of ids (entries past the count were never written
  // and are not used)
  int id[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) id[u] = h.rows[tile * HALO_CAP + min(tid / CPR + RPP * u, HALO_CAP - 1)];
  const int cnt = h.count[tile];
  const bool fast = cnt <= HALO_CAP;                      // workgroup-uniform
  // 64-byte rows: four rows per 256-byte bank row, chunk g ^ [0, 3, 2, 1][row quarter] (see conv_tile_kernel);
  // 128 / 256-byte rows: two / one row per bank row
  auto swz = [](int r) { return CPR == 4 ? ((0 - (r >> 2)) & 3) : CPR == 8 ? ((r >> 1) & 7) : (r & 15); };
  auto chunk_at = [&](char* img, int r, int c) { return reinterpret_cast<FR*>(img + r * RB + 16 * (c ^ swz(r))); };
  auto frag_at = [&](const char* img, int r, int q) {
    return *reinterpret_cast<const FR*>(img + r * RB + 16 * ((4 * q + g) ^ swz(r)));
  };

  park_epi(a, sEpi, C, 0, tid, 256);
  // weight stage s = taps TPS s .. TPS s + TPS - 1: chunk e -> (tap e / WCH, channel row (e % WCH) / CPR, chunk e % CPR);
  // the tap the last stage of an odd count lacks is fetched as tap 26 once more and never used
  int w_t[W_LOADS], w_o[W_LOADS], w_c[W_LOADS];
#pragma unroll
  for (int u = 0; u < W_LOADS; ++u) {
    const int e = tid + 256 * u;
    w_t[u] = e / WCH;
    w_o[u] = (e % WCH) / CPR;
    w_c[u] = e % CPR;
  }
  auto issue_w = [&](int stage, FR (&rw)[W_LOADS]) {
#pragma unroll
    for (int u = 0; u < W_LOADS; ++u) {
      const int d = min(stage * TPS + w_t[u], HALO_TAPS - 1);
      rw[u] = *reinterpret_cast<const FR*>(w + ((int64_t)w_o[u] * HALO_TAPS + d) * C + E * w_c[u]);
    }
  };
  auto stash_w = [&](int buf, const FR (&rw)[W_LOADS]) {
#pragma unroll
    for (int u = 0; u < W_LOADS; ++u) *chunk_at(sW + buf * S::WBUF + w_t[u] * (C * RB), w_o[u], w_c[u]) = rw[u];
  };

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int m = 0; m < MI; ++m)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tid < CPR) *reinterpret_cast<FR*>(sHalo + HALO_CAP * RB + 16 * tid) = F::zero();
  if (fast) {
    FR rw[RING][W_LOADS];
    issue_w(0, rw[0]);
    issue_w(1, rw[1]);
    issue_w(2, rw[2]);
    {
      // the tile's slot table: 432 chunks of eight 16-bit slots, "absent" turned into the zero row
      const s16x8* src = reinterpret_cast<const s16x8*>(h.slots + tile * (HALO_T * HALO_TAPS));
      constexpr int NCH = S::SLOT / 16;
      s16x8 v[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) v[u] = src[min(tid + 256 * u, NCH - 1)];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if ((unsigned short)v[u][i] == (unsigned short)HALO_ABSENT) v[u][i] = (short)HALO_CAP;
        if (tid + 256 * u < NCH) reinterpret_cast<s16x8*>(sSlot)[tid + 256 * u] = v[u];
      }
    }
    // the halo: rows 0..cnt-1 of the tile's list.  FB passes of the workgroup are in flight together - every id of the
    // list, then every row, then LDS: two round trips per tile where a pass-by-pass loop paid two per pass.  A pass
    // beyond the count reads row 0 again (never written to LDS).
    const int fr = tid / CPR, fc = tid % CPR;
    static_for<0, NB>([&](auto bc) {
      constexpr int b = decltype(bc)::value;
      if (b * FB * RPP < cnt) {                             // workgroup-uniform
        FR v[FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) {
          const int r = fr + RPP * (b * FB + u);
          const int src = (b * FB + u < NP && r < cnt) ? id[b * FB + u < NP ? b * FB + u : 0] : 0;
          v[u] = *reinterpret_cast<const FR*>(x + (int64_t)src * C + E * fc);
        }
#pragma unroll
        for (int u = 0; u < FB; ++u) {
          const int r = fr + RPP * (b * FB + u);
          if (r < cnt) *chunk_at(sHalo, r, fc) = v[u];
        }
      }
    });
    stash_w(0, rw[0]);
    issue_w(3, rw[0]);
    __syncthreads();
    // Stage s: weight stage s+1 (in registers since stage s-2) goes to the idle buffer and its register set takes
    // stage s+4; the A fragments of stage s were read from the halo during stage s-1 and its slots during stage s-2,
    // so only the weight fragments stand between the barrier and the matrix core.  Fully unrolled: every register set
    // is named statically and the waits in front of the LDS writes count only their own loads.
    const unsigned short* my_slots = sSlot + (32 * wave + li) * HALO_TAPS;
    int sl[2][TPS][MI];
    FR xf[2][TPS][KQ][MI];
    auto read_slots = [&](int stage, int (&o)[TPS][MI]) {
#pragma unroll
      for (int t = 0; t < TPS; ++t)
#pragma unroll
        for (int m = 0; m < MI; ++m) o[t][m] = my_slots[16 * m * HALO_TAPS + min(stage * TPS + t, HALO_TAPS - 1)];
    };
    auto read_x = [&](const int (&sv)[TPS][MI], FR (&o)[TPS][KQ][MI]) {
#pragma unroll
      for (int t = 0; t < TPS; ++t)
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
          for (int m = 0; m < MI; ++m) o[t][q][m] = frag_at(sHalo, sv[t][m], q);
    };
    read_slots(0, sl[0]);
    read_x(sl[0], xf[0]);
    read_slots(1, sl[1]);
    static_for<0, NSTG>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if constexpr (s + 1 < NSTG) stash_w((s + 1) & 1, rw[(s + 1) % RING]);
      if constexpr (s + 4 < NSTG) issue_w(s + 4, rw[(s + 1) % RING]);
      const char* bw = sW + (s & 1) * S::WBUF;
      FR wf[TPS][KQ][NJ];
#pragma unroll
      for (int t = 0; t < TPS; ++t)
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
          for (int j = 0; j < NJ; ++j) wf[t][q][j] = frag_at(bw + t * (C * RB), 16 * j + li, q);
      if constexpr (s + 1 < NSTG) read_x(sl[(s + 1) & 1], xf[(s + 1) & 1]);
      if constexpr (s + 2 < NSTG) read_slots(s + 2, sl[s & 1]);
#pragma unroll
      for (int t = 0; t < TPS; ++t) {
        if (s * TPS + t >= HALO_TAPS) continue;             // compile-time after unrolling
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
          for (int m = 0; m < MI; ++m)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              acc[m][j] = F::mma(wf[t][q][j], xf[s & 1][t][q][m], acc[m][j]);   // D[channel 4g+r][site li]
      }
      __syncthreads();
    });
  } else {
    // overflowing tile: per tap, the neighbour rows of the 128 sites are gathered into rows 0..127 of the halo image
    // and read back with slot = site.  The tile's table sits in LDS behind those rows (no dependent index read per
    // tap) and the rows of tap d+1 are fetched while tap d computes.
    int32_t* sNbr = reinterpret_cast<int32_t*>(sHalo + HALO_T * RB);         // [128][27]
    {
      constexpr int PER = (HALO_T * HALO_TAPS + 255) / 256;
      int64_t orow[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int64_t r = row0 + (tid + 256 * u) / HALO_TAPS;
        const int64_t rs = r < a.m ? r : 0;
        orow[u] = a.row_order ? (int64_t)a.row_order[rs] : rs;
      }
      int32_t nv[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) nv[u] = a.nbr[orow[u] * HALO_TAPS + (tid + 256 * u) % HALO_TAPS];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int e = tid + 256 * u;
        if (e < HALO_T * HALO_TAPS) sNbr[e] = row0 + e / HALO_TAPS < a.m ? nv[u] : -1;
      }
    }
    __syncthreads();
    const int gr = tid / CPR, gc = tid % CPR;
    FR rw[W_LOADS];
    int32_t nb[G_LOADS];
    FR v[G_LOADS];
    auto fetch = [&](int d) {
#pragma unroll
      for (int u = 0; u < G_LOADS; ++u) nb[u] = sNbr[(gr + RPP * u) * HALO_TAPS + d];
#pragma unroll
      for (int u = 0; u < G_LOADS; ++u) v[u] = *reinterpret_cast<const FR*>(x + (int64_t)(nb[u] >= 0 ? nb[u] : 0) * C + E * gc);
    };
    issue_w(0, rw);
    fetch(0);
    for (int d = 0; d < HALO_TAPS; ++d) {
      const int t = d % TPS;
      __syncthreads();                                      // the readers of the previous tap are done
#pragma unroll
      for (int u = 0; u < G_LOADS; ++u) *chunk_at(sHalo, gr + RPP * u, gc) = nb[u] >= 0 ? v[u] : F::zero();
      if (t == 0) stash_w(0, rw);
      __syncthreads();
      if (d + 1 < HALO_TAPS) {
        fetch(d + 1);
        if ((d + 1) % TPS == 0) issue_w((d + 1) / TPS, rw);
      }
      const char* bw = sW + t * (C * RB);
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        FR xs[MI], ws[NJ];
#pragma unroll
        for (int m = 0; m < MI; ++m) xs[m] = frag_at(sHalo, 32 * wave + 16 * m + li, q);
#pragma unroll
        for (int j = 0; j < NJ; ++j) ws[j] = frag_at(bw, 16 * j + li, q);
#pragma unroll
        for (int m = 0; m < MI; ++m)
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[m][j] = F::mma(ws[j], xs[m], acc[m][j]);
      }
    }
    __syncthreads();
  }
