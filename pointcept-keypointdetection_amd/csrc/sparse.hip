// Active-site hash table and neighbour table ("rulebook") for the submanifold convolutions.
// Replaces spconv's indice-pair generation (called lazily per indice_key by SubMConv3d in
// point_transformer_v3m1_base.py:277-284,499-506 on the tensor built in structure.py:111-146).
#include <stdlib.h>
#include "common.h"
#include "hashtable.h"
#include "halo_plan.h"
#include "../../include/ptv3_hip.h"

namespace ptv3 {

__global__ void ht_insert_kernel(const int32_t* __restrict__ idx, int64_t n, unsigned long long* keys,
                                 int32_t* vals, uint64_t mask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t key = site_key(idx[4 * i], idx[4 * i + 1], idx[4 * i + 2], idx[4 * i + 3]);
  uint64_t slot = mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    unsigned long long prev = atomicCAS(&keys[slot], (unsigned long long)HT_EMPTY, (unsigned long long)key);
    if (prev == HT_EMPTY || prev == key) {
      // duplicates (not produced by GridSample) keep the smallest point index deterministically
      atomicMin(&vals[slot], (int32_t)i);  // vals start at 0x7F7F7F7F
      return;
    }
    slot = (slot + 1) & mask;
  }
}

__global__ void ht_neighbors_kernel(const int32_t* __restrict__ idx, int64_t n,
                                    const unsigned long long* __restrict__ keys,
                                    const int32_t* __restrict__ vals, uint64_t mask, int ksize, int kvol,
                                    int32_t* __restrict__ nbr) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kvol) return;
  int64_t i = t / kvol;
  int d = (int)(t - i * kvol);
  int c = d % ksize, b_ = (d / ksize) % ksize, a = d / (ksize * ksize);
  int half = ksize / 2;
  int x = idx[4 * i + 1] + a - half, y = idx[4 * i + 2] + b_ - half, z = idx[4 * i + 3] + c - half;
  int32_t found = -1;
  if (d == kvol / 2) {
    found = (int32_t)i;  // the centre tap is the site itself
  } else if (x >= 0 && y >= 0 && z >= 0 && x < 65536 && y < 65536 && z < 65536) {
    uint64_t key = site_key(idx[4 * i], x, y, z);
    uint64_t slot = mix64(key) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe) {
      unsigned long long kq = keys[slot];
      if (kq == key) { found = vals[slot]; break; }
      if (kq == HT_EMPTY) break;
      slot = (slot + 1) & mask;
    }
  }
  nbr[t] = found;
}

// The neighbour relation of a submanifold convolution is symmetric: j = nbr[i][d]  <=>  i = nbr[j][kvol - 1 - d] (the
// mirrored offset).  Half the taps are probed; a hit fills both entries, the table is pre-filled with -1.  125 probes per
// site at the 5^3 stem are the longest item in front of a forward's first feature kernel (133 us at 100k sites).
__global__ void ht_neighbors_half_kernel(const int32_t* __restrict__ idx, int64_t n,
                                         const unsigned long long* __restrict__ keys, const int32_t* __restrict__ vals,
                                         uint64_t mask, int ksize, int kvol, int slots_log2,
                                         int32_t* __restrict__ nbr) {
  // a workgroup is 256 >> slots_log2 sites x 2^slots_log2 tap slots (>= kvol / 2 + 1): site and tap by shifts - the
  // flat index of the full-probing kernel costs a 64-bit division per thread, more than its probe
  const int hv = kvol / 2 + 1;
  const int64_t i = (int64_t)blockIdx.x * (256 >> slots_log2) + (threadIdx.x >> slots_log2);
  const int d = threadIdx.x & ((1 << slots_log2) - 1);
  if (i >= n || d >= hv) return;
  if (d == kvol / 2) { nbr[i * kvol + d] = (int32_t)i; return; }   // the centre tap is the site itself
  int c = d % ksize, b_ = (d / ksize) % ksize, a = d / (ksize * ksize);
  int half = ksize / 2;
  int x = idx[4 * i + 1] + a - half, y = idx[4 * i + 2] + b_ - half, z = idx[4 * i + 3] + c - half;
  if (!(x >= 0 && y >= 0 && z >= 0 && x < 65536 && y < 65536 && z < 65536)) return;
  uint64_t key = site_key(idx[4 * i], x, y, z);
  uint64_t slot = mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    unsigned long long kq = keys[slot];
    if (kq == key) {
      const int32_t j = vals[slot];
      nbr[i * kvol + d] = j;
      nbr[(int64_t)j * kvol + (kvol - 1 - d)] = (int32_t)i;
      return;
    }
    if (kq == HT_EMPTY) return;
    slot = (slot + 1) & mask;
  }
}

// ---- neighbour tables from a table of 4 x 4 x 4 blocks (hashtable.h) ---------------------------------------------
// The per-voxel probes above cost one 128-byte line per probed voxel (89 distinct lines per site at 5^3 on the 100k
// surface scene); a k^3 neighbourhood with k <= 5 lies in at most 8 blocks, whose slot and payload lines serve all of
// its taps (16 lines per site on the same scene).  Table memory of n sites, S = ptv3_subm_table_slots(n):
//   S x BlockSlot | payload: n x uint32 | counter (16 bytes) | site_slot: n x int32
// payload holds ~row (0 = never written, every ~row has bit 31 set), so one zero fill initialises slots, payload and
// counter, and "smallest row wins" among duplicate coordinates is an atomicMax.
struct BlockTable {
  BlockSlot* slots; uint32_t* payload; int32_t* counter; int32_t* site_slot; uint64_t smask; size_t zero_bytes;
};
static inline size_t bt_payload_bytes(int64_t n) { return ((size_t)n * 4 + 15) & ~(size_t)15; }
static inline BlockTable bt_layout(void* table, int64_t n) {
  const int64_t S = ptv3_subm_table_slots(n);
  char* p = (char*)table;
  BlockTable t;
  t.slots = (BlockSlot*)p;
  t.payload = (uint32_t*)(p + (size_t)S * sizeof(BlockSlot));
  t.counter = (int32_t*)((char*)t.payload + bt_payload_bytes(n));
  t.site_slot = (int32_t*)((char*)t.counter + 16);
  t.smask = (uint64_t)(S - 1);
  t.zero_bytes = (size_t)S * sizeof(BlockSlot) + bt_payload_bytes(n) + 16;
  return t;
}

// sites (batch, x, y, z) as int32 from the batch ids and (n, 3) coordinates, the coordinates once more as int64 when
// grid64 is given, and the zero fill of the block table that will be built over these sites (zero16 x 16 bytes,
// grid-stride): one launch where a conversion kernel and a memset stood in front of bt_claim_kernel
__global__ void bt_sites_kernel(const int64_t* __restrict__ batch, const void* __restrict__ grid, int is_i64, int64_t n,
                                int32_t* __restrict__ idx, int64_t* __restrict__ grid64, uint4* __restrict__ zero,
                                int64_t zero16) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t j = i; j < zero16; j += (int64_t)gridDim.x * blockDim.x) zero[j] = uint4{0u, 0u, 0u, 0u};
  if (i >= n) return;
  int64_t x, y, z;
  if (is_i64) {
    const int64_t* g = (const int64_t*)grid;
    x = g[3 * i]; y = g[3 * i + 1]; z = g[3 * i + 2];
  } else {
    const int32_t* g = (const int32_t*)grid;
    x = g[3 * i]; y = g[3 * i + 1]; z = g[3 * i + 2];
  }
  reinterpret_cast<int4*>(idx)[i] = int4{(int32_t)batch[i], (int32_t)x, (int32_t)y, (int32_t)z};
  if (grid64) { grid64[3 * i] = x; grid64[3 * i + 1] = y; grid64[3 * i + 2] = z; }
}

// every site claims its block's slot and sets its voxel's bit; the slot is kept for bt_payload_kernel
__global__ void bt_claim_kernel(const int32_t* __restrict__ idx, int64_t n, BlockSlot* slots, uint64_t smask,
                                int32_t* __restrict__ site_slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 s = reinterpret_cast<const int4*>(idx)[i];
  const uint64_t key = block_key(s.x, s.y >> 2, s.z >> 2, s.w >> 2);
  uint64_t slot = mix64(key) & smask;
  int32_t mine = -1;                       // stays -1 only if the table were full (slots >= 2n: it never is)
  for (uint64_t probe = 0; probe <= smask; ++probe) {
    const unsigned long long prev = atomicCAS(&slots[slot].key, 0ull, (unsigned long long)key);
    if (prev == 0 || prev == key) {
      atomicOr(&slots[slot].mask, 1ull << block_bit(s.y, s.z, s.w));
      mine = (int32_t)slot;
      break;
    }
    slot = (slot + 1) & smask;
  }
  site_slot[i] = mine;
}

// payload ranges: a workgroup takes 1024 slots, four per lane, and one atomicAdd for all of them (one per wave was
// 4096 returning atomics on one address at 100k sites: 43 us).  The order of the ranges is free: nbr does not depend
// on it.  The grid covers the slots exactly (a power of two >= 1024).
__global__ __launch_bounds__(256) void bt_base_kernel(BlockSlot* slots, int32_t* counter) {
  __shared__ int s_wave[4];
  __shared__ int s_start;
  const int64_t s0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt[4], mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { cnt[j] = __popcll(slots[s0 + j * 256].mask); mine += cnt[j]; }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_start = total ? atomicAdd(counter, total) : 0;
  }
  __syncthreads();
  int at = s_start + incl - mine;
  for (int w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (cnt[j]) slots[s0 + j * 256].base = at;
    at += cnt[j];
  }
}

__global__ void bt_payload_kernel(const int32_t* __restrict__ idx, int64_t n, const BlockSlot* __restrict__ slots,
                                  const int32_t* __restrict__ site_slot, uint32_t* payload) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t slot = site_slot[i];
  if (slot < 0) return;
  const int4 s = reinterpret_cast<const int4*>(idx)[i];
  const unsigned long long m = slots[slot].mask;
  const int bit = block_bit(s.y, s.z, s.w);
  // the ranges of bt_base_kernel are disjoint and sum to the number of distinct voxels (<= n), and this site's bit is
  // set in m: base + rank < n
  const int at = slots[slot].base + __popcll(m & ((1ull << bit) - 1));
  atomicMax(&payload[at], ~(uint32_t)i);   // duplicate coordinates keep the smallest row, as ht_insert_kernel does
}

// A workgroup serves SITES consecutive sites: its first lanes resolve the candidate blocks of each site once (NB per
// axis: a span of k voxels touches 2 blocks for k <= 5, 3 for k = 7), then all lanes walk the SITES * k^3 entries of
// the output in order - every entry is written exactly once, in coalesced rows, -1 included: no pre-fill.  A payload
// index is base + rank of a slot whose key matched and whose bit is set, so it is < n by the invariant above.
template <int K, int SITES>
__global__ __launch_bounds__(256) void bt_neighbors_kernel(const int32_t* __restrict__ idx, int64_t n,
                                                           const BlockSlot* __restrict__ slots, uint64_t smask,
                                                           const uint32_t* __restrict__ payload,
                                                           int32_t* __restrict__ nbr) {
  constexpr int KVOL = K * K * K, H = K / 2, NB = K <= 5 ? 2 : 3, NC = NB * NB * NB;
  constexpr int ITER = (SITES * KVOL + 255) / 256;
  __shared__ int4 s_site[SITES];
  __shared__ unsigned long long s_mask[SITES * NC];
  __shared__ int32_t s_base[SITES * NC];
  const int64_t i0 = (int64_t)blockIdx.x * SITES;
  for (int c = threadIdx.x; c < SITES * NC; c += 256) {
    const int s = c / NC, cc = c - s * NC;
    unsigned long long m = 0;
    int32_t base = 0;
    if (i0 + s < n) {
      const int4 p = reinterpret_cast<const int4*>(idx)[i0 + s];
      if (cc == 0) s_site[s] = p;
      const int cx = cc / (NB * NB), cy = (cc / NB) % NB, cz = cc % NB;
      const int bx0 = (p.y - H) >> 2, by0 = (p.z - H) >> 2, bz0 = (p.w - H) >> 2;   // -1 at the lower bound
      const int bx = bx0 + cx, by = by0 + cy, bz = bz0 + cz;
      if (bx >= 0 && by >= 0 && bz >= 0 && bx <= ((p.y + H) >> 2) && by <= ((p.z + H) >> 2) &&
          bz <= ((p.w + H) >> 2) && bx < 16384 && by < 16384 && bz < 16384) {
        const int64_t slot = bt_find(slots, smask, p.x, bx, by, bz);
        if (slot >= 0) { m = slots[slot].mask; base = slots[slot].base; }
      }
    }
    s_mask[c] = m;
    s_base[c] = base;
  }
  __syncthreads();
  int32_t v[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int t = threadIdx.x + it * 256;
    const int s = t / KVOL, d = t - s * KVOL;
    v[it] = -1;
    if (t < SITES * KVOL && i0 + s < n) {
      const int4 p = s_site[s];
      const int x = p.y + d / (K * K) - H, y = p.z + (d / K) % K - H, z = p.w + d % K - H;
      if (d == KVOL / 2) {
        v[it] = (int32_t)(i0 + s);   // the centre tap is the site itself
      } else if (x >= 0 && y >= 0 && z >= 0 && x < 65536 && y < 65536 && z < 65536) {
        const int c = s * NC + (((x >> 2) - ((p.y - H) >> 2)) * NB + ((y >> 2) - ((p.z - H) >> 2))) * NB +
                      ((z >> 2) - ((p.w - H) >> 2));
        const unsigned long long m = s_mask[c];
        const int bit = block_bit(x, y, z);
        if ((m >> bit) & 1) v[it] = (int32_t)~payload[s_base[c] + __popcll(m & ((1ull << bit) - 1))];
      }
    }
  }
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int t = threadIdx.x + it * 256;
    if (t < SITES * KVOL && i0 + t / KVOL < n) nbr[i0 * KVOL + t] = v[it];
  }
}

// ---- halo plan (halo_plan.h) -------------------------------------------------------------------------------------
// One workgroup per tile of HALO_T sites: the tile's 128 x 27 table entries are de-duplicated in an LDS hash
// (compare-and-swap, linear probing: at most 3456 keys in 4096 cells), the occupied cells are numbered by a prefix sum
// over the cells - so the numbering depends on the keys alone, not on which lane won a cell - and every (site, tap)
// gets the number of its row's cell.  Nothing is read back: the count stays on the device for the convolution.
constexpr int HALO_HASH = 4096;
__global__ __launch_bounds__(256) void halo_plan_kernel(const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ row_order, int64_t n, HaloPlan p) {
  constexpr int ENT = HALO_T * HALO_TAPS, PER = (ENT + 255) / 256, CELLS = HALO_HASH / 256;
  __shared__ int32_t s_key[HALO_HASH];
  __shared__ uint16_t s_slot[HALO_HASH];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tile = blockIdx.x, row0 = tile * HALO_T;
  for (int c = tid; c < HALO_HASH; c += 256) s_key[c] = -1;
  // entry e = tid + 256 u of the tile's table: all row lookups, then all table reads, in flight together
  int64_t orow[PER];
  bool in[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = tid + 256 * u;
    const int64_t r = row0 + e / HALO_TAPS;
    in[u] = e < ENT && r < n;
    const int64_t rs = in[u] ? r : 0;
    orow[u] = row_order ? (int64_t)row_order[rs] : rs;
  }
  int32_t v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = tid + 256 * u;
    v[u] = nbr[orow[u] * HALO_TAPS + e % HALO_TAPS];
    if (!in[u]) v[u] = -1;
  }
  __syncthreads();
  int cell[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    cell[u] = -1;
    if (v[u] < 0) continue;
    unsigned hsh = ((unsigned)v[u] * 2654435761u) >> 20;   // 12 bits
    for (int probe = 0; probe < HALO_HASH; ++probe) {
      // most entries repeat a row another site has inserted already (16 present taps per site, 2 distinct rows): a
      // plain read finds those without a compare-and-swap on a contended cell
      int32_t prev = *(volatile int32_t*)&s_key[hsh];
      if (prev == -1) prev = atomicCAS(&s_key[hsh], -1, v[u]);
      if (prev == -1 || prev == v[u]) { cell[u] = (int)hsh; break; }
      hsh = (hsh + 1) & (HALO_HASH - 1);
    }
  }
  __syncthreads();
  // thread t owns cells t, t + 256, ...; slots are numbered thread-major
  int mine = 0;
#pragma unroll
  for (int j = 0; j < CELLS; ++j) mine += s_key[tid + 256 * j] >= 0;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int at = incl - mine;
  for (int wv = 0; wv < wave; ++wv) at += s_wave[wv];
#pragma unroll
  for (int j = 0; j < CELLS; ++j) {
    const int32_t key = s_key[tid + 256 * j];
    if (key < 0) continue;
    s_slot[tid + 256 * j] = (uint16_t)at;                    // at < 3456 < HALO_ABSENT
    if (at < HALO_CAP) p.rows[tile * HALO_CAP + at] = key;
    ++at;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = tid + 256 * u;
    if (e < ENT) p.slots[tile * ENT + e] = cell[u] >= 0 ? s_slot[cell[u]] : (uint16_t)HALO_ABSENT;
  }
  if (tid == 0) p.count[tile] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

}  // namespace ptv3

using namespace ptv3;

extern "C" int64_t ptv3_subm_table_slots(int64_t n) {
  int64_t s = 1024;
  while (s < 2 * n) s <<= 1;
  return s;
}

extern "C" int ptv3_subm_build_table(const int32_t* indices, int64_t n, void* table, int64_t slots,
                                     void* stream) {
  PTV3_REQUIRE(slots >= 2 * n && (slots & (slots - 1)) == 0, "subm_build_table: slots must be a power of two >= 2n");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)table;
  int32_t* vals = (int32_t*)((char*)table + slots * 8);
  if (hipMemsetAsync(keys, 0xFF, (size_t)slots * 8, s) != hipSuccess) {
    set_error("subm_build_table: memset failed");
    return PTV3_ERR_LAUNCH;
  }
  if (hipMemsetAsync(vals, 0x7F, (size_t)slots * 4, s) != hipSuccess) {
    set_error("subm_build_table: memset failed");
    return PTV3_ERR_LAUNCH;
  }
  if (n == 0) return PTV3_OK;
  hipLaunchKernelGGL(ht_insert_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, indices, n, keys, vals,
                     (uint64_t)(slots - 1));
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_subm_neighbors(const int32_t* indices, int64_t n, const void* table, int64_t slots,
                                   int ksize, int32_t* nbr, void* stream) {
  PTV3_REQUIRE(ksize >= 1 && ksize <= 7 && (ksize & 1), "subm_neighbors: ksize %d must be odd and <= 7", ksize);
  if (n == 0) return PTV3_OK;
  const int kvol = ksize * ksize * ksize;
  const unsigned long long* keys = (const unsigned long long*)table;
  const int32_t* vals = (const int32_t*)((const char*)table + slots * 8);
  const char* sym = getenv("PTV3_NBR_SYMMETRIC");      // 0: every tap probed (the checker of the symmetric fill)
  if (sym && atoi(sym) == 0) {
    hipLaunchKernelGGL(ht_neighbors_kernel, dim3((unsigned)cdiv(n * kvol, 256)), dim3(256), 0,
                       (hipStream_t)stream, indices, n, keys, vals, (uint64_t)(slots - 1), ksize, kvol, nbr);
  } else {
    if (hipMemsetAsync(nbr, 0xFF, (size_t)n * kvol * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
      set_error("subm_neighbors: memset failed");
      return PTV3_ERR_LAUNCH;
    }
    int sl = 0;
    while ((1 << sl) < kvol / 2 + 1) ++sl;          // 1: 0, 3^3: 4, 5^3: 6, 7^3: 8
    hipLaunchKernelGGL(ht_neighbors_half_kernel, dim3((unsigned)cdiv(n, 256 >> sl)), dim3(256), 0,
                       (hipStream_t)stream, indices, n, keys, vals, (uint64_t)(slots - 1), ksize, kvol, sl, nbr);
  }
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" size_t ptv3_subm_block_table_bytes(int64_t n) {
  if (n < 0) n = 0;
  return (size_t)ptv3_subm_table_slots(n) * sizeof(BlockSlot) + 2 * bt_payload_bytes(n) + 16;
}

extern "C" int ptv3_subm_sites(const int64_t* batch, const void* grid_coord, int coord_is_i64, int64_t n,
                               int32_t* indices, int64_t* grid64, void* table, size_t bytes, void* stream) {
  PTV3_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "subm_sites: n=%lld out of range", (long long)n);
  PTV3_REQUIRE(table && bytes >= ptv3_subm_block_table_bytes(n) && ((uintptr_t)table & 15) == 0,
               "subm_sites: table must be 16-byte aligned and hold ptv3_subm_block_table_bytes(n) bytes");
  PTV3_REQUIRE(n == 0 || (batch && grid_coord && indices), "subm_sites: batch, grid_coord and indices are required");
  PTV3_REQUIRE(((uintptr_t)indices & 15) == 0, "subm_sites: indices must be 16-byte aligned");
  const BlockTable t = bt_layout(table, n);
  hipLaunchKernelGGL(bt_sites_kernel, dim3((unsigned)cdiv(n > 0 ? n : 1, 256)), dim3(256), 0, (hipStream_t)stream, batch,
                     grid_coord, coord_is_i64, n, indices, grid64, (uint4*)table, (int64_t)(t.zero_bytes / 16));
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

// zeroed: the table's first zero_bytes are already zero on the stream (ptv3_subm_sites)
static int build_block_table(const int32_t* indices, int64_t n, void* table, size_t bytes, bool zeroed, void* stream) {
  PTV3_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "subm_build_block_table: n=%lld out of range", (long long)n);
  PTV3_REQUIRE(table && bytes >= ptv3_subm_block_table_bytes(n) && ((uintptr_t)table & 15) == 0,
               "subm_build_block_table: table must be 16-byte aligned and hold ptv3_subm_block_table_bytes(n) bytes");
  PTV3_REQUIRE(n == 0 || indices, "subm_build_block_table: indices are required");
  hipStream_t s = (hipStream_t)stream;
  const BlockTable t = bt_layout(table, n);
  if (!zeroed && hipMemsetAsync(table, 0, t.zero_bytes, s) != hipSuccess) {
    set_error("subm_build_block_table: memset failed");
    return PTV3_ERR_LAUNCH;
  }
  if (n == 0) return PTV3_OK;
  const dim3 sites((unsigned)cdiv(n, 256)), block(256);
  hipLaunchKernelGGL(bt_claim_kernel, sites, block, 0, s, indices, n, t.slots, t.smask, t.site_slot);
  hipLaunchKernelGGL(bt_base_kernel, dim3((unsigned)((t.smask + 1) / 1024)), block, 0, s, t.slots, t.counter);
  hipLaunchKernelGGL(bt_payload_kernel, sites, block, 0, s, indices, n, t.slots, t.site_slot, t.payload);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" int ptv3_subm_build_block_table(const int32_t* indices, int64_t n, void* table, size_t bytes,
                                           void* stream) {
  return build_block_table(indices, n, table, bytes, false, stream);
}

extern "C" int ptv3_subm_build_block_table_zeroed(const int32_t* indices, int64_t n, void* table, size_t bytes,
                                                  void* stream) {
  return build_block_table(indices, n, table, bytes, true, stream);
}

template <int K, int SITES>
static void bt_neighbors_launch(const int32_t* indices, int64_t n, const BlockTable& t, int32_t* nbr, hipStream_t s) {
  hipLaunchKernelGGL((bt_neighbors_kernel<K, SITES>), dim3((unsigned)cdiv(n, SITES)), dim3(256), 0, s, indices, n,
                     t.slots, t.smask, t.payload, nbr);
}

extern "C" int ptv3_subm_neighbors_blocks(const int32_t* indices, int64_t n, const void* table, size_t bytes,
                                          int ksize, int32_t* nbr, void* stream) {
  PTV3_REQUIRE(ksize >= 1 && ksize <= 7 && (ksize & 1), "subm_neighbors_blocks: ksize %d must be odd and <= 7", ksize);
  PTV3_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "subm_neighbors_blocks: n=%lld out of range", (long long)n);
  PTV3_REQUIRE(table && bytes >= ptv3_subm_block_table_bytes(n) && ((uintptr_t)table & 15) == 0,
               "subm_neighbors_blocks: table must be the one ptv3_subm_build_block_table built for these n sites");
  if (n == 0) return PTV3_OK;
  PTV3_REQUIRE(indices && nbr, "subm_neighbors_blocks: indices and nbr are required");
  const BlockTable t = bt_layout(const_cast<void*>(table), n);
  hipStream_t s = (hipStream_t)stream;
  // sites per workgroup: several independent payload reads per lane and a wave or more of block lookups; measured
  // flat around these at 100k sites (5^3: 40.0 / 34.2 / 33.5 / 36.4 us at 4 / 8 / 16 / 32 sites; 3^3: 12.3 / 12.1 /
  // 13.4 / 16.2 us at 16 / 32 / 64 / 128), the smaller choice keeps the deeper levels' few thousand sites spread out
  by_value<1, 3, 5, 7>(ksize, [&](auto K) {
    bt_neighbors_launch<K(), K() == 1 ? 256 : K() == 7 ? 4 : 16>(indices, n, t, nbr, s);
  });
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}

extern "C" size_t ptv3_halo_plan_bytes(int64_t m) { return halo_plan_bytes(m); }

extern "C" int ptv3_halo_plan_shape(int* tile_sites, int* cap_rows) {
  if (tile_sites) *tile_sites = HALO_T;
  if (cap_rows) *cap_rows = HALO_CAP;
  return PTV3_OK;
}

extern "C" int ptv3_halo_plan_build(const int32_t* nbr, const int32_t* row_order, int64_t m, void* plan, size_t bytes,
                                    void* stream) {
  PTV3_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "halo_plan_build: m=%lld out of range", (long long)m);
  if (m == 0) return PTV3_OK;
  PTV3_REQUIRE(nbr != nullptr, "halo_plan_build: the 27-tap neighbour table is required");
  PTV3_REQUIRE(plan && bytes >= halo_plan_bytes(m) && ((uintptr_t)plan & 15) == 0,
               "halo_plan_build: plan must be 16-byte aligned and hold ptv3_halo_plan_bytes(m) bytes");
  const HaloPlan p = halo_layout(plan, m);
  hipLaunchKernelGGL(halo_plan_kernel, dim3((unsigned)p.tiles), dim3(256), 0, (hipStream_t)stream, nbr, row_order, m, p);
  PTV3_LAUNCH_CHECK();
  return PTV3_OK;
}
