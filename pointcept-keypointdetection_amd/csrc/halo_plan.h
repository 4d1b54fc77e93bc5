// Halo plan of a 3^3 submanifold convolution (built in sparse.hip, read by conv_halo_kernel in gemm.hip).
// The sites of a level, taken in row_order, are cut into tiles of HALO_T consecutive sites.  Per tile the plan holds
//   count            number of DISTINCT neighbour rows of the tile's sites (the sites themselves included)
//   rows[HALO_CAP]   those rows, in slot order (only the first min(count, HALO_CAP) entries are written)
//   slots[HALO_T][27] per (site, tap) the 16-bit slot of the neighbour's row in `rows`, HALO_ABSENT for no neighbour
// A tile with count > HALO_CAP overflows: its slots are still numbered, its row list is cut, and the convolution
// gathers it per tap from global memory instead.
//   count: tiles x int32 (padded to 16 bytes) | rows: tiles x HALO_CAP x int32 | slots: tiles x HALO_T x 27 x uint16
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ptv3 {

// One (T, CAP) for every dtype and width, so that the four convolutions of a level share one plan.  CAP is what the LDS
// of two workgroups per CU leaves at C = 64 in bf16: 433 rows x 128 bytes + two weight taps (16 KB) + the slot table
// (6.75 KB) + the epilogue vectors are 77.6 KB of the 80 KB a workgroup may take.  On the 100k-point surface scene
// (tools/replay_halo.py) a 128-site tile has 266 distinct rows on average, 364 at the 99th percentile and 432 at most.
// (CAP = 384 leaves 0.5 % of that scene's tiles, four workgroups, to the per-tap path; measured: profiles/halo_conv.)
constexpr int HALO_T = 128;
constexpr int HALO_CAP = 432;
constexpr int HALO_TAPS = 27;
constexpr unsigned HALO_ABSENT = 0xFFFFu;

struct HaloPlan { int32_t* count; int32_t* rows; uint16_t* slots; int64_t tiles; };

static inline int64_t halo_tiles(int64_t m) { return (m + HALO_T - 1) / HALO_T; }
static inline size_t halo_count_bytes(int64_t tiles) { return ((size_t)tiles * 4 + 15) & ~(size_t)15; }
static inline size_t halo_plan_bytes(int64_t m) {
  const int64_t t = halo_tiles(m < 0 ? 0 : m);
  return halo_count_bytes(t) + (size_t)t * HALO_CAP * 4 + (size_t)t * HALO_T * HALO_TAPS * 2;
}
static inline HaloPlan halo_layout(void* plan, int64_t m) {
  HaloPlan p;
  p.tiles = halo_tiles(m);
  char* b = (char*)plan;
  p.count = (int32_t*)b;
  p.rows = (int32_t*)(b + halo_count_bytes(p.tiles));
  p.slots = (uint16_t*)(b + halo_count_bytes(p.tiles) + (size_t)p.tiles * HALO_CAP * 4);
  return p;
}

}  // namespace ptv3
