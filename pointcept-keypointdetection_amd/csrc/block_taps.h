// Taps of a k^3 submanifold neighbourhood (k <= 5) resolved from the table of 4 x 4 x 4 blocks (hashtable.h, built by
// sparse.hip), for kernels that keep a tile's neighbour rows in LDS instead of reading a table from memory
// (conv_stem.hip).  The rules are those of bt_neighbors_kernel (sparse.hip): a span of k voxels touches at most two
// blocks per axis, a site's up-to-8 candidate blocks are looked up once, every tap is then a bit test and a rank in a
// candidate's mask - taken here per line of k taps along z, which share the 64-bit work.  A tap outside [0, 65536) per
// axis lies in a block outside [0, 16384), whose candidate is dead (mask 0); a tap in an unoccupied voxel or in
// another batch id (the batch id is part of the block key) finds no bit.
#pragma once
#include "hashtable.h"

namespace ptv3 {

constexpr int BT_NB = 2;                       // candidate blocks per axis of a span of k <= 5 voxels
constexpr int BT_NC = BT_NB * BT_NB * BT_NB;   // candidate blocks per site

// Candidate cc (0 .. 7) of site p = (batch, x, y, z) at half width h = k / 2: whether its block can hold a tap, and the
// slot of the table where the probe for it starts.  A dead candidate names slot 0, which every table has.
__device__ __forceinline__ bool bt_candidate(const int4 p, int h, int cc, uint64_t smask, uint64_t& key, uint64_t& slot) {
  const int cx = cc / (BT_NB * BT_NB), cy = (cc / BT_NB) % BT_NB, cz = cc % BT_NB;
  const int bx = ((p.y - h) >> 2) + cx, by = ((p.z - h) >> 2) + cy, bz = ((p.w - h) >> 2) + cz;   // -1 at the lower bound
  const bool live = bx >= 0 && by >= 0 && bz >= 0 && bx <= ((p.y + h) >> 2) && by <= ((p.z + h) >> 2) &&
                    bz <= ((p.w + h) >> 2) && bx < 16384 && by < 16384 && bz < 16384;
  key = block_key(p.x, bx, by, bz);
  slot = live ? mix64(key) & smask : 0;
  return live;
}

// The probe that follows a first slot which held another block's key (rare: the table is at most half full): mask and
// base of the block `key`, or mask 0.
__device__ __forceinline__ void bt_probe_on(const BlockSlot* __restrict__ slots, uint64_t smask, uint64_t key, uint64_t slot,
                                            unsigned long long& m, int32_t& base) {
  m = 0; base = 0;
  for (uint64_t probe = 1; probe <= smask; ++probe) {
    slot = (slot + 1) & smask;
    const unsigned long long kq = slots[slot].key;
    if (kq == key) { m = slots[slot].mask; base = slots[slot].base; return; }
    if (kq == 0) return;
  }
}

// The K taps (dx, dy, 0 .. K-1) of site p, a line along z: which voxels of it are occupied (bit zr of `occ`, zr counted
// from the first voxel of candidate z-block 0) and the payload index in front of the line's row in either z-block.
struct BtLine { unsigned occ; int below[2]; int zr0; };
__device__ __forceinline__ void bt_line(const int4 p, int h, int dx, int dy, const unsigned long long* __restrict__ cmask,
                                        const int32_t* __restrict__ cbase, BtLine& ln) {
  const int x = p.y + dx - h, y = p.z + dy - h;
  const int cxy = ((((x >> 2) - ((p.y - h) >> 2)) & 1) * BT_NB + (((y >> 2) - ((p.z - h) >> 2)) & 1)) * BT_NB;
  const int sh = ((x & 3) << 4) | ((y & 3) << 2);   // the row's four voxels are bits sh .. sh + 3 of a block's mask
  const unsigned long long m0 = cmask[cxy], m1 = cmask[cxy + 1];
  ln.occ = ((unsigned)(m0 >> sh) & 15u) | (((unsigned)(m1 >> sh) & 15u) << 4);
  ln.below[0] = cbase[cxy] + __popcll(m0 & ((1ull << sh) - 1));
  ln.below[1] = cbase[cxy + 1] + __popcll(m1 & ((1ull << sh) - 1));
  ln.zr0 = (p.w - h) & 3;
}
// tap i of the line: present, and then its payload index
__device__ __forceinline__ bool bt_line_tap(const BtLine& ln, int i, int& rank) {
  const int zr = ln.zr0 + i;                        // 0 .. 7
  const unsigned row = zr < 4 ? ln.occ & 15u : ln.occ >> 4;
  rank = (zr < 4 ? ln.below[0] : ln.below[1]) + __popc(row & ((1u << (zr & 3)) - 1));
  return (ln.occ >> zr) & 1;
}

}  // namespace ptv3
